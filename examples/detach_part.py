"""A piece is cut off a bending beam and goes on as a body of its own, with the motion it had -- made on the device, never on the host.

    python examples/detach_part.py

A clamped beam of 16 x 5 x 5 nodes is loaded and stepped until it bends.  It is cut through mid-span with FB_CUT_CARRY (rest shape
and state kept), the cut is opened (fb_fem_split_parts), and the free part is detached with removal (fb_fem_detach_part,
FB_DETACH_REMOVE: what the reference's CuttableMesh::convertDisjointPartsToMeshes does with a part).  The piece starts with the
displacement and the velocity its nodes had in the beam; the stump loses the piece's elements and keeps its own state; the volumes of
the two add up to the beam's.  Both bodies step on under the same load: where examples/split_parts.py had to start its piece at
rest and keep simulating it in the parent as well, here the tissue is simulated once."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402

v, t = truth_cube(16, 5, 5, 0.1)
fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(5, 5))
beam = FemIntegrator(v, t, fixed, expect_cuts=True)
for _ in range(5):
    beam.set_uniform_force(1, -60.0)
    beam.do_timestep()
tip = float(beam.get_q_state()[0].reshape(-1, 3)[:, 1].min())
assert tip < -1e-4
print("the beam bends: largest deflection %.4g" % -tip)

# the blade: a plane across mid-span, tilted a little so that it passes through no node
nrm = np.array([1.0, 0.02, 0.013])
nrm /= np.linalg.norm(nrm)
a = np.cross(nrm, [0.0, 1.0, 0.0])
a /= np.linalg.norm(a)
b = np.cross(nrm, a)
p = v.min(0) + (v.max(0) - v.min(0)) * np.array([0.51, 0.5, 0.5])
quad = np.array([p - 5 * a - 5 * b, p - 5 * a + 5 * b, p + 5 * a - 5 * b, p + 5 * a + 5 * b])
info, _ = beam.cut(quad, mode="carry", track=False)
assert info["status"] == fl.FB_CUT_DONE, info
assert beam.parts()["n_parts"] == 2
split = beam.split_parts(quad, 0.05, track=False)
assert split["n_front_parts"] == 1 and split["n_back_parts"] == 1, split

volume_before = beam.part_table()["volume"].sum()
q, qvel, _ = beam.get_q_state()
n_before = beam.num_tets()
free = 1 - int(beam.element_parts()[0])          # the part that does not hold element 0, which sits at the clamp
piece, ids, nodes = beam.detach_part(free, remove=True)
info = piece.detach_info
print("detached part %d: %d elements on %d nodes, %d constrained DOFs; the stump keeps %d elements (re-sync path %d)"
      % (free, info["n_elements"], info["n_nodes"], info["n_fixed_dofs"], info["parent_elements_left"], info["parent_resync_path"]))
assert info["n_fixed_dofs"] == 0 and info["n_elements"] + info["parent_elements_left"] == n_before

# the piece starts with the displacement and the velocity it had
pq, pv, _ = piece.get_q_state()
assert np.array_equal(pq, q.reshape(-1, 3)[nodes].reshape(-1)) and np.array_equal(pv, qvel.reshape(-1, 3)[nodes].reshape(-1))
assert np.abs(pq).max() > 1e-4 and np.abs(pv).max() > 0
# ... the stump keeps its own, and the two volumes are the beam's
sq, sv, _ = beam.get_q_state()
assert np.array_equal(sq, q) and np.array_equal(sv, qvel)
assert beam.parts()["n_parts"] == 1 and piece.parts()["n_parts"] == 1
volume_stump, volume_piece = beam.part_table()["volume"].sum(), piece.part_table()["volume"].sum()
assert abs(volume_stump + volume_piece - volume_before) <= 1e-12 * volume_before
print("volumes: stump %.6f + piece %.6f = %.6f" % (volume_stump, volume_piece, volume_before))

y0 = float(pq.reshape(-1, 3)[:, 1].mean())
for _ in range(3):
    for body in (beam, piece):
        body.set_uniform_force(1, -60.0)
        body.do_timestep()
        assert body.last.converged == 1
y1 = float(piece.get_q_state()[0].reshape(-1, 3)[:, 1].mean())
assert y1 < y0
print("both bodies step on: the piece fell from %.4g to %.4g" % (y0, y1))
beam.close()
piece.close()
print("detach part ok")
