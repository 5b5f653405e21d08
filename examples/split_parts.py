"""A piece is cut off, the cut is opened, and the piece goes on as a body of its own -- the parts never return to the host as a whole mesh.

    python examples/split_parts.py [--out OUTDIR]

A clamped beam of 16 x 5 x 5 nodes is cut through mid-span.  The handle counts its disjoint parts on the device (fb_fem_parts: what the
reference's IScalpel does after every cut with VolMesh::get_disjoint_parts), pushes the two sides of the blade's quad 0.05 apart
(fb_fem_split_parts: CuttableMesh::splitParts) and hands the free part over as a mesh (fb_fem_read_part: convertDisjointPartsToMeshes),
of which a second FemIntegrator is made.  Both bodies step under the same load: the clamped stump bends, the free piece falls.  With
--out the two surfaces are written: body.obj (the handle, which keeps both parts, with the cut open) and piece.obj."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402


def write_obj(path, fem):
    s = fem.surface()
    xyz, normals, _ = fem.surface_update()
    compact = np.searchsorted(s["vertex_ids"], s["faces"]) + 1      # faces index node ids; the file indexes the compact vertex list
    with open(path, "w") as fh:
        for p in xyz:
            fh.write("v %.9g %.9g %.9g\n" % tuple(p))
        for n in normals:
            fh.write("vn %.9g %.9g %.9g\n" % tuple(n))
        for a, b, c in compact:
            fh.write("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c))
    return len(s["faces"])


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()

v, t = truth_cube(16, 5, 5, 0.1)
fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(5, 5))
fem = FemIntegrator(v, t, fixed)
print("before the cut: %d part(s) of %d elements" % (fem.parts()["n_parts"], len(t)))

# the blade: a plane across mid-span, tilted a little so that it passes through no node
nrm = np.array([1.0, 0.02, 0.013])
nrm /= np.linalg.norm(nrm)
a = np.cross(nrm, [0.0, 1.0, 0.0])
a /= np.linalg.norm(a)
b = np.cross(nrm, a)
p = v.min(0) + (v.max(0) - v.min(0)) * np.array([0.51, 0.5, 0.5])
quad = np.array([p - 5 * a - 5 * b, p - 5 * a + 5 * b, p + 5 * a - 5 * b, p + 5 * a + 5 * b])
info, _ = fem.cut(quad, track=False)
assert info["status"] == fl.FB_CUT_DONE, info

parts = fem.parts()
table = fem.part_table()
assert parts["n_parts"] == 2 and parts["n_shared_nodes"] == 0, parts
for k in range(parts["n_parts"]):
    print("part %d: %d elements on %d nodes from element %d on, volume %.6f" % (k, table["elements"][k], table["nodes"][k], table["first_element"][k], table["volume"][k]))

split = fem.split_parts(quad, 0.05, track=False)
assert split["n_front_parts"] == 1 and split["n_back_parts"] == 1 and split["n_straddling_parts"] == 0, split
print("the cut opened: %d nodes moved by +-%s" % (split["n_nodes_moved"], split["shift"]))

# the free part: the one that does not hold element 0 (which sits at the clamp)
free = 1 - int(fem.element_parts()[0])
ids, nodes, xyz, tets = fem.read_part(free)
assert not np.isin(nodes, cube_fixed_plane_i0(5, 5)).any()
piece = FemIntegrator(xyz, tets, np.zeros(0, np.int32))
assert piece.parts()["n_parts"] == 1
for _ in range(3):
    for body in (fem, piece):
        body.set_uniform_force(1, -3000.0)
        body.do_timestep()
        assert body.last.converged == 1
dy = piece.get_q_state()[0].reshape(-1, 3)[:, 1]
assert dy.mean() < 0 and dy.std() < 0.05 * abs(dy.mean()), (dy.mean(), dy.std())   # a rigid fall
print("the free piece (%d elements, %d nodes) fell by %.4g, every node alike" % (len(ids), len(nodes), -dy.mean()))
if args.out:
    os.makedirs(args.out, exist_ok=True)
    print("body.obj: %d faces, piece.obj: %d faces" % (write_obj(os.path.join(args.out, "body.obj"), fem), write_obj(os.path.join(args.out, "piece.obj"), piece)))
fem.close()
piece.close()
print("split parts ok")
