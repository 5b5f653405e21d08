"""A piece cut off a beam is dropped onto it: with the contact call it lands, without it falls through.

    python examples/parts_collide.py [--steps 60] [--stiffness 5000]

The clamped beam of examples/detach_part.py (16 x 5 x 5 nodes) is cut through mid-span and its free half detached into a body of its own
(fb_fem_cut, fb_fem_detach_part with removal).  The piece is lifted over the stump, a little above its top, and released at rest under
gravity -- a uniform force per node.  Two runs of the same steps: one calls fb_fem_body_contact once per step, after both bodies have
their gravity and before they step, and the piece comes to lie on the stump; the other does not, and nothing keeps the two apart (the
only other obstacles a body knows are a floor plane and the probe's box): the piece falls through the stump by the free-fall distance.

The penalty forces enter the implicit step as external forces, that is explicitly: the stiffness is chosen so that (stiffness x contacts)
dt^2 / mass of the piece stays below one.  Prints the height of the piece's centroid over the beam's top for both runs."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--stiffness", type=float, default=5000.0)
args = ap.parse_args()

DT, RHO, GRAVITY, GAP = 0.01, 1000.0, -6.0, 0.05   # seconds | kg / m^3 | force per node | the piece starts so far above the beam's top


def run(contact):
    v, t = truth_cube(16, 5, 5, 0.1)
    beam = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(5, 5)), rho=RHO, timestep=DT, expect_cuts=True)
    # the blade: a plane across mid-span, tilted a little so that it passes through no node
    nrm = np.array([1.0, 0.02, 0.013])
    nrm /= np.linalg.norm(nrm)
    a = np.cross(nrm, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    p = v.min(0) + (v.max(0) - v.min(0)) * np.array([0.51, 0.5, 0.5])
    quad = np.array([p - 5 * a - 5 * b, p - 5 * a + 5 * b, p + 5 * a - 5 * b, p + 5 * a + 5 * b])
    info, _ = beam.cut(quad, mode="carry", track=False)
    assert info["status"] == fl.FB_CUT_DONE and beam.parts()["n_parts"] == 2, info
    free = 1 - int(beam.element_parts()[0])          # the part that does not hold element 0, which sits at the clamp
    volume = float(beam.part_table()["volume"][free])
    piece, _, _ = beam.detach_part(free, remove=True)
    # over the stump, GAP above its top, at rest
    x = piece.read_mesh()[0]
    top = float(v[:, 1].max())
    lift = np.array([v[:, 0].min() + 0.02 - x[:, 0].min(), top + GAP - x[:, 1].min(), 0.013])
    piece.set_q_state(np.tile(lift, len(x)), np.zeros(3 * len(x)), np.zeros(3 * len(x)))
    start = float(x[:, 1].mean() + lift[1]) - top
    most = 0
    for _ in range(args.steps):
        for body in (beam, piece):
            body.set_uniform_force(1, GRAVITY)
        if contact:
            c = beam.body_contact(piece, args.stiffness)
            most = max(most, sum(c["n_contacts"]))
        for body in (beam, piece):
            body.do_timestep()
            assert body.last.converged == 1
    end = float((x + piece.get_q_state()[0].reshape(-1, 3))[:, 1].mean()) - top
    # the centre of mass of a free body under the total force F falls by F / m dt^2 k (k + 1) / 2 in k implicit Euler steps
    fall = -GRAVITY * len(x) / (RHO * volume) * DT * DT * args.steps * (args.steps + 1) / 2
    beam.close()
    piece.close()
    return start, end, fall, most


start, with_contact, fall, most = run(True)
_, without, _, _ = run(False)
print("the piece's centroid starts %.4f above the beam's top; free fall over %d steps: %.4f" % (start, args.steps, fall))
print("with contact (at most %d contacts in a step): centroid %.4f over the beam's top" % (most, with_contact))
print("without contact: centroid %.4f over the beam's top" % without)
print("RESULT start=%.17g with=%.17g without=%.17g fall=%.17g contacts=%d" % (start, with_contact, without, fall, most))
assert with_contact > 0 > without
print("parts collide ok")
