"""A slab cut off the top of a clamped block stays in the same body and comes to rest on the stump: contact of a body with itself.

    python examples/cut_slab_rests.py [--n 6] [--steps 60] [--stiffness 1000]

A block of n x (n + 1) x n nodes, clamped at its base, is cut through horizontally a little above mid-height with fb_fem_cut.  Both
halves stay in ONE handle: the stump holds the clamp, the slab above it holds nothing.  Gravity is a uniform force per node.  Two runs
of the same steps: in one the body collides with itself (``Deformable.set_self_collision(mode="other_parts")``: every ``timestep`` adds
fb_fem_self_contact's forces behind gravity), and the slab settles on the stump a few thousandths of a cell deep; in the other nothing
tells the two halves of each other and the slab sinks through the stump by the free-fall distance.

Right after the cut the lips coincide bit for bit, every contact is at depth 0 and pushes nothing: the slab first falls into the stump
and is then carried.  The penalty forces enter the implicit step as external forces, that is explicitly: the stiffness is chosen so that
(stiffness x contacts) dt^2 / mass of the slab stays below one.  Prints the slab's lowest node height over the stump's top for both."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import Deformable  # noqa: E402
from fembrain_amd.meshgen import truth_cube  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=6)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--stiffness", type=float, default=1000.0)
args = ap.parse_args()

H, DT, RHO, GRAVITY = 0.1, 0.01, 1000.0, -6.0   # cell | seconds | kg / m^3 | force per node


def run(contact):
    n = args.n
    v, t = truth_cube(n, n + 1, n, H)
    base = np.nonzero(v[:, 1] == v[:, 1].min())[0]
    body = Deformable(v, t, fixed_vertices=base, rho=RHO, timestep=DT, expect_cuts=True)
    body.GRAVITY_FORCE = GRAVITY
    # the blade: a plane at 0.53 of the height, tilted a little so that it passes through no node
    nrm = np.array([0.002, 1.0, 0.0013])
    nrm /= np.linalg.norm(nrm)
    a = np.cross(nrm, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    p = v.min(0) + (v.max(0) - v.min(0)) * np.array([0.5, 0.53, 0.5])
    info, _ = body.cut(np.array([p - 5 * a - 5 * b, p - 5 * a + 5 * b, p + 5 * a - 5 * b, p + 5 * a + 5 * b]), mode="carry")
    it = body.integrator
    assert info["status"] == fl.FB_CUT_DONE and it.parts()["n_parts"] == 2, info
    x = it.read_mesh()[0]
    slab = it.node_parts() == 1 - int(it.element_parts()[0])   # the part that does not hold element 0, which sits at the clamp
    top = float(x[~slab, 1].max())                             # the stump's top: the lower lip
    if contact:
        body.set_self_collision(args.stiffness, 0.0, "other_parts")
    most = 0
    for _ in range(args.steps):
        body.timestep()
        assert it.last.converged == 1
        if contact:
            most = max(most, len(it.read_self_contact()["node"]))
    low = float((x + it.get_q_state()[0].reshape(-1, 3))[slab, 1].min()) - top
    it.close()
    return low, most, int(slab.sum())


with_contact, most, n_slab = run(True)
without, _, _ = run(False)
print("the slab (%d nodes) after %d steps, lowest node over the stump's top, in cells:" % (n_slab, args.steps))
print("with self-collision (at most %d contacts in a step): %.4f" % (most, with_contact / H))
print("without: %.4f" % (without / H))
print("RESULT with=%.17g without=%.17g cell=%.17g contacts=%d" % (with_contact, without, H, most))
assert with_contact > -H > without
print("cut slab rests ok")
