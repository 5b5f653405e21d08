"""A block pushed sideways on another: without friction it glides off like a free body, with friction above the load ratio it stays.

    python examples/friction_holds.py [--steps 40] [--stiffness 4000] [--damping 40] [--slip-speed 0.15]

A small block (4 x 4 x 4 nodes, 27 kg) rests on a wider one that is clamped along its bottom plane.  Both carry a uniform downward
load per node -- 384 N on the small block -- and the small block also a uniform sideways load of 0.1 of it.  fb_fem_body_contact runs
once per step, after both bodies have their loads and before they step.  Three runs of the same steps:
  mu = 0      the contact is frictionless: the block glides sideways like a free body under the sideways load;
  mu = 0.5    above the load ratio: the block is held (it creeps, because the friction law is regularised: below slip_speed the
              friction is a damper, so a held block moves at slip_speed * load ratio / mu);
  mu = 0.05   below the load ratio: the block slides, slower than the free one.

The contact forces enter the implicit step as external forces, that is explicitly (fembrain_hip.h, "Friction and damping of a
contact"): (stiffness x contacts) dt^2, mu N / slip_speed dt and damping dt all stay below the mass they push.  For the 27 kg block
under 384 N with mu = 0.5 and dt = 0.01 the second bound asks for slip_speed >= 0.5 * 384 * 0.01 / 27 = 0.071; 0.15 it is.  The
damping settles the landing: the block starts at rest about as deep in the lower one as the penalty spring carries it.
Prints the sideways drift of the small block's mean node position for each run."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import fixed_vertices_to_dofs, truth_cube  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--stiffness", type=float, default=4000.0)
ap.add_argument("--damping", type=float, default=40.0)
ap.add_argument("--slip-speed", type=float, default=0.15)
args = ap.parse_args()

DT, RHO, DOWN, RATIO = 0.01, 1000.0, -6.0, 0.1   # seconds | kg / m^3 | force per node, downward | sideways load / downward load
SINK = 0.003                                      # the small block starts so deep in the lower one


def run(mu):
    vu, tu = truth_cube(4, 4, 4, 0.1)
    vl, tl = truth_cube(9, 3, 9, 0.1)
    bottom = np.nonzero(vl[:, 1] == vl[:, 1].min())[0]
    lower = FemIntegrator(vl, tl, fixed_vertices_to_dofs(bottom), rho=RHO, timestep=DT)
    # on top of the lower block, off its grid lines, SINK deep
    vu = vu + np.array([0.0137 - 0.1, vl[:, 1].max() - SINK - vu[:, 1].min(), 0.0171])[None, :]
    upper = FemIntegrator(vu, tu, rho=RHO, timestep=DT)
    side = np.zeros((len(vu), 3))
    side[:, 0], side[:, 1] = -DOWN * RATIO, DOWN
    most, rate = 0, 0.0
    for _ in range(args.steps):
        lower.set_uniform_force(1, DOWN)
        upper.set_external_forces(side.reshape(-1))
        c = upper.body_contact(lower, args.stiffness, mu=mu, slip_speed=args.slip_speed, damping=args.damping)
        most, rate = max(most, sum(c["n_contacts"])), max(rate, c.get("max_stick_rate", 0.0))
        for body in (lower, upper):
            body.do_timestep()
            assert body.last.converged == 1
    q = upper.get_q_state()[0].reshape(-1, 3)
    drift, sunk = float(q[:, 0].mean()), float(q[:, 1].mean())
    lower.close()
    upper.close()
    return drift, sunk, most, rate


mass = RHO * 0.3 ** 3
# the centre of mass of a free body under the total force F moves by F / m dt^2 k (k + 1) / 2 in k implicit Euler steps
free = -DOWN * RATIO * 64 / mass * DT * DT * args.steps * (args.steps + 1) / 2
drifts = {}
for mu in (0.0, 0.5, 0.05):
    drifts[mu], sunk, most, rate = run(mu)
    print("mu = %-4g: the block drifts %.5f sideways in %d steps (%.3f of the free %.5f), sinks %.5f; at most %d contacts, stick rate * dt at most %.2f kg" % (
        mu, drifts[mu], args.steps, drifts[mu] / free, free, -sunk, most, rate * DT))
print("RESULT free=%.17g mu0=%.17g mu05=%.17g mu005=%.17g" % (free, drifts[0.0], drifts[0.5], drifts[0.05]))
assert drifts[0.5] < drifts[0.05] < drifts[0.0]
print("friction holds ok")
