"""A rigid instrument -- a capsule with a sphere at its tip -- is lowered onto a clamped beam and dragged along it with friction.

    python examples/tool_pushes.py [--n 12] [--lower 25] [--drag 25] [--out DIR]

A beam of n x 4 x 4 nodes is clamped at one end.  Every step the tool moves a little, ``Deformable.set_tool`` hands its shapes (the
tuples of fembrain_amd/erosion.py), its reference point and its velocity to the body, and ``timestep`` applies it behind gravity:
fb_fem_tool_contact pushes every surface vertex the tool holds out along the shape's normal, on the device, and returns the force and
the torque the tissue gives back to the tool -- the wrench a haptic device renders -- which the loop prints.  While the tool is dragged,
regularised Coulomb friction (``mu``, ``slip_speed``) takes the tissue along and pulls the tool back.

The penalty spring and the friction are explicit: stiffness * dt^2 and mu * N / slip_speed * dt stay below the mass a contact pushes
(a top-face node carries rho h^3 / 2 = 0.5 kg here; the run prints both).  The reference has only the probe's axis-aligned box.
Writes the drawn surface before, pressed and dragged as .obj (fb_fem_surface / fb_fem_surface_update) where --out names a directory."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd.fem import Deformable  # noqa: E402
from fembrain_amd.meshgen import truth_cube  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=12)
ap.add_argument("--lower", type=int, default=25)
ap.add_argument("--drag", type=int, default=25)
ap.add_argument("--out", default=None)
args = ap.parse_args()

H, DT = 0.1, 0.005            # cell, time step
STIFFNESS = 8000.0            # stiffness * DT^2 = 0.2 kg
MU, SLIP, DAMPING = 0.3, 0.5, 20.0
RADIUS, SHAFT = 0.12, 0.08    # the tip's sphere and the capsule behind it
STEP = 0.04 * H               # the tool's travel per step, lowering and dragging


def write_obj(path, it):
    s = it.surface()
    xyz = it.surface_update()[0]
    local = np.full(it.n_nodes, -1, np.int64)
    local[s["vertex_ids"]] = np.arange(len(s["vertex_ids"]))
    with open(path, "w") as f:
        for p in xyz:
            f.write("v %.9g %.9g %.9g\n" % tuple(p))
        for tri in local[s["faces"]] + 1:
            f.write("f %d %d %d\n" % tuple(tri))


def tool(tip):
    """the shapes with the sphere's centre at tip, the shaft rising from it, leaning back a little"""
    tip = np.asarray(tip, np.float64)
    return [("sphere", tuple(tip), RADIUS), ("capsule", tuple(tip), tuple(tip + [-0.1, 0.5, 0.0]), SHAFT)]


n = args.n
v, t = truth_cube(n, 4, 4, H)
body = Deformable(v, t, fixed_vertices=np.arange(16), gravity=False, E=1e6, timestep=DT)
it = body.integrator
if args.out:
    os.makedirs(args.out, exist_ok=True)
    write_obj(os.path.join(args.out, "before.obj"), it)

top = v[:, 1].max()
tip = np.array([v[:, 0].min() + 0.6 * (v[:, 0].max() - v[:, 0].min()), top + RADIUS, 0.5 * (v[:, 2].min() + v[:, 2].max())])
print("explicit bounds: stiffness dt^2 = %.3f kg, a top-face node carries %.3f kg" % (STIFFNESS * DT * DT, 1000.0 * H ** 3 / 2))
pressed = dragged = None
for k in range(1, args.lower + args.drag + 1):
    lowering = k <= args.lower
    move = np.array([0.0, -STEP, 0.0]) if lowering else np.array([STEP, 0.0, 0.0])
    tip = tip + move
    body.set_tool(tool(tip), STIFFNESS, origin=tuple(tip), velocity=tuple(move / DT), mu=MU, slip_speed=SLIP, damping=DAMPING)
    body.timestep()
    assert it.last.converged == 1
    info = body.last_tool_contact
    if k % 5 == 0 or k in (args.lower, args.lower + args.drag):
        print("step %3d (%s): %2d contacts, depth %.4f, force on the tool (%8.2f, %8.2f, %8.2f), torque (%7.3f, %7.3f, %7.3f), stick rate dt %.3f kg" % (
            (k, "lower" if lowering else "drag ", info["n_contacts"], info["max_depth"]) + tuple(info["force_on_tool"]) + tuple(info["torque_on_tool"])
            + (info["max_stick_rate"] * DT,)))
    if k == args.lower:
        pressed = info
        if args.out:
            write_obj(os.path.join(args.out, "pressed.obj"), it)
dragged = body.last_tool_contact
if args.out:
    write_obj(os.path.join(args.out, "dragged.obj"), it)
body.clear_tool()
q = it.get_q_state()[0].reshape(-1, 3)
travel = args.lower * STEP
print("RESULT contacts=%d travel=%.17g depth=%.17g fy_pressed=%.17g fx_dragged=%.17g fy_dragged=%.17g sag=%.17g along=%.17g" % (
    dragged["n_contacts"], travel, pressed["max_depth"], pressed["force_on_tool"][1], dragged["force_on_tool"][0], dragged["force_on_tool"][1],
    float(q[:, 1].min()), float(q[:, 0].max())))
it.close()
assert pressed["n_contacts"] > 0 and pressed["force_on_tool"][1] > 0 and pressed["max_depth"] < travel
assert dragged["force_on_tool"][0] < 0      # the tissue holds the tool back
print("tool pushes ok")
