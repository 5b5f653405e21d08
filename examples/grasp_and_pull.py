"""A tool closes on the free end of a clamped beam, drags and twists it, reads the force the tissue returns, and lets go.

    python examples/grasp_and_pull.py [--n 12] [--steps 20] [--free 20] [--out DIR]

A beam of n x 4 x 4 nodes is clamped at one end.  The nodes in a box around the other end are found on the device
(``Deformable.pick_vertices`` -> fb_fem_pick_box) and gripped (``grip`` -> fb_fem_grasp: their DOFs join the constrained list and follow
targets from then on).  Every step the tool moves a little further -- along the beam, and turning about the beam's axis -- and
``move_grip`` sets the targets on the device; the step takes the held nodes there bit for bit, the free nodes feel them through the
matrix columns a clamp does not have, and ``grip_force`` is the force the tissue returns to the tool: what a displacement-driven haptic
device is fed.  Then ``release_grip``: the held nodes are free DOFs again with the state they have, and the beam springs back.

What the reference only flags (IAvatar::grip(), src/deformable/IScalpel.cpp:42-44).  Writes the drawn surface before, held and after
as .obj (fb_fem_surface / fb_fem_surface_update) where --out names a directory."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd.fem import Deformable  # noqa: E402
from fembrain_amd.meshgen import truth_cube  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=12)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--free", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

H = 0.1                       # cell
PULL, TWIST = 0.15, 0.5       # cells along the beam and radians about its axis, over all steps


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


n = args.n
v, t = truth_cube(n, 4, 4, H)
body = Deformable(v, t, fixed_vertices=np.arange(16), gravity=False)
it = body.integrator
if args.out:
    os.makedirs(args.out, exist_ok=True)
    write_obj(os.path.join(args.out, "before.obj"), it)

# the jaws: a box around the last plane of nodes
end = v[:, 0].max()
_, held = body.pick_vertices([end - 0.25 * H, v[:, 1].min() - H, v[:, 2].min() - H], [end + 0.25 * H, v[:, 1].max() + H, v[:, 2].max() + H])
info = body.grip(held)
print("gripped %d nodes: %d DOFs follow the tool" % (len(held), info["n_dofs"]))
pivot = v[held].mean(axis=0)
force = np.zeros(3)
for k in range(1, args.steps + 1):
    a = TWIST * k / args.steps
    R = [[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]]
    body.move_grip(R, (PULL * H * k / args.steps, 0.0, 0.0), pivot)
    body.timestep()
    assert it.last.converged == 1
    force = body.grip_force()
    if k % 5 == 0 or k == args.steps:
        print("step %3d: the tissue pulls the tool with (%.1f, %.1f, %.1f)" % ((k,) + tuple(force)))
mi = it.motion_info()
q_held = it.get_q_state()[0].reshape(-1, 3)
want = (v[held] - pivot) @ np.array(R).T + pivot + [PULL * H, 0.0, 0.0] - v[held]
follow = float(np.abs(q_held[held] - want).max())
if args.out:
    write_obj(os.path.join(args.out, "held.obj"), it)

body.release_grip()
for _ in range(args.free):
    body.timestep()
    assert it.last.converged == 1
q_free = it.get_q_state()[0].reshape(-1, 3)
if args.out:
    write_obj(os.path.join(args.out, "after.obj"), it)
print("table: %d elements listed, %d nodes touched, longest run %d, built %d time(s)" % (mi["n_listed_elements"], mi["n_touched_nodes"], mi["longest_run"], mi["table_builds"]))
print("RESULT held=%d follow=%.17g fx=%.17g end_held=%.17g end_free=%.17g builds=%d fixed_after=%d" % (
    len(held), follow, force[0], float(q_held[held, 0].mean()), float(q_free[held, 0].mean()), mi["table_builds"], len(it.constrained_dofs())))
it.close()
assert follow <= 1e-12 and force[0] < 0 and mi["table_builds"] == 1
print("grasp and pull ok")
