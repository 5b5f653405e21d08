"""A probe touches the tissue: pick a surface node, pull it for a few steps, watch the volume -- nothing mesh-sized crosses the bus.

    python examples/haptic_probe.py [n] [steps]

A cantilever of n^3 nodes (default 12) hangs from its clamped face.  The node of its free end closest to a point outside is picked on
the device (fb_fem_pick_vertex: 40 bytes come back), the nodes in a small box around it are listed (fb_fem_pick_box), and for `steps`
steps (default 5) the picked node is pulled: gravity is generated on the device and the pull is spread over the rings around the node
there too (fb_fem_add_haptic_forces -- what Deformable.timestep does under a probe).  After every step the volume (fb_fem_volume) and
where the pulled node has got to are printed; at the end the volume drift against the rest volume."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd.fem import Deformable  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, truth_cube  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 12
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
v, t = truth_cube(n, n, n, 0.1)
body = Deformable(v, t, fixed_vertices=cube_fixed_plane_i0(n, n))
rest_volume = body.compute_volume()
touch = (10.0, 0.1 * (n // 2), 0.0)                      # far beyond the free end, at mid height
node, where = body.pick_vertex(touch)
around, ids = body.pick_vertices(where - 0.11, where + 0.11)
print("picked node %d at %s; %d nodes within a cell of it: %s" % (node, np.round(where, 4), len(ids), list(ids)))
assert body.haptic_start_at(touch)                       # (a clamped node would be refused)
body.set_haptic_force_radius(4)
body.haptic_set_current_forces([node], [(1500.0, 4000.0, 0.0)])
for step in range(steps):
    iters = body.timestep()
    _, xyz, _ = body.integrator.pick_vertex(where)       # the node closest to where the picked one was
    print("step %d: %d PCG iterations, volume %.9f, node nearest the touch point now at %s" % (step, iters, body.compute_volume(), np.round(xyz, 4)))
body.haptic_end()
volume = body.compute_volume()
print("volume drift: %.3e of %.6f (%.4f %%)" % (volume - rest_volume, rest_volume, 100.0 * (volume - rest_volume) / rest_volume))
body.integrator.close()
