"""A tool box is lowered onto the clamped beam: the probe's contact runs on the device, only a few numbers come back per frame.

    python examples/probe_contact.py [nx] [steps]

A beam of nx x 6 x 6 nodes (default nx = 16) hangs from its clamped face.  A box as wide as the beam's free half is lowered onto its top
over `steps` frames (default 6), a twentieth of a cell deeper each frame.  Every frame is what FemBrain's AvatarProbe::onTranslate and
Deformable::timestep do: the contact session on the device decides which nodes the box has touched (they keep their first-touch
positions), which of the box's faces presses, and the penalty forces (Deformable.probe_move -> fb_fem_contact_move); the step spreads
the list over the rings around every touched node, whatever their number (fb_fem_contact_apply).  Printed per frame: touched and new
nodes, the face, the contact distance, the pushing nodes; at the end the volume before and after."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import Deformable, ProbeContact  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, truth_cube  # noqa: E402

nx = int(sys.argv[1]) if len(sys.argv) > 1 else 16
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 6
v, t = truth_cube(nx, 6, 6, 0.1)
body = Deformable(v, t, fixed_vertices=cube_fixed_plane_i0(6, 6), gravity=False)
rest_volume = body.compute_volume()
top = v[:, 1].max()
lo, hi = np.array([-0.05, top, v[:, 2].min() - 0.5]), np.array([v[:, 0].max() + 0.5, top + 1.0, v[:, 2].max() + 0.5])
body.set_haptic_force_radius(3)
body.probe_start()
status = {fl.FB_CONTACT_MISS: "miss", fl.FB_CONTACT_EMPTY: "empty", fl.FB_CONTACT_SET: "set"}
touched = []
for frame in range(steps):
    lo[1] = top + 0.02 - 0.05 * frame                       # the first frame hovers above the beam: a miss
    info = body.probe_move(lo, hi, 1000.0)
    iters = body.timestep()
    face = ProbeContact.FACES[info["face"]] if info["face"] >= 0 else "none"
    print("frame %d: %s, %d touched (%d new), face %s, contact distance %.4f, %d pushing, %d PCG iterations"
          % (frame, status[info["status"]], info["n_touched"], info["n_new"], face, info["contact_dist"], info["n_pushing"], iters))
    touched.append(info["n_touched"])
volume = body.compute_volume()
body.probe_end()
after = body.integrator.contact_info()
print("touched counts: %s" % touched)
print("after the probe's mouse-up: %d touched, face kept %s" % (after["list_size"], ProbeContact.FACES[after["face"]] if after["face"] >= 0 else "none"))
print("volume before %.9f after %.9f (%.4f %%)" % (rest_volume, volume, 100.0 * (volume - rest_volume) / rest_volume))
assert touched[0] == 0 and touched[1] > 0 and touched == sorted(touched), touched   # (nodes never leave the set)
print("probe contact ok")
body.integrator.close()
