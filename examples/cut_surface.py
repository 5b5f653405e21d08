"""What a host draws, before and after a scalpel pass, without an element ever returning to the host.

    python examples/cut_surface.py OUTDIR [n]

A cantilever of n^3 nodes (default 16) sags under a load for a few steps, a blade passes through mid-span, the two halves sag on.  The
render surface -- the boundary triangles of the tet mesh, the positions and the normals of their vertices -- is built and kept current on
the device (fb_fem_surface / fb_fem_surface_update); the host receives 24 bytes per surface vertex after a step and the face list once
per cut.  The cut runs with track=False: the element list is never read back.  Writes OUTDIR/before.obj and after.obj (positions,
normals, faces) and the same arrays as before.npz / after.npz."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402


def write_obj(path, xyz, normals, faces, vertex_ids):
    compact = np.searchsorted(vertex_ids, faces) + 1      # faces index node ids; the file indexes the compact vertex list
    with open(path, "w") as fh:
        for p in xyz:
            fh.write("v %.9g %.9g %.9g\n" % tuple(p))
        for n in normals:
            fh.write("vn %.9g %.9g %.9g\n" % tuple(n))
        for a, b, c in compact:
            fh.write("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c))


def dump(fem, outdir, stem):
    s = fem.surface()                       # topology: rebuilt on the device only if the mesh changed
    xyz, normals, box = fem.surface_update()
    write_obj(os.path.join(outdir, stem + ".obj"), xyz, normals, s["faces"], s["vertex_ids"])
    np.savez(os.path.join(outdir, stem + ".npz"), xyz=xyz, normals=normals, faces=s["faces"], vertex_ids=s["vertex_ids"], face_tets=s["face_tets"])
    print("%s: %d faces on %d vertices (build %d), box %s .. %s" % (stem, len(s["faces"]), len(s["vertex_ids"]), s["n_builds"], box[0], box[1]))
    return s


outdir = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 16
os.makedirs(outdir, exist_ok=True)
v, t = truth_cube(n, n, n, 0.1)
v = np.asarray(v, np.float64).reshape(-1, 3)
fem = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n)), expect_cuts=True)
for _ in range(3):
    fem.set_uniform_force(1, -300.0)
    fem.do_timestep()
before = dump(fem, outdir, "before")
# the blade: a plane across mid-span, tilted a little so that it passes through no node
lo, hi = v.min(0), v.max(0)
span = float((hi - lo).max())
nrm = np.array([1.0, 0.031, 0.017])
nrm /= np.linalg.norm(nrm)
a = np.cross(nrm, [0.0, 1.0, 0.0])
a /= np.linalg.norm(a)
b = np.cross(nrm, a)
info = None
for shift in (0.0, 0.013, 0.029, 0.057, 0.11):  # a blade that meets a node or an edge's end is refused (or leaves an unhandled cell): moved a little, swept again
    p = lo + 0.5 * (hi - lo) + shift * span / (n - 1) * nrm
    try:
        info, _ = fem.cut(np.array([p - span * a - span * b, p - span * a + span * b, p + span * a - span * b, p + span * a + span * b]), mode="carry", track=False)
    except fl.FbError as e:
        print("blade moved on:", e)
        continue
    if info["status"] == fl.FB_CUT_DONE:
        break
assert info is not None and info["status"] == fl.FB_CUT_DONE, info
for _ in range(3):
    fem.set_uniform_force(1, -300.0)
    fem.do_timestep()
after = dump(fem, outdir, "after")
assert after["n_builds"] == before["n_builds"] + 1 and len(after["faces"]) > len(before["faces"])
print("cut surface ok")
