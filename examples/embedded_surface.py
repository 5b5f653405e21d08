"""The surface a host draws, finer than the tets, bound to them and moved on the device -- through a step, a cut and a split.

    python examples/embedded_surface.py OUTDIR [model.blob] [cellsize]

Polygonizes the model (default: the ventricle fixture) twice: coarsely into the tet mesh the FEM handle simulates, and at half the cell
size into the marching-cubes surface that is drawn.  The surface goes to the handle on the device (fb_fem_embed_from_poly): every vertex
is bound to the element that contains it through a uniform grid.  The body sags for a few steps, a blade passes through it, the parts are
pushed apart; the binding follows each change inside the call that makes it, and what reaches the host per frame is 24 bytes per drawn
vertex (fb_fem_embed_update) -- no displacement vector, no deformation callback.  Before the cut the drawn surface is clicked: a ray
finds the triangle under it on the device (fb_fem_embed_pick_ray), a pull on that triangle's three vertices goes to the nodes through the
binding (fb_fem_embed_add_forces), the body steps, and the surface is written coloured by the von Mises stress of the element behind every
vertex (fb_fem_embed_stress).  Writes OUTDIR/before.obj, touched.obj (vertex colours) and after.obj."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.blobtree import read_blob  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import fixed_vertices_to_dofs  # noqa: E402
from fembrain_amd.poly import GpuPoly  # noqa: E402


def write_obj(path, xyz, normals, triangles, scalar=None):
    """scalar: one value per vertex, written as a blue-to-red vertex colour behind the position"""
    with open(path, "w") as fh:
        if scalar is None:
            for p in xyz:
                fh.write("v %.9g %.9g %.9g\n" % tuple(p))
        else:
            c = np.clip(np.asarray(scalar, np.float64) / max(float(np.max(scalar)), 1e-30), 0.0, 1.0)
            for p, x in zip(xyz, c):
                fh.write("v %.9g %.9g %.9g %.4f %.4f %.4f\n" % (p[0], p[1], p[2], x, 0.2, 1.0 - x))
        for n in normals:
            fh.write("vn %.9g %.9g %.9g\n" % tuple(n))
        for a, b, c in np.asarray(triangles, np.int64) + 1:
            fh.write("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c))


here = os.path.dirname(os.path.abspath(__file__))
outdir = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "..", "tests", "golden", "blob", "ventricle.blob")
cell = float(sys.argv[3]) if len(sys.argv) > 3 else 0.3
os.makedirs(outdir, exist_ok=True)
blob = read_blob(path)
coarse, fine = GpuPoly(blob), GpuPoly(blob)
xyz, tets = coarse.run_tetrahedralizer(cell)
fine.sweep(0.5 * cell)
fine.classify()
counts = fine.surface()
triangles = fine.read_surface()[2]          # the index buffer, once: it never changes
lo, hi = xyz.min(0), xyz.max(0)
fixed = fixed_vertices_to_dofs(np.nonzero(xyz[:, 1] < lo[1] + 0.05 * (hi[1] - lo[1]))[0].astype(np.int32))
fem = FemIntegrator.from_poly(coarse, fixed)
eid, info = fem.embed_from_poly(fine, info=True)
print("%d tets; %d drawn vertices, %d triangles bound through a %d x %d x %d grid (%d wide elements), %d outside the tets"
      % (len(tets), info["n_points"], info["n_triangles"], *info["grid"], info["n_wide"], info["n_external"]))
for _ in range(3):
    fem.set_uniform_force(1, -30.0)
    fem.do_timestep()
pos, nrm, state = fem.embed_update(eid)
write_obj(os.path.join(outdir, "before.obj"), pos, nrm, triangles)
# a click on what is drawn: a ray from above the body, straight down but for a tilt that keeps it off the vertices
top = pos[np.argmax(pos[:, 1])].astype(np.float64)
origin, direction = top + [0.11 * cell, 2.0 * float((hi - lo).max()), 0.07 * cell], np.array([0.013, -1.0, 0.021])
hit = fem.embed_pick_ray(eid, origin, direction)
assert hit["triangle"] >= 0, hit
u, v = hit["bary"]
ids = np.asarray(triangles[hit["triangle"]], np.int32)
order = np.argsort(ids)
pull = np.array([0.0, 4000.0, 0.0])
for _ in range(2):
    fem.set_uniform_force(1, -30.0)
    fem.embed_add_forces(eid, (np.array([1.0 - u - v, u, v])[:, None] * pull)[order], ids[order])
    fem.do_timestep()
fem.stress()
vm = fem.embed_stress(eid)
pos_t, nrm_t, _ = fem.embed_update(eid)
write_obj(os.path.join(outdir, "touched.obj"), pos_t, nrm_t, triangles, scalar=vm)
nearest, _, _ = fem.embed_pick_point(eid, hit["xyz"])
print("clicked triangle %d at t = %.4f (nearest drawn vertex %d); pulled, the surface rose by %.3g there; von Mises up to %.3g, %.3g at the click"
      % (hit["triangle"], hit["t"], nearest, pos_t[nearest, 1] - pos[nearest, 1], vm.max(), vm[nearest]))
assert nearest in ids and pos_t[nearest, 1] > pos[nearest, 1] and vm.max() > 0 and fem.embed_forces_info(eid)["n_table_builds"] == 1
# the blade: a plane through the middle of the body, tilted a little so that it passes through no node
span = float((hi - lo).max())
n = np.array([1.0, 0.031, 0.017])
n /= np.linalg.norm(n)
a = np.cross(n, [0.0, 1.0, 0.0])
a /= np.linalg.norm(a)
b = np.cross(n, a)
status, strip = None, None
for shift in (0.0, 0.013, 0.029, 0.057, 0.11):  # a blade that meets a node or leaves an unhandled cell is moved a little and swept again
    p = 0.5 * (lo + hi) + shift * cell * n
    strip = np.array([p - span * a - span * b, p - span * a + span * b, p + span * a - span * b, p + span * a + span * b])
    try:
        status = fem.cut(strip, mode="bake", track=False)[0]["status"]
    except fl.FbError as e:
        print("blade moved on:", e)
        continue
    if status == fl.FB_CUT_DONE:
        break
assert status == fl.FB_CUT_DONE, status
split = fem.split_parts(strip, 0.5 * cell, track=False)
for _ in range(2):
    fem.set_uniform_force(1, -30.0)
    fem.do_timestep()
pos2, nrm2, state2 = fem.embed_update(eid)
write_obj(os.path.join(outdir, "after.obj"), pos2, nrm2, triangles)
print("after the cut: %d parts, %d drawn vertices re-bound among the pieces of their elements, %d searches in all"
      % (fem.parts()["n_parts"], state2["n_rebound"], state2["n_locates"]))
assert len(pos2) == len(pos) == counts.n_surface_vertices and state2["n_rebound"] > 0
assert np.abs(pos2 - pos).max() > 0.25 * cell, "the parts went apart, and the drawn surface with them"
print("embedded surface ok")
