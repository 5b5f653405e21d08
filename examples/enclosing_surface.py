"""A closed surface drawn AROUND the body -- a skin over coarser tets -- bound to them and moved on the device.

    python examples/enclosing_surface.py [n] [cellsize]

The clamped beam (4 n x n x n nodes) and the marching-cubes surface of the sphere, stretched into an ellipsoid that encloses it: every
drawn vertex lies outside the tets and binds to the element with the closest centre (fb_fem_embed).  With this many outside points
(some 17,000 at the default cell size; the rule wants 8,192) the search does not scan the mesh for each of them: it builds a grid of the
element centres once and looks only at the cells that could hold a closer centre; a point that sees too many centres at about its closest
distance is left to the scan (fb_fem_embed_search_info_get says how many).  The beam sags for a few steps and the skin follows it
(fb_fem_embed_update)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.blobtree import sphere_blob  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import fixed_vertices_to_dofs, truth_cube  # noqa: E402
from fembrain_amd.poly import GpuPoly  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
cell = float(sys.argv[2]) if len(sys.argv) > 2 else 0.015
v, t = truth_cube(4 * n, n, n, 0.1)
v, t = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(t, np.int32).reshape(-1, 4)
lo, hi = v.min(0), v.max(0)
fixed = fixed_vertices_to_dofs(np.nonzero(v[:, 0] <= lo[0] + 1e-12)[0].astype(np.int32))
poly = GpuPoly(sphere_blob())
sx, _, triangles = poly.run(cell)
poly.close()
# the unit sphere's directions times the half-diagonal of the beam's box, axis by axis: an ellipsoid through the box's corners, then 5 % more
unit = sx.astype(np.float64) / np.linalg.norm(sx.astype(np.float64), axis=1)[:, None]
skin = 0.5 * (lo + hi) + unit * (1.05 * np.sqrt(3.0) * 0.5 * (hi - lo))
fem = FemIntegrator(v, t, fixed)
eid, info = fem.embed(skin, triangles.astype(np.int32), info=True)
search = fem.embed_search_info(eid)
names = {fl.FB_EMBED_CLOSEST_NONE: "none", fl.FB_EMBED_CLOSEST_SCAN: "scan", fl.FB_EMBED_CLOSEST_RING: "ring"}
print("%d tets; %d drawn vertices, %d outside the tets" % (len(t), info["n_points"], info["n_external"]))
print("closest centres by %s: %d centres tested, %.1f per point (a scan tests %d per point), %d points left to the scan, %d centre grid(s) built"
      % (names[search["path"]], search["centres_tested"], search["centres_tested"] / max(search["n_outside"], 1), len(t), search["n_far"], search["centre_grid_builds"]))
assert info["n_external"] == info["n_points"] == search["n_outside"]
rest = fem.embed_update(eid)[0]
for _ in range(2):
    fem.set_uniform_force(1, -30.0)
    fem.do_timestep()
pos, nrm, state = fem.embed_update(eid)
free, clamped = skin[:, 0] > hi[0], skin[:, 0] < lo[0]
sank = rest[:, 1].astype(np.float64) - pos[:, 1]
print("the skin beyond the free end sank by %.3g, the skin behind the clamped end by %.3g" % (sank[free].mean(), sank[clamped].mean()))
assert np.isfinite(pos).all() and free.any() and clamped.any() and sank[free].mean() > 0 and state["n_locates"] == 1
fem.close()
print("enclosing surface ok")
