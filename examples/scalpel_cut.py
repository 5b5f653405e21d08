"""A scalpel pass through a polygonized BlobTree model, on the device end to end (CuttableMesh::cut + cutCompleted in one call).

    python examples/scalpel_cut.py [model.blob] [cellsize] [mode]

Polygonizes the model (default: the ventricle fixture) into the FEM handle without a host copy, lets it sag under gravity for two
steps, sweeps a blade through the whole body (one quad of the swept strip, slightly tilted so that it passes no node) and cuts it with
fb_fem_cut -- every crossed edge split in two nodes, every crossed element subdivided, the handle re-synced -- then steps again.
mode: bake (FemBrain: the deformed shape becomes the rest shape) or carry (the rest shape and the state are kept)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.blobtree import read_blob  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import fixed_vertices_to_dofs  # noqa: E402
from fembrain_amd.poly import GpuPoly  # noqa: E402

here = os.path.dirname(os.path.abspath(__file__))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "tests", "golden", "blob", "ventricle.blob")
cell = float(sys.argv[2]) if len(sys.argv) > 2 else 0.05
mode = sys.argv[3] if len(sys.argv) > 3 else "bake"
poly = GpuPoly(read_blob(path))
xyz, tets = poly.run_tetrahedralizer(cell)
low = np.nonzero(xyz[:, 1] <= np.percentile(xyz[:, 1], 10))[0]
fem = FemIntegrator.from_poly(poly, fixed_vertices_to_dofs(low))
print("%s at cell %.3f: %d vertices, %d tets" % (os.path.basename(path), cell, len(xyz), len(tets)))
for step in range(2):
    fem.set_uniform_force(1, -200.0)
    fem.do_timestep()
# the blade: a vertical plane across the body at 40 % of its x extent, tilted a little about y and z
lo, hi = xyz.min(0), xyz.max(0)
span = float((hi - lo).max())
c = lo + (hi - lo) * np.array([0.4, 0.5, 0.5])
n = np.array([1.0, 0.031, 0.017])
n /= np.linalg.norm(n)
a = np.cross(n, [0.0, 1.0, 0.0])
a /= np.linalg.norm(a)
b = np.cross(n, a)
for shift in (0.0, 0.013, 0.029):  # a blade that would leave a cell in a pattern the subdivision refuses is moved a little and swept again
    p = c + shift * cell * n
    strip = np.array([p - span * a - span * b, p - span * a + span * b, p + span * a - span * b, p + span * a + span * b])
    info, delta = fem.cut(strip, mode=mode)
    print("cut (%s): status %d, %d cut edges, %d + %d cells of case A + B, %d unhandled, %d removed, %d added, %d new nodes, "
          "smallest piece %.2e of its parent" % (mode, info["status"], info["n_cut_edges"], info["n_case_a"], info["n_case_b"],
                                                info["n_unhandled"], info["n_removed"], info["n_added"], info["n_new_nodes"],
                                                info["min_volume_ratio"]))
    if info["status"] == fl.FB_CUT_DONE:
        break
assert info["status"] == fl.FB_CUT_DONE, info
print("after the cut: %d vertices, %d tets (re-sync path %d)" % (fl.lib().fb_fem_num_nodes(fem.h), fl.lib().fb_fem_num_tets(fem.h), fem.resync_path()))
for step in range(3):
    fem.set_uniform_force(1, -200.0)
    it = fem.do_timestep()
    print("step %d after the cut: %d PCG iterations, converged %d, max |q| %.4f" % (step, it, fem.last.converged, np.abs(fem.get_q_state()[0]).max()))
    assert fem.last.converged == 1
print("scalpel cut ok")
