"""Where a stiff inclusion carries the load: element stress on the device, drawn on the surface.

    python examples/stress_map.py [--n 16] [--out DIR]

The body of examples/tumor_inclusion.py -- an n^3 cube of soft tissue clamped at one face, a ball of tumour tissue fifty times stiffer in
its middle -- sags under gravity, is cut through the inclusion, and sags again.  Before and after the cut the stress of every element
is computed on the device (fb_fem_stress: the bracket of the corotational element force, with each element's own material); what comes
back is the summary and, for the drawing, one float per surface vertex (fb_fem_surface_stress) next to the positions of
fb_fem_surface_update.  The surface is written as stress_before.obj / stress_after.obj with the scalar of vertex k in the k-th
"# vm" line."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402


def write_obj(path, xyz, faces, vertex_ids, vm):
    compact = {int(c): k + 1 for k, c in enumerate(vertex_ids)}   # caller id -> 1-based index of the .obj
    with open(path, "w") as f:
        f.write("# surface of the simulated mesh; '# vm' lines: mean von Mises stress behind the vertex, in vertex order\n")
        for p in xyz:
            f.write("v %.7g %.7g %.7g\n" % tuple(p))
        for s in vm:
            f.write("# vm %.7g\n" % s)
        for a, b, c in faces:
            f.write("f %d %d %d\n" % (compact[int(a)], compact[int(b)], compact[int(c)]))


def report(g, when, out):
    info = g.stress()
    vm = g.element_stress()["von_mises"]              # (for the split by material only: the drawing needs none of it)
    ids = g.element_materials()
    print("largest von Mises stress %s: %.4g in the tissue, %.4g in the tumour (element %d of %d; %d inverted, min J %.3f, energy %.4g)"
          % (when, vm[ids == 0].max(), vm[ids == 1].max(), info["max_element"], info["n_elements"], info["n_inverted"], info["min_J"], info["energy"]))
    assert info["max_von_mises"] == vm.max()
    surf = g.surface()
    xyz, _, _ = g.surface_update()
    colour = g.surface_stress()
    if out:
        name = os.path.join(out, "stress_%s.obj" % when.split()[0])
        write_obj(name, xyz, surf["faces"], surf["vertex_ids"], colour)
        print("  %s: %d vertices, %d triangles, scalar %.4g .. %.4g" % (name, len(xyz), len(surf["faces"]), colour.min(), colour.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--out", default=None, help="directory for stress_before.obj / stress_after.obj")
    a = ap.parse_args()
    n = a.n
    v, t = truth_cube(n, n, n, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    centre = 0.5 * (v.min(0) + v.max(0))
    radius = 0.25 * (v.max(0) - v.min(0)).min()
    ids = (np.linalg.norm(v[t].mean(axis=1) - centre, axis=1) < radius).astype(np.uint8)   # 1: tumour
    tissue, tumour = (2e5, 0.45, 1000.0), (1e7, 0.40, 1100.0)
    g = FemIntegrator(v, t, fixed, E=tissue[0], nu=tissue[1], rho=tissue[2], expect_cuts=True)
    g.set_materials(*zip(tissue, tumour), element_ids=ids)
    print("%d elements, %d of them tumour" % (len(t), int(ids.sum())))
    for _ in range(5):
        g.set_uniform_force(1, -5.0)
        g.do_timestep()
    report(g, "before the cut", a.out)
    # a blade through the middle of a cell across the inclusion
    xs = np.unique(v[:, 0])
    k = len(xs) // 2
    point = np.array([0.5 * (xs[k - 1] + xs[k]), centre[1], centre[2]])
    nrm = np.array([1.0, 0.013, 0.007])
    nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    half = 4.0 * (v.max(0) - v.min(0)).max()
    strip = np.array([point - half * e1 - half * e2, point - half * e1 + half * e2, point + half * e1 - half * e2, point + half * e1 + half * e2])
    info, _ = g.cut(strip, mode="carry")
    assert info["status"] == fl.FB_CUT_DONE, info
    try:
        g.surface_stress()
        raise AssertionError("the stress of the uncut mesh must not be served for the cut one")
    except fl.FbError:
        pass
    for _ in range(3):
        g.set_uniform_force(1, -5.0)
        g.do_timestep()
    report(g, "after the cut", a.out)
    g.close()


if __name__ == "__main__":
    main()
