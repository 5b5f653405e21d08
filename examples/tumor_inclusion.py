"""A stiff inclusion in soft tissue: per-element materials through a step, a cut and a read-back.

    python examples/tumor_inclusion.py [--n 16]

An n^3 cube of soft tissue clamped at one face, a ball of tumour tissue (fifty times stiffer, a little denser) in its middle.  The body
sags under gravity for a few steps -- the inclusion barely deforms -- then a blade cuts through the inclusion (fb_fem_cut: on the
device, every piece inherits the material of the element it was cut from), the body is stepped again, and the materials are read back."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fembrain_amd import lib as fl  # noqa: E402
from fembrain_amd.fem import FemIntegrator  # noqa: E402
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube  # noqa: E402


def strains(x, t, q):
    """largest edge stretch of every element: |deformed edge| / |rest edge| - 1"""
    p, r = (x + q)[t], x[t]
    pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
    s = [np.linalg.norm(p[:, a] - p[:, b], axis=1) / np.linalg.norm(r[:, a] - r[:, b], axis=1) - 1.0 for a, b in pairs]
    return np.abs(np.array(s)).max(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
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
    print("%d elements, %d of them tumour; table %s" % (len(t), int(ids.sum()), [tuple(m) for m in zip(*g.materials())]))
    for _ in range(5):
        g.set_uniform_force(1, -5.0)
        g.do_timestep()
    q = g.get_q_state()[0].reshape(-1, 3)
    s = strains(v, t, q)
    print("after 5 steps: largest edge stretch %.3f in the tissue, %.4f in the tumour" % (s[ids == 0].max(), s[ids == 1].max()))
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
    info, delta = g.cut(strip, mode="carry")
    assert info["status"] == fl.FB_CUT_DONE, info
    x, tt = g.read_mesh()
    now = g.element_materials()
    inside = np.linalg.norm(x[tt].mean(axis=1) - centre, axis=1) < radius
    print("cut: %d elements removed, %d pieces added; %d of %d elements are tumour now" % (info["n_removed"], info["n_added"], int(now.sum()), len(tt)))
    # a piece lies inside its parent, and the ball was marked by element centroids: pieces of tumour elements are tumour
    parents_kept = np.ones(len(t), bool)
    parents_kept[delta["removed"]] = False
    assert np.array_equal(now[:parents_kept.sum()], ids[parents_kept])
    print("pieces whose centroid lies in the ball: %d, tumour pieces: %d" % (int(inside[parents_kept.sum():].sum()), int(now[parents_kept.sum():].sum())))
    for _ in range(3):
        g.set_uniform_force(1, -5.0)
        g.do_timestep()
    print("3 steps after the cut: %d PCG iterations in the last, max |q| %.4f" % (g.last.cg_iterations, np.abs(g.get_q_state()[0]).max()))
    g.close()


if __name__ == "__main__":
    main()
