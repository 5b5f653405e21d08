"""tests/hapticref.py and fembrain_amd.fem.spread_haptic_forces pinned without a GPU: what tests/test_haptic_gpu.py compares the device against."""
import math
import os

import numpy as np

import hapticref as hr
from fembrain_amd.fem import spread_haptic_forces
from fembrain_amd.meshgen import truth_cube

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_volume_of_a_truth_cube_is_its_box():
    v, t = truth_cube(5, 4, 3, 0.1)
    vol = hr.element_volumes(v, t)
    assert len(vol) == len(t) and (vol > 0).all()
    # six tets of equal volume per cell: h^3 / 6 each
    assert np.abs(vol - 0.1 ** 3 / 6).max() < 1e-15
    assert abs(math.fsum(vol) - 0.4 * 0.3 * 0.2) < 1e-14


def test_volume_against_the_determinant_formula_on_beam3():
    d = np.load(os.path.join(GOLDEN, "fem_beam3.npz"))
    v, t = d["verts"].astype(np.float64), d["tets"].astype(np.int64)
    q = 0.01 * np.sin(3.0 * v + 0.2)
    p = hr.positions(v, q)
    assert np.array_equal(p, v + q)
    vol = hr.element_volumes(p, t)
    m = np.stack([p[t[:, 0]] - p[t[:, 3]], p[t[:, 1]] - p[t[:, 3]], p[t[:, 2]] - p[t[:, 3]]], axis=1)
    want = np.abs(np.linalg.det(m)) / 6.0
    assert len(vol) == len(t) and np.abs(vol - want).max() <= 1e-12 * want.max()


def test_pick_takes_the_lowest_index_of_equal_distances():
    p = np.array([[1.0, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, -0.5, 0.0], [0.0, 0.5, 0.0], [3.0, 0.0, 0.0]])
    i, xyz, d = hr.pick_vertex(p, (0.0, 0.0, 0.0))
    assert i == 1 and d == 0.25 and np.array_equal(xyz, p[1])       # 1, 2 and 3 tie
    i, _, d = hr.pick_vertex(p[::-1], (0.0, 0.0, 0.0))
    assert i == 1 and d == 0.25
    i, _, d = hr.pick_vertex(p, (10.0, 0.0, 0.0))
    assert i == 4 and d == 49.0


def test_box_bounds_are_inclusive_and_ids_ascend():
    v, _ = truth_cube(3, 3, 3, 0.5)
    ids, xyz = hr.pick_box(v, v[13], v[26])                          # from the middle node to the last corner, bounds on the lattice
    assert list(ids) == [13, 14, 16, 17, 22, 23, 25, 26] and np.array_equal(xyz, v[ids])
    assert len(hr.pick_box(v, (5.0, 5.0, 5.0), (6.0, 6.0, 6.0))[0]) == 0
    assert len(hr.pick_box(v, v.min(0), v.max(0))[0]) == 27


def test_spread_on_a_path_of_tets():
    """elements (k, k+1, k+2, k+3): node i neighbours i-3 .. i+3, so ring j of a source s is the nodes at 3j-2 .. 3j from it"""
    n = 14
    tets = np.array([[k, k + 1, k + 2, k + 3] for k in range(n - 3)], np.int32)
    bptr, bcol = hr.node_pattern(n, tets)
    assert list(bcol[bptr[5]:bptr[6]]) == [2, 3, 4, 5, 6, 7, 8]
    f = np.zeros(3 * n)
    spread_haptic_forces(bptr, bcol, [0], [(0.0, 4.0, 1.0)], 4, f)
    want = np.zeros((n, 3))
    for i in range(n):
        ring = (i + 2) // 3                                           # 0 | 1 1 1 | 2 2 2 | 3 3 3 | beyond
        if ring < 4:
            want[i] = np.array([0.0, 4.0, 1.0]) * (1.0 if ring == 0 else 1.0 * (4 - ring) / 4.0)
    assert np.array_equal(f.reshape(-1, 3), want)
    # size 1: the direct add only; a source in the middle reaches both ways; two sources add in order; a duplicate counts twice
    g = np.zeros(3 * n)
    spread_haptic_forces(bptr, bcol, [6], [(2.0, 0.0, 0.0)], 1, g)
    assert g[18] == 2.0 and np.count_nonzero(g) == 1
    g[:] = 0
    spread_haptic_forces(bptr, bcol, [6, 6], [(2.0, 0.0, 0.0), (0.0, 0.0, 8.0)], 2, g)
    want = np.zeros((n, 3))
    want[3:10] = (1.0, 0.0, 4.0)
    want[6] = (2.0, 0.0, 8.0)
    assert np.array_equal(g.reshape(-1, 3), want)
    # rings that run out of mesh add nothing further
    a = np.zeros(3 * n)
    spread_haptic_forces(bptr, bcol, [0], [(1.0, 0.0, 0.0)], 200, a)
    reached = a.reshape(-1, 3)[:, 0]
    assert all(reached[i] == (1.0 if i == 0 else 1.0 * (200 - (i + 2) // 3) / 200.0) for i in range(n))


def test_the_level_sweep_is_the_breadth_first_walk():
    """the formulation the device runs (hapticref.spread_by_levels) against the walk, bit for bit: overlapping balls, a duplicate, sources
    across a batch boundary, rings that run out of mesh"""
    v, t = truth_cube(5, 4, 4, 0.1)
    n = len(v)
    bptr, bcol = hr.node_pattern(n, t)
    rng = np.random.default_rng(5)
    for ids, size, batch in (([37], 5, 32), ([37, 38, 37, 0], 3, 32), ([int(i) for i in rng.permutation(n)[:7]] + [3, 3], 4, 4), ([11, 70], 12, 32), ([5], 1, 32)):
        frc = rng.uniform(-3000.0, 3000.0, size=(len(ids), 3))
        a = np.zeros(3 * n)
        a[1::3] = -10000.0
        b = a.copy()
        spread_haptic_forces(bptr, bcol, ids, [tuple(x) for x in frc], size, a)
        hr.spread_by_levels(n, t, ids, frc, size, b, batch=batch)
        assert np.array_equal(a, b), (ids, size)
