"""fembrain_amd/erosion.py (the erosion rule in numpy) against an independent scalar loop over the elements, and the counts of
the 16 x 5 x 5-node beam pinned.  No GPU."""
import numpy as np
import pytest

from fembrain_amd import erosion as er
from fembrain_amd.meshgen import truth_cube

CENTRE = (-0.1 + 0.013, 0.2 + 0.007, -0.05 - 0.004)
CAPSULE = ("capsule", (-0.47, 0.21, -0.07), (0.13, 0.26, -0.04), 0.13)
# radius, rule, selected, freed
SPHERES = [(0.05, "centroid", 1, 0), (0.05, "any_node", 24, 1), (0.12, "centroid", 44, 1), (0.12, "all_nodes", 2, 0), (0.12, "any_node", 118, 7),
           (0.2, "centroid", 213, 11), (0.2, "all_nodes", 54, 1), (0.2, "any_node", 340, 44), (0.3, "centroid", 484, 83)]


@pytest.fixture(scope="module")
def beam():
    v, t = truth_cube(16, 5, 5, 0.1)
    v, t = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(t, np.int32).reshape(-1, 4)
    assert len(v) == 400 and len(t) == 1440
    assert np.allclose(v.min(0), [-0.8, 0.0, -0.25]) and np.allclose(v.max(0), [0.7, 0.4, 0.15])
    q = np.random.default_rng(3).normal(size=3 * len(v)) * 0.01
    return v, t, q


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _inside_scalar(shape, p):
    kind, a = shape[0], [float(x) for x in shape[1]]
    u = [p[i] - a[i] for i in range(3)]
    if kind == "sphere":
        return _dot(u, u) <= float(shape[2]) * float(shape[2])
    if kind == "capsule":
        b, r = [float(x) for x in shape[2]], float(shape[3])
        d = [b[i] - a[i] for i in range(3)]
        dd = _dot(d, d)
        t = min(max(_dot(u, d) / dd, 0.0), 1.0) if dd > 0 else 0.0
        c = [a[i] + t * d[i] for i in range(3)]
        w = [p[i] - c[i] for i in range(3)]
        return _dot(w, w) <= r * r
    half = [float(x) for x in shape[2]]
    R = np.eye(3) if len(shape) < 4 or shape[3] is None else np.asarray(shape[3], np.float64).reshape(3, 3)
    return all(abs(_dot([float(x) for x in R[i]], u)) <= half[i] for i in range(3))


def _select_scalar(x0, tets, q, shapes, rule, frame):
    """element by element, python floats"""
    out = []
    for e, t in enumerate(tets):
        P = []
        for n in t:
            P.append([float(x0[n, d]) + float(q[3 * n + d]) if frame == "world" else float(x0[n, d]) for d in range(3)])
        if rule == "centroid":
            c = [((P[0][d] + P[1][d]) + (P[2][d] + P[3][d])) * 0.25 for d in range(3)]
            ok = any(_inside_scalar(s, c) for s in shapes)
        else:
            ins = [any(_inside_scalar(s, p) for s in shapes) for p in P]
            ok = all(ins) if rule == "all_nodes" else any(ins)
        if ok:
            out.append(e)
    return np.array(out, np.int32)


def _freed_scalar(tets, sel):
    sel = set(int(e) for e in sel)
    kept = set()
    for e, t in enumerate(tets):
        if e not in sel:
            kept.update(int(n) for n in t)
    return np.array(sorted(set(int(n) for e in sel for n in tets[e]) - kept), np.int32)


@pytest.mark.parametrize("radius,rule,n_sel,n_freed", SPHERES)
def test_sphere_counts(beam, radius, rule, n_sel, n_freed):
    v, t, _ = beam
    shapes = [("sphere", CENTRE, radius)]
    ids = er.select(v, t, None, shapes, rule=rule, frame="rest")
    assert np.array_equal(ids, _select_scalar(v, t, None, shapes, rule, "rest"))
    freed = er.freed_nodes(t, ids)
    assert np.array_equal(freed, _freed_scalar(t, ids))
    assert (len(ids), len(freed)) == (n_sel, n_freed)


def test_capsule_counts(beam):
    v, t, _ = beam
    ids = er.select(v, t, None, [CAPSULE], frame="rest")
    assert np.array_equal(ids, _select_scalar(v, t, None, [CAPSULE], "centroid", "rest"))
    assert (len(ids), len(er.freed_nodes(t, ids))) == (249, 5)


@pytest.mark.parametrize("rule", er.RULES)
def test_world_frame_and_mixed_shapes_against_the_scalar_loop(beam, rule):
    v, t, q = beam
    c, s = np.cos(0.5), np.sin(0.5)
    shapes = [("sphere", CENTRE, 0.12), CAPSULE, ("box", (0.3, 0.35, -0.05), (0.12, 0.08, 0.3), [[c, s, 0], [-s, c, 0], [0, 0, 1]])]
    ids = er.select(v, t, q, shapes, rule=rule, frame="world")
    assert 0 < len(ids) < len(t)
    assert np.array_equal(ids, _select_scalar(v, t, q, shapes, rule, "world"))
    assert not np.array_equal(ids, er.select(v, t, q, shapes, rule=rule, frame="rest"))
    assert np.array_equal(er.freed_nodes(t, ids), _freed_scalar(t, ids))


@pytest.mark.parametrize("rule", er.RULES)
def test_a_capsule_of_no_length_is_the_sphere(beam, rule):
    v, t, q = beam
    for r in (0.05, 0.12, 0.2):
        assert np.array_equal(er.select(v, t, q, [("capsule", CENTRE, CENTRE, r)], rule=rule), er.select(v, t, q, [("sphere", CENTRE, r)], rule=rule))


def test_an_aligned_box_is_an_interval_test(beam):
    v, t, q = beam
    c, half = np.array([0.05, 0.3, -0.05]), np.array([0.21, 0.11, 0.08])
    X = v + q.reshape(-1, 3)
    cen = ((X[t[:, 0]] + X[t[:, 1]]) + (X[t[:, 2]] + X[t[:, 3]])) * 0.25
    want = np.nonzero((np.abs(cen - c) <= half).all(1))[0]
    assert len(want) > 0
    assert np.array_equal(er.select(v, t, q, [("box", c, half, None)]), want)
    assert np.array_equal(er.select(v, t, q, [("box", c, half, np.eye(3))]), want)


def test_overlapping_shapes_select_an_element_once(beam):
    v, t, q = beam
    a, b = ("sphere", CENTRE, 0.2), ("sphere", (CENTRE[0] + 0.1, CENTRE[1], CENTRE[2]), 0.2)
    ia, ib, both = er.select(v, t, q, [a]), er.select(v, t, q, [b]), er.select(v, t, q, [a, b, a])
    assert len(np.intersect1d(ia, ib)) > 0
    assert np.array_equal(both, np.union1d(ia, ib)) and len(np.unique(both)) == len(both)


def test_filters_and_sums(beam):
    v, t, q = beam
    mats = np.arange(len(t)) % 2
    assert np.array_equal(er.select(v, t, q, [], material_ids=mats, material=1), np.arange(1, len(t), 2))
    assert len(er.select(v, t, q, [], material=1)) == 0 and len(er.select(v, t, q, [], material=0)) == len(t)
    vm = np.random.default_rng(1).random(len(t))
    vm[7] = np.nan
    got = er.select(v, t, q, [("sphere", CENTRE, 0.3)], von_mises=vm, min_von_mises=0.5)
    assert np.array_equal(got, np.intersect1d(er.select(v, t, q, [("sphere", CENTRE, 0.3)]), np.nonzero(vm >= 0.5)[0])) and 7 not in got
    with pytest.raises(ValueError):
        er.select(v, t, q, [])
    V = er.rest_volumes(v, t)
    assert abs(V.sum() - 1.5 * 0.4 * 0.4) <= 1e-12
    vol, mass = er.volume_and_mass(v, t, np.arange(10), rho=[1000.0, 1200.0], material_ids=mats)
    assert abs(vol - V[:10].sum()) <= 1e-15 and abs(mass - (V[:10:2].sum() * 1000.0 + V[1:10:2].sum() * 1200.0)) <= 1e-12


def test_bad_arguments_are_refused_before_the_handle_is_touched():
    nan, inf = float("nan"), float("inf")
    ok = ("sphere", CENTRE, 0.2)
    bad_shapes = [("ball", CENTRE, 0.2), ("sphere", CENTRE, -0.1), ("sphere", CENTRE, nan), ("sphere", CENTRE, inf), ("sphere", (nan, 0, 0), 0.1),
                  ("capsule", CENTRE, (0, inf, 0), 0.1), ("capsule", CENTRE, CENTRE, -1.0), ("box", CENTRE, (0.1, -0.1, 0.1), None),
                  ("box", CENTRE, (0.1, nan, 0.1), None), ("box", CENTRE, (0.1, 0.1, 0.1), np.full((3, 3), nan)), ("box", (0, 0, inf), (0.1, 0.1, 0.1), None)]
    for s in bad_shapes:
        with pytest.raises(ValueError):
            er.erode_host(None, [ok, s])          # (None: a handle would have been read)
    for kw in (dict(rule="nodes"), dict(frame="body"), dict(material=-1), dict(material=256), dict(min_von_mises=-1.0), dict(min_von_mises=nan),
               dict(min_von_mises=inf), dict(max_elements=-1)):
        with pytest.raises(ValueError):
            er.erode_host(None, [ok], **kw)
    with pytest.raises(ValueError):
        er.erode_host(None, [])
    er.check_shapes([ok, CAPSULE, ("box", CENTRE, (0.1, 0.0, 0.1), np.eye(3))])
