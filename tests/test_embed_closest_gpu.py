"""The closest centre for the points no element contains, through the grid of centres (csrc/embed_closest.hip; FEMBRAIN_EMBED_CLOSEST=ring)
against the full scan (=scan) and the numpy restatement (tests/embedref.py): the two passes must make the same binding bit for bit, on
points next to the body and many extents away, on exact ties, on grids one cell thick, around a cavity, under a small budget and across
mesh generations; and the ring must look at a small part of the mesh only, which is the point of it (fb_fem_embed_search_info_get)."""
import functools

import numpy as np
import pytest

import cutref as cr
import embedref as er
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import delaunay_jittered, truth_cube
from test_embed_gpu import _check_generic, _fixed_of, _shuffled

pytestmark = pytest.mark.gpu

OFF, ON = fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON
NONE, SCAN, RING = fl.FB_EMBED_CLOSEST_NONE, fl.FB_EMBED_CLOSEST_SCAN, fl.FB_EMBED_CLOSEST_RING
KEYS = ("elements", "vertices", "weights", "rest_xyz")


def _cube(nx, ny=None, nz=None):
    v, t = truth_cube(nx, ny or nx, nz or nx, 0.1)
    return np.array(v, np.float64).reshape(-1, 3), np.array(t, np.int32).reshape(-1, 4)


def outside_points(v, n, seed):
    """n seeded points outside the box of v: a point of the box pushed out along 1, 2 or 3 axes, on either side, by 1e-6, 0.02, 0.3, 3 or
    50 times the largest extent times a factor in [0.5, 1.5]; float32 values"""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    big = (hi - lo).max()
    p = lo + rng.random((n, 3)) * (hi - lo)
    for i in range(n):
        axes = rng.permutation(3)[:rng.integers(1, 4)]
        for k in axes:
            push = rng.choice([1e-6, 0.02, 0.3, 3.0, 50.0]) * big * rng.uniform(0.5, 1.5)
            p[i, k] = hi[k] + push if rng.random() < 0.5 else lo[k] - push
    p = np.float32(p).astype(np.float64)
    assert ((p < lo) | (p > hi)).any(axis=1).all()
    return p


def _both(monkeypatch, v, t, pts, renumber=OFF, fixed=None, budget=None):
    """pts bound twice on one handle, the external pass forced to the scan and to the ring: (scan, ring) as (binding, info, search info)"""
    g = FemIntegrator(v, t, _fixed_of(v) if fixed is None else fixed, renumber=renumber)
    if budget is None:
        monkeypatch.delenv("FEMBRAIN_EMBED_RING_BUDGET", raising=False)
    else:
        monkeypatch.setenv("FEMBRAIN_EMBED_RING_BUDGET", str(budget))
    out = []
    for path in ("scan", "ring"):
        monkeypatch.setenv("FEMBRAIN_EMBED_CLOSEST", path)  # (read at every search)
        eid, info = g.embed(pts, info=True)
        out.append((g.embedding(eid), info, g.embed_search_info(eid)))
    g.close()
    return out


def _same(a, b):
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return er.jittered_cube() if name == "cube" else delaunay_jittered(6)[:2]


# ---- 1. ring == scan == the restatement ----
@pytest.mark.parametrize("renumber", [OFF, ON])
@pytest.mark.parametrize("name,seed", [("cube", 42), ("delaunay", 42)])
def test_ring_equals_scan_equals_the_restatement(gpu, monkeypatch, name, seed, renumber):
    v, t = _mesh(name)
    pts = outside_points(v, 600, seed)
    if renumber == ON:
        v, t = _shuffled(v, t)
    (a, ia, sa), (b, ib, sb) = _both(monkeypatch, v, t, pts, renumber)
    _same(a, b)
    ref = _check_generic(v, t, pts, b, ib)  # (every point generic, by choice of seed: asserted in there)
    assert ref["n_external"] == 600 and ia["n_external"] == 600
    assert sa["path"] == SCAN and sa["n_outside"] == 600 and sa["centres_tested"] == 600 * len(t) and sa["centre_grid_builds"] == 0
    # At the default budget, max(64, n_tets / 32), some points are the scan's and some are not.  (Not the far ones as such: a point 50
    # extents out touches the mesh with a ball that is nearly a plane there and tests few centres.  The points that pass the budget are
    # those with many centres at about their closest distance -- on the CPU, 100 of these 600 on the cube and 437 on the Delaunay mesh.)
    assert sb["path"] == RING and sb["n_outside"] == 600 and 0 < sb["n_far"] < 600 and sb["centre_grid_builds"] == 1
    print("ring: %d far of 600, %d centres tested (scan %d), most of one point %d" % (sb["n_far"], sb["centres_tested"], sa["centres_tested"], sb["max_centres_one_point"]))


# ---- 2. ties ----
def test_an_exact_tie_goes_to_the_lower_id_through_the_ring(gpu, monkeypatch):
    # tests/test_embed_gpu.py's mirrored pair: the two tied centres lie in different cells, 300 elements and many cells apart in the second mesh
    a = np.array([[-1.0, 0, 0], [-0.5, 0, 0], [-0.75, 0.5, 0], [-0.75, 0, 0.5]])
    b = a[[1, 0, 2, 3]] * [-1.0, 1, 1]
    v = np.vstack([a, b])
    t = np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.int32)
    pts = np.array([[0.0, 4.0, 0.25], [0.0, -2.5, 1.0], [0.0, 0.125, 0.125]])
    k = np.arange(300)
    far = (a[None, :, :] + np.stack([np.zeros(300), 64.0 + k, np.zeros(300)], axis=1)[:, None, :]).reshape(-1, 3)
    v3 = np.vstack([a, far, b])
    t3 = np.vstack([t[:1], (4 + 4 * k)[:, None] + np.arange(4)[None, :], [[1204, 1205, 1206, 1207]]]).astype(np.int32)
    for verts, tets in ((v, t), (v, t[::-1].copy()), (v3, t3), (v3, t3[::-1].copy())):
        d = er.centre_distances(verts, tets, pts)
        assert np.array_equal(d[:, 0], d[:, -1])
        (sc, _, _), (rg, info, si) = _both(monkeypatch, verts, tets, pts, fixed=np.arange(3, dtype=np.int32))
        ref = er.bind(verts, tets, pts)
        assert si["path"] == RING and si["n_outside"] == 3 and info["n_external"] == 3
        assert np.array_equal(rg["elements"], [0, 0, 0]) and np.array_equal(ref["elements"], [0, 0, 0])
        assert np.array_equal(rg["weights"], ref["weights"])
        _same(sc, rg)


# ---- 3. grid shapes ----
def _around(v):
    """points on all 26 sides of the box of v, near and far, and points exactly on the faces of the grid's padded box"""
    lo, hi = v.min(0), v.max(0)
    c, half, big = 0.5 * (lo + hi), 0.5 * (hi - lo), (hi - lo).max()
    pts = []
    for d in np.ndindex(3, 3, 3):
        d = np.array(d) - 1.0
        if d.any():
            for push in (0.003, 0.07, 0.9):
                pts.append(c + d * (half + push * big) + (1 - np.abs(d)) * half * [0.31, -0.17, 0.23])
    pad = np.ldexp(big if big > 0 else 1.0, -30)  # (embed_grid_build's padding)
    for k in range(3):
        for face in (lo[k] - pad, hi[k] + pad):
            for s, u in ((0.13, 0.29), (0.5, 0.5), (0.87, 0.61), (0.0, 1.0)):
                p = lo + (hi - lo) * [s, u, 0.41]
                p[k] = face
                pts.append(p)
    return np.array(pts)


def _wide_mesh():
    cv, ct = er.jittered_cube()
    n0 = len(cv)
    far = cv.min(0) - 1.0 + np.vstack([np.zeros(3), 2.0 * np.eye(3)])
    return np.vstack([cv, far]), np.vstack([ct, np.array([[n0, n0 + 1, n0 + 2, n0 + 3]], np.int32)])


@pytest.mark.parametrize("shape", ["one_element", "slab", "wide", "delaunay"])
def test_grid_shapes(gpu, monkeypatch, shape):
    if shape == "one_element":
        v, t = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 1, 0], [0.0, 0, 1]]), np.array([[0, 1, 2, 3]], np.int32)
    elif shape == "slab":
        v, t = _cube(6, 6, 2)  # one layer of cells
    elif shape == "wide":
        v, t = _wide_mesh()    # the wide element has a centre like any other
    else:
        v, t = _mesh("delaunay")
    pts = _around(v)
    (a, ia, sa), (b, ib, sb) = _both(monkeypatch, v, t, pts, fixed=np.arange(3, dtype=np.int32))
    _same(a, b)
    assert sb["path"] == RING and sb["n_outside"] == ia["n_external"] == ib["n_external"] >= 3 * 26
    ref = er.bind(v, t, pts)
    d = er.centre_distances(v, t, pts)
    ext = np.nonzero(ref["external"])[0]
    # whatever rounding decides about containment on the device, an external point's element is a closest one, the lowest of them
    got = b["elements"][ext]
    assert np.array_equal(got, d[ext].argmin(axis=1))


# ---- 4. a cavity ----
def test_points_in_a_cavity(gpu, monkeypatch):
    v, t = _cube(8)
    mid = 0.5 * (v.min(0) + v.max(0))
    keep = ~(np.abs(er.centres(v, t) - mid) <= 0.1).all(axis=1)
    assert len(t) == 2058 and keep.sum() == 1994
    t = np.ascontiguousarray(t[keep])
    pts = np.float32(mid + (np.random.default_rng(5).random((300, 3)) - 0.5) * 0.19).astype(np.float64)
    (a, ia, sa), (b, ib, sb) = _both(monkeypatch, v, t, pts)
    _same(a, b)
    ref = _check_generic(v, t, pts, b, ib)
    assert ref["n_external"] > 150 and sb["path"] == RING and sb["n_outside"] == ref["n_external"]
    assert not (v.min(0) > pts).any() and not (v.max(0) < pts).any()  # inside the box, outside the tets


# ---- 5. the budget ----
def test_a_small_budget_sends_points_to_the_scan(gpu, monkeypatch):
    v, t = _mesh("cube")
    pts = outside_points(v, 600, 42)
    (a, ia, sa), (b, ib, sb) = _both(monkeypatch, v, t, pts, budget=8)
    _same(a, b)
    _check_generic(v, t, pts, b, ib)
    assert sb["path"] == RING and sb["n_far"] > 0
    print("budget 8: %d far of 600" % sb["n_far"])


# ---- 6. the work is local ----
def test_the_ring_looks_at_a_small_part_of_the_mesh(gpu, monkeypatch):
    """The cap: the grid has about one cell per element (cell edge 0.055) and the closest centre is at most 1.4 mesh cells away; a search
    that visited the whole box p +- (2 d + 2 cells), far more than the second phase needs, would test 327 centres per point on average
    and 966 at most on this input (computed on the CPU), against n_tets / 8 = 998.  A "ring" that quietly scanned would test 7,986."""
    v, t = _cube(12)
    assert len(t) == 7986
    rng = np.random.default_rng(6)
    lo, hi = v.min(0), v.max(0)
    pts = lo + rng.random((2000, 3)) * (hi - lo)
    pts[:, 0] = hi[0] + (1.0 - rng.random(2000)) * 0.1  # out of one face by up to one cell
    pts = np.float32(pts).astype(np.float64)
    assert (pts[:, 0] > hi[0]).all()
    (a, ia, sa), (b, ib, sb) = _both(monkeypatch, v, t, pts)
    _same(a, b)
    assert sa["path"] == SCAN and sa["n_outside"] == 2000 and sa["centres_tested"] == 2000 * len(t) and sa["max_centres_one_point"] == len(t)
    print("ring: %.1f centres per point, most %d; n_tets / 8 = %d" % (sb["centres_tested"] / sb["n_outside"], sb["max_centres_one_point"], len(t) // 8))
    assert sb["path"] == RING and sb["n_outside"] == 2000 and sb["n_far"] == 0
    assert sb["centres_tested"] / sb["n_outside"] <= len(t) / 8
    d = er.centre_distances(v, t, pts[:200])
    assert np.array_equal(b["elements"][:200], d.argmin(axis=1))


# ---- 7. mesh generations ----
def test_the_centre_grid_follows_the_mesh_generations(gpu, monkeypatch):
    """One centre grid per mesh generation that searches through it, none for a second embedding on the same generation; after a cut and
    after a re-sync to another mesh a search through the ring gives what a fresh handle on that mesh gives, bit for bit.  (The embedding
    that was live during the cut is not compared after it: a point outside the body keeps the element it has across a change in place,
    by the header's rule, where a new search may prefer the centre of a piece.  The search on the cut mesh is a new embedding's.)"""
    monkeypatch.setenv("FEMBRAIN_EMBED_CLOSEST", "ring")
    monkeypatch.delenv("FEMBRAIN_EMBED_RING_BUDGET", raising=False)
    v, t = _cube(6)
    fixed = _fixed_of(v)
    lo, ext = v.min(0), v.max(0) - v.min(0)
    rng = np.random.default_rng(8)
    u = rng.normal(size=(400, 3))
    pts = np.float32(lo + 0.5 * ext + u / np.linalg.norm(u, axis=1)[:, None] * 0.9 * ext.max()).astype(np.float64)  # a sphere around the cube

    def fresh(x, tets, points=pts, fix=fixed):
        twin = FemIntegrator(x, tets, fix)
        out = twin.embedding(twin.embed(points))
        twin.close()
        return out

    g = FemIntegrator(v, t, fixed, expect_cuts=True)
    e0, i0 = g.embed(pts, info=True)
    assert i0["n_external"] == 400
    s0 = g.embed_search_info(e0)
    assert s0["path"] == RING and s0["centre_grid_builds"] == 1
    e1 = g.embed(pts)
    assert g.embed_search_info(e1)["centre_grid_builds"] == 1, "a second embedding on the same generation builds nothing"
    _same(g.embedding(e0), g.embedding(e1))
    _same(g.embedding(e0), fresh(v, t))
    # a cut: the next generation
    info, _ = g.cut(cr.plane_strip(lo + 0.5 * ext + [0.0013, 0.0007, 0.0003], (1.0, 0.013, 0.007)), mode="carry")
    assert info["status"] == fl.FB_CUT_DONE
    x2, t2 = g.read_mesh()
    e2 = g.embed(pts)
    s2 = g.embed_search_info(e2)
    assert s2["path"] == RING and s2["n_outside"] == 400 and s2["centre_grid_builds"] == 2
    _same(g.embedding(e2), fresh(x2, t2))
    # a re-sync to another mesh: every live embedding is searched again when next read
    v3, t3, _ = delaunay_jittered(6)
    g.resync(v3, t3, _fixed_of(v3))
    for eid in (e0, e1, e2):  # (the cut has refreshed the location of the points it re-bound: each is searched from its own rest_xyz)
        after = g.embedding(eid)
        _same(after, fresh(v3, t3, after["rest_xyz"], _fixed_of(v3)))
    assert np.array_equal(g.embedding(e2)["rest_xyz"], pts)
    s3 = g.embed_search_info(e0)
    assert s3["path"] == RING and s3["centre_grid_builds"] == 3, "one build for the three searches of this generation"
    g.close()


# ---- 8. the interface ----
def test_search_info_and_timing(gpu, monkeypatch):
    monkeypatch.delenv("FEMBRAIN_EMBED_CLOSEST", raising=False)
    monkeypatch.delenv("FEMBRAIN_EMBED_RING_BUDGET", raising=False)
    v, t = _mesh("cube")
    g = FemIntegrator(v, t, _fixed_of(v))
    for bad in (-1, 0, 3, 8):
        with pytest.raises(fl.FbError) as e:
            g.embed_search_info(bad)
        assert e.value.code == fl.FB_EINVAL
    inside = np.float32(v.min(0) + (0.2 + 0.6 * np.random.default_rng(9).random((50, 3))) * (v.max(0) - v.min(0))).astype(np.float64)
    e_in, info = g.embed(inside, info=True)
    assert info["n_external"] == 0
    assert g.embed_search_info(e_in) == dict(path=NONE, n_outside=0, n_far=0, centre_grid_builds=0, max_centres_one_point=0, centres_tested=0)
    pts = outside_points(v, 40, 42)
    eid, info = g.embed(pts, info=True)
    si = g.embed_search_info(eid)
    assert si["path"] == SCAN and si["n_outside"] == 40 and si["centre_grid_builds"] == 0, "few outside points and no centre grid: the rule scans"
    before = g.embedding(eid)
    for path in (SCAN, RING):
        build, run = g.time_embed_closest(eid, path, reps=3)
        assert run > 0 and (build > 0) == (path == RING)
    for bad_path in (NONE, 3):
        with pytest.raises(fl.FbError) as e:
            g.time_embed_closest(eid, bad_path, reps=1)
        assert e.value.code == fl.FB_EINVAL
    _same(before, g.embedding(eid))
    assert g.embed_update(eid)[2]["n_locates"] == info["n_locates"] == 1
    assert g.embed_search_info(eid) == si, "timing runs on a scratch copy: no centre grid is left behind, no count moves"
    # with a centre grid of this generation in place the rule takes the ring at any count
    monkeypatch.setenv("FEMBRAIN_EMBED_CLOSEST", "ring")
    e2 = g.embed(pts)
    monkeypatch.delenv("FEMBRAIN_EMBED_CLOSEST")
    e3 = g.embed(pts)
    s3 = g.embed_search_info(e3)
    assert s3["path"] == RING and s3["centre_grid_builds"] == 1
    _same(g.embedding(e2), before)
    _same(g.embedding(e3), before)
    g.close()
