"""The independent checker (tests/cutchecks.py) and the restatement (tests/cutref.py) against each other, without a GPU, on the inputs of
tests/test_fem_cut_unstructured_gpu.py (tests/cut_inputs.py); doctored deltas show that the checker fails where it should."""
import warnings

import numpy as np
import pytest

import cut_inputs as ci
import cutchecks as cc
import cutref as cr
from fembrain_amd.meshgen import truth_cube


def _bodies_cut(v, t, plane):
    """how many face-connected components a cut by the plane adds: the parts of every element on either side (one or two), joined across a
    face where the face has a node on that side -- stated on the uncut mesh, without a piece table"""
    t = np.asarray(t, np.int64)
    m = len(t)
    side = (v - plane[0]) @ plane[1] > 0
    has = np.stack([(~side[t]).any(1), side[t].any(1)], axis=1)          # element e has a part on side s
    faces, owner = cc._faces(t)
    order = np.lexsort(faces.T[::-1])
    fs, ow = faces[order], owner[order]
    same = np.nonzero(np.all(fs[1:] == fs[:-1], axis=1))[0]
    parent = np.arange(2 * m)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in same:
        for s in (0, 1):
            if (side[fs[i]] == bool(s)).any():
                a, b = find(2 * ow[i] + s), find(2 * ow[i + 1] + s)
                parent[a] = b
    after = len({find(2 * e + s) for e in range(m) for s in (0, 1) if has[e, s]})
    return after - len(np.unique(cr.face_components(t)))


def _delaunay_cuts():
    for n, seed, pseed, k in ci.DELAUNAY_CASES:
        v, t, _ = ci.delaunay(n, seed)
        for q in (None, ci.smooth_displacement(v)):
            for mode in ("bake", "carry"):
                for p, nrm, s in ci.random_planes(pseed, k):
                    yield v, t, q, mode, p, nrm, s


def test_the_restatement_passes_the_checker_on_delaunay_meshes_and_reaches_every_pair():
    cov, worst = set(), 0.0
    for v, t, q, mode, p, nrm, s in _delaunay_cuts():
        e = cr.cut(v, t, s, q, mode)
        assert e["status"] == 1
        pos = v if q is None else v + q
        cov |= cc.check_cut(pos, t, e, strip=s, plane=(p, nrm), rest=v if mode == "carry" else None, components=2)
    assert len(cov) == cc.ALL_PAIRS == 168
    # the cubes and planes of tests/test_fem_cut_gpu.py reach 20 of them
    cube = set()
    for n in (6, 12, 13):
        v, t = truth_cube(n, n, n, 0.1)
        lo, hi = v.min(0), v.max(0)
        for s in (cr.plane_strip(lo + (hi - lo) * [0.47, 0.5, 0.5] + [0.013, 0, 0], (1.0, 0.013, 0.007), half=10.0),
                  cr.plane_strip(lo + (hi - lo) * [0.5, 0.53, 0.5], (0.013, 1.0, 0.021), half=10.0)):
            e = cr.cut(v, t, s)
            if e["status"] == 1:
                cube |= cc.coverage(t, e)
    assert len(cube) < 40


@pytest.mark.parametrize("name", ci.SHIPPED)
def test_the_restatement_passes_the_checker_on_shipped_meshes(name):
    v, t, _ = ci.shipped(name)
    before = len(np.unique(cr.face_components(t)))
    if name in ci.SHIPPED_BODIES:
        assert before == ci.SHIPPED_BODIES[name]
    else:
        assert before == 624  # implicit_sphere: every polygonizer cell on its own
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (zero-length edges between unwelded twins used to raise "invalid value" in cutref.segments)
        for p, nrm, s in ci.shipped_planes(name, v):
            e = cr.cut(v, t, s)
            assert e["status"] == 1
            cc.check_cut(v, t, e, strip=s, plane=(p, nrm), components=before + _bodies_cut(v, t, (p, nrm)))


def test_zero_length_edges_are_never_cut():
    # two coincident nodes joined by an edge (a collapsed element beside a sound one): the edge has no direction, 0 * inf stays out of it
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0], [1, 0, 0]])
    lo, hi = np.array([1, 0]), np.array([4, 1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rd, ln = cr.segments(v[lo], v[hi])
        cut, _ = cr.cut_edges(v, lo, hi, cr.usable_quads(cr.plane_strip((1.0, 0, 0), (1, 0.1, 0), half=5.0)))
    assert ln[0] == 0.0 and not np.any(rd[0]) and np.isfinite(rd).all()
    assert cut[1]


def test_folded_strips_and_the_narrow_v():
    v, t, _ = ci.delaunay(*ci.FOLD_MESH)
    done = 0
    for nq, fold, seed in ci.FOLDED_CASES:
        s = ci.folded_strip(nq, fold, seed)
        e = cr.cut(v, t, s)
        assert e["n_quads"] == nq
        if e["status"] == 1:
            done += 1
            cc.check_cut(v, t, e)
    assert done >= 8
    for a in ci.V_CASES:
        e = cr.cut(v, t, ci.v_strip(a))
        assert e["status"] == 1 and e["n_quads"] == 2
        cc.check_cut(v, t, e)
        # an edge that crosses both wings is not cut: cells crossed by both come out as case B through the odd-count rule alone
        q = cr.usable_quads(ci.v_strip(a))
        ed = np.unique(np.sort(t[:, [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]].reshape(-1, 2), axis=1), axis=0)
        h0, _ = cr.cut_edges(v, ed[:, 0], ed[:, 1], q[:1])
        h1, _ = cr.cut_edges(v, ed[:, 0], ed[:, 1], q[1:])
        both = set(map(tuple, ed[h0 & h1].tolist()))
        assert len(both) > 20
        cells = [i for i in e["removed"] if any((min(t[i][x], t[i][y]), max(t[i][x], t[i][y])) in both for x, y in cc.EDGES)]
        # (... or as case A where one node lies between the wings)
        assert sum(bin(int(e["codes"][i])).count("1") == 4 for i in cells) > 10 and len(cells) > 40
    e = cr.cut(v, t, ci.ending_blade())
    assert e["status"] == 2 and e["n_unhandled"] > 10


def test_node_touching_blades_are_unhandled_by_the_restatement():
    v, t = truth_cube(7, 7, 7, 0.1)
    for nrm, n_unh in ci.TOUCHING_NORMALS:
        e = cr.cut(v, t, ci.touching_blade(v, nrm))
        assert e["status"] == 2 and e["n_unhandled"] == n_unh, (nrm, e["n_unhandled"])


def test_the_zero_volume_state_is_reachable():
    t = np.array([[0, 1, 2, 3]], np.int32)
    for p in ((1.0, 0, 0), (0.0, 0, 0)):
        e = cr.cut(ci.UNIT_TET, t, cr.plane_strip(p, (1, 0, 0), half=5.0))
        assert e["status"] == 1 and e["codes"][0] == 25 and e["min_volume_ratio"] == 0.0
        assert sorted(np.abs(e["edge_frac"][::2]).tolist()) in ([0.0, 0.0, 1.0], [0.0, 1.0, 1.0])
    e = cr.cut(ci.UNIT_TET, t, cr.plane_strip((0.0, 0, 0), (1, 1, 1), half=5.0))
    assert e["status"] == 1 and e["codes"][0] == 7 and 0 < e["min_volume_ratio"] < 1e-45
    # ... the piece at node 0 has a volume no float holds, the other three do
    x2, t2 = ci.cut_mesh(ci.UNIT_TET, t, e)
    vol = np.abs(cc.vol6(x2, t2)) / 6
    assert np.float32(vol.min()) == 0 and np.sum(vol.astype(np.float32) >= np.finfo(np.float32).tiny) == 3
    for x, ratio in ((1e-5, 1e-5), (1 - 1e-5, 1e-15)):
        e = cr.cut(ci.UNIT_TET, t, cr.plane_strip((x, 0, 0), (1, 0, 0), half=5.0))
        assert e["status"] == 1 and e["min_volume_ratio"] == pytest.approx(ratio, rel=1e-4)
        x2, t2 = ci.cut_mesh(ci.UNIT_TET, t, e)
        assert np.all((np.abs(cc.vol6(x2, t2)) / 6).astype(np.float32) >= np.finfo(np.float32).tiny)
        cc.check_cut(ci.UNIT_TET, t, e)


def test_split_tolerance_is_four_times_the_measured_error():
    worst = 0.0
    for v, t, q, mode, p, nrm, s in _delaunay_cuts():
        e = cr.cut(v, t, s, q, mode)
        d, _, scale = cc.split_errors(v if q is None else v + q, e, s, v if mode == "carry" else None)
        worst = max(worst, d.max() / scale)
    for name in ci.SHIPPED:
        v, t, _ = ci.shipped(name)
        for p, nrm, s in ci.shipped_planes(name, v):
            d, _, scale = cc.split_errors(v, cr.cut(v, t, s), s)
            worst = max(worst, d.max() / scale)
    print("largest split-point error normal to the blade / coordinate scale: %.3e" % worst)
    assert 0.5 * cc.SPLIT_MEASURED <= worst <= cc.SPLIT_MEASURED and cc.SPLIT_TOL == 4 * cc.SPLIT_MEASURED


# ---- the checker fails on doctored deltas ----
def _case():
    v, t, _ = ci.delaunay(*ci.FOLD_MESH)
    p, nrm, s = ci.random_planes(3, 1)[0]
    e = cr.cut(v, t, s)
    cc.check_cut(v, t, e, strip=s, plane=(p, nrm))
    return v, t, e, (p, nrm), s


def _pieces_of(t, e, i):
    n = np.where(np.array([bin(int(c)).count("1") for c in cc.parent_codes(t, e)]) == 3, 4, 6)
    first = np.concatenate([[0], np.cumsum(n)])
    return first[i], first[i + 1]


def test_checker_fails_when_one_prism_is_split_by_the_other_diagonal():
    v, t, e, plane, s = _case()
    N = len(v)
    allx = np.concatenate([v, e["new_xyz"]])
    f, own = cc._faces(t)
    keys, cnt = np.unique(cc._face_keys(f, N), return_counts=True)
    shared = set(keys[cnt == 2].tolist())
    for i, el in enumerate(e["removed"]):
        a, b = _pieces_of(t, e, i)
        g = t[el].astype(np.int64)
        inner = all(k in shared for k in cc._face_keys(np.sort(g[[list(fc) for fc in cc._FACES]], axis=1), N).tolist())
        if b - a != 4 or not inner:
            continue
        # case A, every face shared: piece 0 is the tet at the isolated node, pieces 1..3 the prism of three split points over three old nodes
        top = sorted(set(e["added"][a + 1:b].reshape(-1).tolist()) - set(g.tolist()))
        iso = [n for n in e["added"][a] if n < N][0]
        bottom = [[n for n in e["edge_nodes"][m - N] if n != iso][0] for m in top]
        ids = top + bottom
        # the same prism split as if its old nodes were numbered the other way round: a valid split, through the other diagonal of its quads
        # (negating all six ids changes nothing: the new nodes are numbered in the order of their old ends)
        other = [[ids[k] for k in tt] for tt in cr.prism_tets(top + [-n for n in bottom])]
        if set(map(frozenset, other)) == set(map(frozenset, e["added"][a + 1:b].tolist())):
            continue
        d = {k: np.array(val, copy=True) if isinstance(val, np.ndarray) else val for k, val in e.items()}
        sign = np.sign(cc.vol6(v, g[None])[0])
        for j, pc in enumerate(other):
            pc = np.array(pc)
            if np.sign(cc.vol6(allx, pc[None])[0]) != sign:
                pc[[2, 3]] = pc[[3, 2]]
            d["added"][a + 1 + j] = pc
        with pytest.raises(AssertionError, match="different diagonals"):
            cc.check_cut(v, t, d, plane=plane)
        return
    pytest.fail("no inner case A parent whose prism has another split")


def test_checker_fails_when_two_coincident_nodes_are_swapped_in_one_piece():
    v, t, e, plane, s = _case()
    N = len(v)
    d = {k: np.array(val, copy=True) if isinstance(val, np.ndarray) else val for k, val in e.items()}
    p = d["added"][5]
    k = int(np.nonzero(p >= N)[0][0])
    p[k] = N + ((p[k] - N) ^ 1)   # the other copy: same coordinates, the other side's node
    with pytest.raises(AssertionError, match="other side's copy"):
        cc.check_cut(v, t, d, plane=plane)


def test_checker_fails_when_one_piece_is_reversed():
    v, t, e, plane, s = _case()
    d = {k: np.array(val, copy=True) if isinstance(val, np.ndarray) else val for k, val in e.items()}
    big = int(np.argmax(e["ratios"]))
    d["added"][big] = d["added"][big][[0, 1, 3, 2]]
    with pytest.raises(AssertionError, match="reversed"):
        cc.check_cut(v, t, d, plane=plane)
