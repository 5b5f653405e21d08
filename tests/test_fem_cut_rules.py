"""The restatement behind tests/test_fem_cut_gpu.py (tests/cutref.py) checked on its own, without a GPU: the prism rule, the case tables
derived from it, and one element cut in every case A / B pattern."""
import itertools

import numpy as np
import pytest

import cutref as cr

TET = np.array([[0.05, 0.02, -0.01], [1.1, 0.03, 0.07], [0.13, 0.97, 0.02], [0.04, 0.11, 1.03]])


def one_tet_strip(code):
    """a planar quad that separates the nodes of one tet the way `code` says"""
    if code in cr.CASE_A:
        a = cr.CASE_A[code]
        rest = [k for k in range(4) if k != a]
        far = TET[rest].mean(0)
        return cr.plane_strip(TET[a] + 0.37 * (far - TET[a]), far - TET[a], half=5.0)
    b = cr.CASE_B[code]
    cd = [k for k in (1, 2, 3) if k != b]
    m1, m2 = TET[[0, b]].mean(0), TET[cd].mean(0)
    return cr.plane_strip(m1 + 0.43 * (m2 - m1), m2 - m1, half=5.0)


def test_every_prism_order_splits_into_three_tets_that_fill_it():
    assert cr.all_prism_orders_positive()


def test_case_tables_cover_every_valid_code():
    # case A: 4 codes of 3 edges at a node; case B: 3 codes of 4 edges with the uncut two opposite; nothing else is valid
    valid = set()
    for n in range(4):
        valid.add(sum(1 << cr.edge_of(n, k) for k in range(4) if k != n))
    for x in (1, 2, 3):
        y, z = [k for k in (1, 2, 3) if k != x]
        valid.add(63 ^ (1 << cr.edge_of(0, x)) ^ (1 << cr.edge_of(y, z)))
    assert set(cr.CASE_A) | set(cr.CASE_B) == valid and len(valid) == 7
    for code in valid:
        pieces = cr.piece_tokens(code)
        assert sum(4 if kind == "tet" else 0 for kind, _ in pieces) + sum(6 if kind == "prism" else 0 for kind, _ in pieces) in (10, 12)
        n = sum(1 if kind == "tet" else 3 for kind, _ in pieces)
        assert n == (4 if code in cr.CASE_A else 6)


@pytest.mark.parametrize("code", sorted(set(cr.CASE_A) | set(cr.CASE_B)))
@pytest.mark.parametrize("perm", [(0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)])
def test_one_element_every_case(code, perm):
    # the element's nodes under several numberings: the split depends on the ids, the union of the pieces does not
    tets = np.array([perm], np.int32)
    xyz = np.zeros((4, 3))
    xyz[list(perm)] = TET
    r = cr.cut(xyz, tets, one_tet_strip(code))
    assert r["status"] == 1 and r["codes"][0] == code
    assert len(r["added"]) == (4 if code in cr.CASE_A else 6)
    allx = np.concatenate([xyz, r["new_xyz"]])
    parent = cr.tet_vol6(xyz[tets[0]])
    vols = np.array([cr.tet_vol6(allx[p]) for p in r["added"]])
    assert np.all(np.sign(vols) == np.sign(parent))
    assert abs(vols.sum() - parent) <= 1e-12 * abs(parent)
    # no piece uses both copies of one cut edge
    for p in r["added"]:
        new = p[p >= 4] - 4
        assert len(set(new // 2)) == len(new)
    # the split points lie on their edges at t from lo
    for k in range(r["n_cut_edges"]):
        lo, hi = r["edge_nodes"][2 * k]
        f = r["edge_frac"][2 * k]
        assert 0 < f < 1
        assert np.allclose(r["new_xyz"][2 * k], xyz[lo] + f * (xyz[hi] - xyz[lo]), atol=1e-12)


def test_random_split_fractions_keep_the_orientation():
    # the piece order is chosen combinatorially: any split points strictly inside their edges give pieces of the parent's sign
    rng = np.random.default_rng(3)
    for code in sorted(set(cr.CASE_A) | set(cr.CASE_B)):
        for _ in range(20):
            perm = rng.permutation(4)
            g = np.array(perm)
            pieces = []
            for kind, toks in cr.piece_tokens(code):
                if kind == "tet":
                    pieces.append(cr.orient(toks))
                else:
                    ids = [int(g[t[1]]) if t[0] == "n" else 4 + 2 * cr.edge_of(t[1], t[2]) + (int(g[t[3]]) > int(g[t[1] if t[3] == t[2] else t[2]])) for t in toks]
                    pieces += [cr.orient([toks[k] for k in tt]) for tt in cr.prism_tets(ids)]
            f = rng.uniform(0.05, 0.95, 6)

            def point(t):
                if t[0] == "n":
                    return TET[t[1]]
                e = cr.edge_of(t[1], t[2])
                return TET[t[1]] + f[e] * (TET[t[2]] - TET[t[1]])
            parent = cr.tet_vol6(TET)
            vols = [cr.tet_vol6(np.array([point(t) for t in p])) for p in pieces]
            assert all(np.sign(v) == np.sign(parent) for v in vols)
            assert abs(sum(vols) - parent) <= 1e-12 * abs(parent)


def test_the_odd_count_rule_and_degenerate_quads():
    xyz, tets = TET.copy(), np.array([[0, 1, 2, 3]], np.int32)
    s = one_tet_strip(7)
    assert cr.cut(xyz, tets, np.concatenate([s[:2], s[2:], s[:2], s[2:]]))["status"] == 1  # quads 0 and 2 equal, quad 1 crosses (s2 s3 s0 s1)
    two = np.concatenate([s, s])  # quads 0 and 2 cut the same edges: an even count
    r = cr.cut(xyz, tets, two)
    assert r["n_quads"] == 3
    flat = np.repeat(s[:1], 4, axis=0)
    assert cr.cut(xyz, tets, flat)["n_quads"] == 0
