"""tests/selfcontactref.py, the numpy restatement of fb_fem_self_contact's rule, against bodycontactref on a shape where the two rules must
say the same, and on the coincident lips of a fresh cut (no GPU)."""
import numpy as np

import bodycontactref as B
import selfcontactref as S

K = 1000.0


def _two_way():
    va, ta, vb, tb = B.two_cubes(*B.SHAPES["two_way"])
    v, t, na, _ = S.union("two_way")
    return (va, ta, vb, tb), (v, t, na)


def test_union_of_two_cubes_is_the_two_directions_of_body_contact():
    (va, ta, vb, tb), (v, t, na) = _two_way()
    two = B.body_contact(va, ta, va, vb, tb, vb, K)
    one = S.self_contact(v, t, v, K, mode=S.ANY)
    ab, ba = two["dirs"]
    assert (len(one["vids"]), len(one["node"]), len(ab["node"]), len(ba["node"])) == (148, 25, 16, 9)
    # a's nodes come first in the union, so its contacts do: a into b, then b into a
    assert np.array_equal(one["node"], np.concatenate([ab["node"], ba["node"] + na]))
    assert np.array_equal(one["element"], np.concatenate([ab["element"] + len(ta), ba["element"]]))
    # the same faces after the index shift, as node triples (the union's surface orders its faces in its own way)
    want_faces = np.concatenate([two["faces_b"][ab["face"]] + na, two["faces_a"][ba["face"]]])
    assert np.array_equal(one["faces"][one["face"]], want_faces)
    for key in ("closest", "bary", "depth", "force"):
        assert np.array_equal(one[key], np.concatenate([ab[key], ba[key]])), key
    assert one["n_dropped"] == 0 and not one["degenerate"].any()
    # one vector: a node of a is pushed as a point and pushes back as a corner
    both_roles = np.intersect1d(one["node"], one["faces"][one["face"]].reshape(-1))
    assert len(both_roles) == 24
    # the sums are the two bodies' sums taken apart by role: record order is the order body_contact adds in inside a direction
    assert np.allclose(one["force_on_points"] + one["force_on_faces"], 0.0, atol=1e-9)
    assert np.allclose(one["f"].sum(axis=0), 0.0, atol=1e-9)
    assert one["max_depth"] == two["max_depth"]


def test_any_and_other_parts_agree_on_the_union():
    _, (v, t, na) = _two_way()
    a, o = S.self_contact(v, t, v, K, mode=S.ANY), S.self_contact(v, t, v, K, mode=S.OTHER_PARTS)
    assert o["n_parts"] == 2
    for key in ("node", "element", "face", "closest", "bary", "depth", "force", "f", "force_on_points", "force_on_faces"):
        assert np.array_equal(a[key], o[key]), key


def test_one_part_has_no_contacts_under_other_parts():
    v, t, cur = S.rolled_beam()
    assert len(S.self_contact(v, t, cur, K, mode=S.ANY)["node"]) == 12
    r = S.self_contact(v, t, cur, K, mode=S.OTHER_PARTS)
    assert r["n_parts"] == 1 and len(r["node"]) == 0 and not r["f"].any()


def test_coincident_lips_push_nothing():
    v, t = S.cut_beam()
    for mode in (S.ANY, S.OTHER_PARTS):
        r = S.self_contact(v, t, v, K, mode=mode)
        assert len(r["vids"]) == 436 and len(r["node"]) > 0
        assert (r["depth"] == 0).all() and r["degenerate"].all() and not r["f"].any()


def test_pressed_lips_and_the_limit_of_any():
    v, t = S.cut_beam()
    cur = S.pressed(v, t)
    a, o = S.self_contact(v, t, cur, K, mode=S.ANY), S.self_contact(v, t, cur, K, mode=S.OTHER_PARTS)
    assert len(a["node"]) == 129 and np.array_equal(a["node"], o["node"])
    assert (a["face"] != o["face"]).any()          # 0.31 of a cell deep: under ANY a face of the vertex's own side can win
    assert round(a["max_depth"], 4) == 0.0275 and round(o["max_depth"], 4) == 0.0309
    assert np.allclose(o["f"].sum(axis=0), 0.0, atol=1e-9)
