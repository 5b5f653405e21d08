"""tests/bodycontactref.py, the numpy restatement of fb_fem_body_contact's rule, on cases with known answers (no GPU)."""
import numpy as np

import bodycontactref as R

# the unit cube as five elements: the corner elements and the inner one
CUBE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]], np.float64)
CUBE_TETS = np.array([[0, 1, 2, 4], [3, 2, 1, 7], [5, 4, 7, 1], [6, 7, 4, 2], [1, 2, 4, 7]], np.int32)


def _point_body(p):
    """a tiny element whose node 0 is the point p and whose other nodes lie far outside the cube"""
    x = np.array([p, [5, 5, 5], [6, 5, 5], [5, 6, 5]], np.float64)
    return x, np.array([[0, 1, 2, 3]], np.int32)


def _one_point(p, stiffness=100.0, depth_cap=0.0):
    xa, ta = _point_body(p)
    r = R.body_contact(xa, ta, xa, CUBE, CUBE_TETS, CUBE, stiffness, depth_cap, directions=R.A_INTO_B)
    d = r["dirs"][0]
    assert list(d["candidates"]) == [0] and list(d["node"]) == [0]
    return r, d


def test_closest_point_regions():
    a, b, c = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1, 0])
    cases = [((-1, -1, 1), (0, 0, 0), (0, 0)), ((2, -1, 0), (1, 0, 0), (1, 0)), ((0.25, -1, 0), (0.25, 0, 0), (0.25, 0)), ((-1, 2, 0), (0, 1, 0), (0, 1)),
             ((-1, 0.5, 2), (0, 0.5, 0), (0, 0.5)), ((1, 1, 0), (0.5, 0.5, 0), (0.5, 0.5)), ((0.25, 0.25, 3), (0.25, 0.25, 0), (0.25, 0.25))]
    for p, q, vw in cases:
        got, v, w = R.closest_on_triangle(np.array(p, np.float64), a, b, c)
        assert np.array_equal(got, np.array(q, np.float64)) and (float(v), float(w)) == vw, (p, got, v, w)


def test_point_in_cube_is_pushed_to_the_nearest_face():
    r, d = _one_point((0.5, 0.3, 0.1))
    faces = r["faces_b"]
    assert abs(d["depth"][0] - 0.1) < 1e-15 and np.allclose(d["closest"][0], (0.5, 0.3, 0.0), atol=1e-15)
    assert set(CUBE[faces[d["face"][0]]][:, 2]) == {0.0}        # a face of the side z = 0
    assert np.allclose(d["force"][0], (0, 0, -100.0 * 0.1), atol=1e-12)
    assert abs(d["bary"][0].sum() - 1) < 1e-15 and (d["bary"][0] >= 0).all()
    assert np.allclose((d["bary"][0][:, None] * CUBE[faces[d["face"][0]]]).sum(axis=0), d["closest"][0], atol=1e-15)
    assert d["contain_margin"][0] > 0.01 and d["gap"][0] > 0.05    # (the side's other triangle is 0.073 further)


def test_equal_distances_take_the_lower_face():
    r, d = _one_point((0.25, 0.25, 0.7))   # as far from x = 0 as from y = 0, in binary exactly
    faces = r["faces_b"]
    tri = CUBE[faces]
    q, _, _ = R.closest_on_triangle(np.array([0.25, 0.25, 0.7]), tri[:, 0], tri[:, 1], tri[:, 2])
    dist = R.distance(np.array([0.25, 0.25, 0.7]), q)
    tied = np.nonzero(dist == dist.min())[0]
    assert len(tied) >= 2 and dist.min() == 0.25
    assert d["face"][0] == tied.min()
    assert d["gap"][0] == 0.0                                    # (... and the margin says so: the tests leave such a point out)


def test_forces_sum_to_zero():
    for shape in R.SHAPES.values():
        va, ta, vb, tb = R.two_cubes(*shape)
        r = R.body_contact(va, ta, va, vb, tb, vb, 1000.0)
        n = sum(len(d["node"]) for d in r["dirs"])
        assert n > 0
        scale = 1000.0 * r["max_depth"] * 3 * n
        assert np.abs(r["force_on_a"] + r["force_on_b"]).max() <= 8 * 2.0 ** -52 * scale
        assert np.abs(r["fa"].sum(axis=0) + r["fb"].sum(axis=0)).max() <= 8 * 2.0 ** -52 * scale
        assert np.abs(r["fa"].sum(axis=0) - r["force_on_a"]).max() <= 8 * 2.0 ** -52 * scale


def test_depth_cap_clamps():
    r0, d0 = _one_point((0.5, 0.3, 0.1))
    r1, d1 = _one_point((0.5, 0.3, 0.1), depth_cap=0.04)
    assert d1["depth"][0] == d0["depth"][0] and r1["max_depth"] == 0.04
    assert np.allclose(d1["force"][0], (0, 0, -100.0 * 0.04), atol=1e-12)
    r2, d2 = _one_point((0.5, 0.3, 0.1), depth_cap=0.5)          # a cap above the depth changes nothing
    assert np.array_equal(d2["force"], d0["force"])


def test_quoted_counts_of_the_shapes():
    want = {"two_way": (16, 9), "many_onto_one": (392, 4), "deep": (26, 0)}
    for name, shape in R.SHAPES.items():
        va, ta, vb, tb = R.two_cubes(*shape)
        r = R.body_contact(va, ta, va, vb, tb, vb, 1000.0)
        assert tuple(len(d["node"]) for d in r["dirs"]) == want[name]
        for k, d in enumerate(r["dirs"]):
            body = vb if k == 0 else va
            cand_ok, contact_ok = R.generic(d, float((body.max(axis=0) - body.min(axis=0)).max()))
            assert cand_ok.all() and contact_ok.all()               # nothing is left out in the structured cases
        if name == "deep":
            depth = r["dirs"][0]["depth"]
            assert 0.36 < depth.min() and depth.max() < 0.44 and len(r["dirs"][1]["candidates"]) == 0


def test_disjoint_boxes_and_wider_format():
    va, ta, vb, tb = R.two_cubes((3, 3, 3, 0.1), (3, 3, 3, 0.1), (0.5, 0.0, 0.0))
    r = R.body_contact(va, ta, va, vb, tb, vb, 1000.0)
    assert all(not d["boxes_meet"] and len(d["candidates"]) == 0 for d in r["dirs"]) and not r["fa"].any() and not r["fb"].any()
    va, ta, vb, tb = R.two_cubes(*R.SHAPES["two_way"])
    r64 = R.body_contact(va, ta, va, vb, tb, vb, 1000.0)
    rld = R.body_contact(va, ta, va, vb, tb, vb, 1000.0, dtype=np.longdouble)
    assert R.spread(r64, rld) <= 64 * 2.0 ** -52 * 1000.0 * r64["max_depth"]
