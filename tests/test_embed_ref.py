"""The numpy restatement of fb_fem_embed's binding rule (tests/embedref.py) against what the reference's own
VolumetricMesh::generateInterpolationWeights returned (tests/golden/embed_ref.npz, made by tests/golden/make_embed_golden.py): no GPU.

Every generic point of the fixture is asserted to BE generic (embedref.margin >= 1e-9: no weight of the point, in any element, close enough
to zero for a rounding to flip it, and no two centres close enough to tie), so elements must agree exactly and weights within
embedref.weight_bound.  The eleven degenerate points (ten nodes, one face centroid) lie in several elements up to rounding; for them the
reference's choice must be one the restatement finds containing within 1e-12."""
import os

import numpy as np
import pytest

import embedref as er

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-9


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "embed_ref.npz"))


def test_the_fixture_is_small():
    assert os.path.getsize(os.path.join(HERE, "golden", "embed_ref.npz")) < 300 * 1000


@pytest.mark.parametrize("name", ["cube", "beam3"])
def test_restatement_equals_the_reference(golden, name):
    v, t = golden[name + "_verts"], golden[name + "_tets"]
    gen, deg = golden[name + "_generic"].astype(np.float64), golden[name + "_degenerate"]
    n = len(gen)
    assert n == 3000 and len(deg) == 11
    assert {"cube": (64, 162), "beam3": (208, 450)}[name] == (len(v), len(t))
    W = er.all_weights(v, t, gen)
    m = er.margin(v, t, gen, W)
    print("%s: smallest margin %.3g" % (name, m.min()))
    assert (m >= MARGIN).all(), "every generic point of the fixture is generic"
    ref = er.bind(v, t, gen, W=W)
    assert np.array_equal(ref["elements"], golden[name + "_elements"][:n])
    assert np.array_equal(ref["vertices"], golden[name + "_vertices"][:n])
    err = np.abs(ref["weights"] - golden[name + "_weights"][:n]).max(axis=1)
    print("%s: weights differ by at most %.3g, largest error / bound %.3g" % (name, err.max(), (err / ref["bound"]).max()))
    assert (err <= ref["bound"]).all()
    assert 0 < ref["n_external"] < n
    # the count of the whole run: the generic points' and however many of the degenerate ones the reference found outside
    d = er.bind(v, t, deg, tol=1e-12)
    assert ref["n_external"] <= int(golden[name + "_n_external"]) <= ref["n_external"] + len(deg)
    for k in range(len(deg)):
        e = golden[name + "_elements"][n + k]
        assert e in d["containing"][k], (k, e, d["containing"][k])
        assert np.array_equal(golden[name + "_vertices"][n + k], t[e])
        w = golden[name + "_weights"][n + k]
        assert abs(w.sum() - 1.0) <= 1e-12 and np.abs(w @ v[t[e]] - deg[k]).max() <= 1e-12 * np.linalg.norm(v.max(0) - v.min(0))


def test_generic_points_are_float32_values_inside_the_grown_box():
    v, _ = er.jittered_cube()
    p = er.generic_points(v, 500, 3)
    lo, hi = v.min(0), v.max(0)
    assert np.array_equal(np.float32(p).astype(np.float64), p)
    assert (p >= lo - 0.1001 * (hi - lo)).all() and (p <= hi + 0.1001 * (hi - lo)).all()
    assert ((p < lo) | (p > hi)).any()


def test_weight_bound_holds_between_two_evaluation_orders():
    # the same weights from determinants expanded about the point instead (another, equally valid order of the operations)
    v, t = er.jittered_cube()
    p = er.generic_points(v, 400, 4)
    b = er.bind(v, t, p)
    x = v[t[b["elements"]]]
    d0 = np.linalg.det(x[:, 1:] - x[:, :1])
    w = np.empty((len(p), 4))
    for i in range(4):
        y = x.copy()
        y[:, i] = p
        w[:, i] = np.linalg.det(y[:, 1:] - y[:, :1]) / d0
    assert (np.abs(w - b["weights"]).max(axis=1) <= b["bound"]).all()


def test_positions_and_normals_of_a_flat_patch():
    v, t = er.jittered_cube()
    lo, ext = v.min(0), v.max(0) - v.min(0)
    p = lo + ext * np.array([[0.3, 0.3, 0.45], [0.7, 0.3, 0.45], [0.3, 0.7, 0.45], [0.7, 0.7, 0.45], [0.15, 0.15, 0.15]])
    tri = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    b = er.bind(v, t, p)
    assert not b["external"].any()
    at_rest = er.positions(v, np.zeros(v.size), b["vertices"], b["weights"])
    assert np.abs(at_rest - p).max() <= 1e-15
    shifted = er.positions(v, np.tile([0.01, -0.02, 0.03], len(v)), b["vertices"], b["weights"])
    assert np.abs(shifted - (p + [0.01, -0.02, 0.03])).max() <= 1e-15
    n = er.normals(at_rest, tri)
    assert np.allclose(n[:4], [0, 0, 1], atol=1e-12) and not n[4].any()


# ---- the rule for a cut ----
def _cube6():
    from fembrain_amd.meshgen import truth_cube
    v, t = truth_cube(6, 6, 6, 0.1)
    return np.array(v, np.float64).reshape(-1, 3), np.array(t, np.int32).reshape(-1, 4)


@pytest.mark.parametrize("mode", ["bake", "carry"])
@pytest.mark.parametrize("mesh", ["cube", "delaunay"])
def test_the_pieces_of_a_parent_tile_it(mesh, mode):
    import cut_inputs as ci
    import cutref as cr
    if mesh == "cube":
        v, t = _cube6()
        strip = cr.plane_strip(0.5 * (v.min(0) + v.max(0)) + [0.0013, 0.0007, 0.0003], (1.0, 0.013, 0.007))
    else:
        v, t, _ = ci.delaunay(400, 7)
        strip = ci.folded_strip(4, 0.15, 45)
    q = ci.smooth_displacement(v)
    d = cr.cut(v, t, strip, q=q, mode=mode)
    assert d["status"] == 1 and len(d["removed"]) > 20
    x_new, t_new = ci.cut_mesh(v + q if mode == "bake" else v, t, d)
    pts = er.generic_points(v, 700, 81, grow=0.05)
    b = er.bind(v, t, pts)
    b["rest_xyz"] = pts
    f = er.follow_cut(t, b, d, x_new, t_new, mode == "bake")
    inside = f["rebound"] & ~b["external"]
    assert inside.sum() > 15
    assert f["margin"][f["rebound"]].min() >= MARGIN, "every re-bound point of the fixture is generic"
    # a point its parent contained is contained in the piece it was given: the pieces leave no gap
    w, _ = er.weights_in(x_new, t_new, f["rest_xyz"][inside], f["elements"][inside])
    assert (w >= 0).all()
    assert (np.abs(w - f["weights"][inside]) == 0).all()
    # kept points: the same weights, the element's new id names the same four nodes
    kept = ~f["rebound"]
    assert np.array_equal(f["weights"][kept], b["weights"][kept]) and np.array_equal(t_new[f["elements"][kept]], t[b["elements"][kept]])
    # where the point is: unchanged by a carry cut (up to the rounding of the weighted sum), moved with the rest shape by a bake
    if mode == "carry":
        assert np.abs(f["rest_xyz"] - pts).max() <= 1e-12
    else:
        assert np.abs(f["rest_xyz"][~b["external"]] - pts[~b["external"]]).max() <= 2 * np.abs(q).max()
