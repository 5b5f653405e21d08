"""fb_fem_embed / fb_fem_read_embedding / fb_fem_embed_update on the device against the reference's own results (tests/golden/embed_ref.npz)
and the numpy restatement of the rule (tests/embedref.py, pinned to the golden without a GPU by tests/test_embed_ref.py).

Generic points -- every weight of the point, over ALL elements, at least 1e-9 from zero, and for external points the two closest centres
at least 1e-9 apart, relatively; asserted for every point of every case, by choice of seed -- must get the restatement's element and
caller vertex ids exactly and its weights within embedref.weight_bound.  Degenerate points (on a node, an edge, a face; an exact tie of
two centres) are in several elements up to rounding: the chosen element must be one the restatement finds containing within 1e-12, the
weights must sum to 1 (within four times the weight bound of the chosen element: the sum is exact in exact arithmetic) and reproduce
the point within 1e-12 of the box diagonal; the exact tie must go to the lower id."""
import os

import numpy as np
import pytest

import cut_inputs as ci
import embedref as er
from fembrain_amd import lib as fl
from fembrain_amd.fem import Deformable, FemIntegrator
from fembrain_amd.meshgen import delaunay_jittered, fixed_vertices_to_dofs, truth_cube

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OFF, ON = fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON
MARGIN = 1e-9
NORMAL_TOL, MIN_SUM = 2e-7, 1e-3  # tests/test_fem_surface_gpu.py's bound for a normal component, and where it applies


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "embed_ref.npz"))


def _fixed_of(v):
    return fixed_vertices_to_dofs(np.nonzero(v[:, 0] <= v[:, 0].min() + 1e-12)[0].astype(np.int32))


def _shuffled(v, t, seed=3):
    perm = np.random.default_rng(seed).permutation(len(v))  # new id of old node
    v2 = np.empty_like(v)
    v2[perm] = v
    return v2, np.ascontiguousarray(perm[t].astype(np.int32))


def _degenerate(v, t):
    """nodes, edge midpoints and face centroids of a few elements spread over the mesh"""
    el = np.linspace(0, len(t) - 1, 6).astype(int)
    p = [v[t[el, 0]], v[t[el, 3]], 0.5 * (v[t[el, 0]] + v[t[el, 1]]), 0.5 * (v[t[el, 2]] + v[t[el, 3]]),
         (v[t[el, 0]] + v[t[el, 1]] + v[t[el, 2]]) / 3.0, (v[t[el, 1]] + v[t[el, 2]] + v[t[el, 3]]) / 3.0]
    return np.vstack(p)


def _check_generic(v, t, pts, got, info, ref=None, zero_threshold=0.0):
    """the device's binding of generic points equal to the restatement's (ref: a bind() made before)"""
    W = er.all_weights(v, t, pts)
    m = er.margin(v, t, pts, W)
    assert m.min() >= MARGIN, "a generic point of the fixture is not generic: margin %.3g" % m.min()
    ref = ref or er.bind(v, t, pts, zero_threshold, W=W)
    assert np.array_equal(got["elements"], ref["elements"])
    assert np.array_equal(got["vertices"], ref["vertices"])
    err = np.abs(got["weights"] - ref["weights"]).max(axis=1)
    print("weights: max error %.3g, largest error / bound %.3g" % (err.max(), (err / ref["bound"]).max()))
    assert (err <= ref["bound"]).all()
    assert np.array_equal(got["weights"] == 0, ref["weights"] == 0)
    if info is not None:
        assert info["n_external"] == ref["n_external"] and info["n_zeroed"] == ref["n_zeroed"]
    return ref


def _check_degenerate(v, t, pts, got):
    ref = er.bind(v, t, pts, tol=1e-12)
    diag = np.linalg.norm(v.max(0) - v.min(0))
    for k in range(len(pts)):
        assert got["elements"][k] in ref["containing"][k], (k, got["elements"][k], ref["containing"][k])
        assert np.array_equal(got["vertices"][k], t[got["elements"][k]])
    # The sum is exactly 1 in exact arithmetic, and each of the four weights is off by at most the forward bound of its element.  A node
    # also lies in every sliver that has it as a vertex, and the lowest-numbered such element may be one: its |D_0| is small and its
    # bound is above 1e-12 (1.6e-12 was seen on the Delaunay mesh), so no fixed figure holds for the sum; where the bound is below
    # 1e-12 it is the tighter of the two and is what is asked.  The point itself must come back within 1e-12 of the diagonal either way.
    assert (np.abs(got["weights"].sum(axis=1) - 1.0) <= 4 * er.weight_bound(v, t, pts, got["elements"]) + 4 * er.U).all()
    back = (got["weights"][:, :, None] * v[got["vertices"]]).sum(axis=1)
    assert np.abs(back - pts).max() <= 1e-12 * diag


# ---- 1. the binding ----
@pytest.mark.parametrize("renumber", [OFF, ON])
@pytest.mark.parametrize("name", ["cube", "beam3"])
def test_binding_equals_the_reference_and_the_restatement(gpu, golden, name, renumber):
    v, t = golden[name + "_verts"], golden[name + "_tets"]
    gen, deg = golden[name + "_generic"].astype(np.float64), golden[name + "_degenerate"]
    gold_vertices = golden[name + "_vertices"]
    if renumber == ON:  # the same mesh under shuffled node ids, on a handle that works in an order of its own: the record's ids through the shuffle
        gold_vertices = np.random.default_rng(3).permutation(len(v))[gold_vertices]
        v, t = _shuffled(v, t, seed=3)
    g = FemIntegrator(v, t, _fixed_of(v), renumber=renumber)
    assert g.renumbering()[0] == (renumber == ON)
    eid, info = g.embed(np.vstack([gen, deg]), info=True)
    got = g.embedding(eid)
    n = len(gen)
    head = {k: a[:n] for k, a in got.items()}
    ref = _check_generic(v, t, gen, head, None)
    # the reference's own record: elements and vertices exact, weights within the bound (its arithmetic is the restatement's)
    assert np.array_equal(head["elements"], golden[name + "_elements"][:n]) and np.array_equal(head["vertices"], gold_vertices[:n])
    assert (np.abs(head["weights"] - golden[name + "_weights"][:n]).max(axis=1) <= ref["bound"]).all()
    assert np.array_equal(got["rest_xyz"], np.vstack([gen, deg]))
    assert info["n_points"] == n + len(deg) and info["n_locates"] == 1 and info["n_rebound"] == 0 and info["n_zeroed"] == 0
    # (the degenerate points may fall either side of a face of the hull: the external count is pinned on the generic ones)
    assert ref["n_external"] <= info["n_external"] <= ref["n_external"] + len(deg)
    e2, i2 = g.embed(gen, info=True)
    assert e2 != eid and i2["n_external"] == ref["n_external"]
    # the gathers of the update go through the internal ids: at rest the points come back, one float rounding of the fp64 sum
    want = np.float32(er.positions(v, np.zeros(v.size), gold_vertices[:n], golden[name + "_weights"][:n]))
    xyz = g.embed_update(e2)[0]
    assert (np.abs(xyz.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    _check_degenerate(v, t, np.vstack([deg, _degenerate(v, t)]), g.embedding(g.embed(np.vstack([deg, _degenerate(v, t)]))))
    g.close()


@pytest.mark.parametrize("renumber", [OFF, ON])
def test_binding_on_a_delaunay_mesh_under_shuffled_ids(gpu, renumber):
    v, t, _ = delaunay_jittered(6)
    if renumber == ON:
        v, t = _shuffled(v, t)
    g = FemIntegrator(v, t, _fixed_of(v), renumber=renumber)
    assert g.renumbering()[0] == (renumber == ON)
    pts = er.generic_points(v, 1500, 21)
    eid, info = g.embed(pts, info=True)
    _check_generic(v, t, pts, g.embedding(eid), info)
    deg = _degenerate(v, t)
    _check_degenerate(v, t, deg, g.embedding(g.embed(deg)))
    g.close()


def test_an_exact_tie_of_two_centres_goes_to_the_lower_id(gpu):
    # two elements mirrored in the plane x = 0 on dyadic coordinates (the second with two vertices swapped: the same orientation), and
    # points of that plane outside both: the two distances are the same bits
    a = np.array([[-1.0, 0, 0], [-0.5, 0, 0], [-0.75, 0.5, 0], [-0.75, 0, 0.5]])
    b = a[[1, 0, 2, 3]] * [-1.0, 1, 1]
    v = np.vstack([a, b])
    t = np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.int32)
    pts = np.array([[0.0, 4.0, 0.25], [0.0, -2.5, 1.0], [0.0, 0.125, 0.125]])
    d = er.centre_distances(v, t, pts)
    assert np.array_equal(d[:, 0], d[:, 1])
    for tets in (t, t[::-1].copy()):
        g = FemIntegrator(v, tets, np.arange(3, dtype=np.int32))
        eid, info = g.embed(pts, info=True)
        got = g.embedding(eid)
        assert info["n_external"] == 3 and np.array_equal(got["elements"], [0, 0, 0]) and np.array_equal(got["vertices"], np.tile(tets[0], (3, 1)))
        assert np.array_equal(got["weights"], er.bind(v, tets, pts)["weights"])
        g.close()
    # the same pair with 300 far elements between them in the list: the closest-centre pass works through the list in chunks, and the
    # two tied elements fall into different ones
    k = np.arange(300)
    far = (a[None, :, :] + np.stack([np.zeros(300), 64.0 + k, np.zeros(300)], axis=1)[:, None, :]).reshape(-1, 3)
    v3 = np.vstack([a, far, b])
    t3 = np.vstack([t[:1], (4 + 4 * k)[:, None] + np.arange(4)[None, :], [[1204, 1205, 1206, 1207]]]).astype(np.int32)
    for tets, low in ((t3, 0), (t3[::-1].copy(), 0)):
        g = FemIntegrator(v3, tets, np.arange(3, dtype=np.int32))
        eid, info = g.embed(pts, info=True)
        got = g.embedding(eid)
        ref = er.bind(v3, tets, pts)
        assert info["n_external"] == 3 and np.array_equal(got["elements"], [low] * 3) and np.array_equal(ref["elements"], [low] * 3)
        assert np.array_equal(got["weights"], ref["weights"])
        g.close()


# ---- 2. elements of the overflow list ----
@pytest.mark.parametrize("renumber", [OFF, ON])
@pytest.mark.parametrize("first", [False, True])
def test_wide_elements(gpu, first, renumber):
    cv, ct = er.jittered_cube()
    n0 = len(cv)
    # one large element over four far nodes, beside the cube (last) or over a corner of it (first: the lowest id, it wins where both contain)
    # (a corner one unit below the cube's, legs of 2: short of the cube; legs of 3.45: the slanted face passes through the cube's centre)
    c0 = cv.min(0) - 1.0
    far = c0 + np.vstack([np.zeros(3), (3.45 if first else 2.0) * np.eye(3)])
    v = np.vstack([cv, far])
    big = np.array([[n0, n0 + 1, n0 + 2, n0 + 3]], np.int32)
    t = np.vstack([big, ct]) if first else np.vstack([ct, big])
    wide_id = 0 if first else len(t) - 1
    if renumber == ON:
        v, t = _shuffled(v, t)
    g = FemIntegrator(v, t, _fixed_of(v), renumber=renumber)
    assert g.renumbering()[0] == (renumber == ON)
    rng = np.random.default_rng(5)
    only_big = np.float32(c0 + 0.1 + 0.5 * rng.random((200, 3))).astype(np.float64)
    pts = np.vstack([er.generic_points(cv, 1200, 31), only_big, er.generic_points(np.vstack([cv, far]), 400, 32, grow=0.1)])
    eid, info = g.embed(pts, info=True)
    assert info["n_wide"] >= 1 and np.prod(info["grid"]) > 64
    got = g.embedding(eid)
    ref = _check_generic(v, t, pts, got, info)
    assert (got["elements"][1200:1400] == wide_id).all() and not ref["external"][1200:1400].any()
    if first:
        assert (got["elements"][:1200] == 0).sum() > 50 and (got["elements"][:1200] > 0).sum() > 50
    g.close()


# ---- 3. zero_threshold ----
def test_zero_threshold(gpu, golden):
    v, t = golden["cube_verts"], golden["cube_tets"]
    pts = golden["cube_generic"].astype(np.float64)
    g = FemIntegrator(v, t, _fixed_of(v))
    thr = 0.06
    ref = er.bind(v, t, pts, thr)
    # (the threshold itself must not sit on a rounding: no point's distance within 1e-9 of it)
    d = np.sqrt(((v[ref["vertices"]] - pts[:, None, :]) ** 2).sum(axis=2)).min(axis=1)
    assert np.abs(d - thr).min() > 1e-9 and 100 < ref["n_zeroed"] < len(pts) - 100
    eid, info = g.embed(pts, zero_threshold=thr, info=True)
    _check_generic(v, t, pts, g.embedding(eid), info, ref=ref)
    assert info["n_zeroed"] == ref["n_zeroed"]
    g.close()


# ---- 4. the update ----
def _triangle_grid(lo, hi, k):
    """k x k points on a tilted plane inside the box and the 2 (k - 1)^2 triangles over them"""
    s, u = np.meshgrid(np.linspace(0.08, 0.92, k), np.linspace(0.1, 0.9, k), indexing="ij")
    p = np.stack([s, u, 0.3 + 0.35 * s + 0.1 * u], axis=-1).reshape(-1, 3)
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    return lo + p * (hi - lo), np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)


def _check_update(g, eid, tri, n_tri_points):
    b = g.embedding(eid)
    x0, _ = g.read_mesh()
    q = g.get_q_state()[0]
    want = er.positions(x0, q, b["vertices"], b["weights"])
    xyz, nrm, info = g.embed_update(eid)
    w32 = np.float32(want)
    ulp = np.spacing(np.abs(w32))
    assert xyz.dtype == np.float32 and (np.abs(xyz.astype(np.float64) - w32.astype(np.float64)) <= ulp).all(), "within one float ulp of the fp64 sum"
    print("positions: %d of %d components differ from numpy's rounding" % ((xyz != w32).sum(), xyz.size))
    assert np.array_equal(info["aabb"], np.array([xyz.min(axis=0), xyz.max(axis=0)]))
    ref = er.normals(want, tri) if len(tri) else np.zeros_like(want)
    p = want[tri]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    total = np.zeros_like(want)
    np.add.at(total, tri.ravel(), np.repeat(n / np.linalg.norm(n, axis=1)[:, None], 3, axis=0))
    ok = np.linalg.norm(total, axis=1) >= MIN_SUM
    assert ok[:n_tri_points].all() and not ok[n_tri_points:].any()
    err = np.abs(nrm.astype(np.float64) - ref)[ok].max()
    print("normals: max abs error %.3g" % err)
    assert err <= NORMAL_TOL
    assert not nrm[n_tri_points:].any(), "a point without a triangle has no normal"
    return xyz, nrm


def test_update_follows_the_state(gpu):
    v, t = truth_cube(6, 4, 4, 0.1)
    v, t = np.array(v, np.float64).reshape(-1, 3), np.array(t, np.int32).reshape(-1, 4)
    for renumber in (OFF, ON):
        g = FemIntegrator(v, t, _fixed_of(v), renumber=renumber)
        gp, tri = _triangle_grid(v.min(0), v.max(0), 15)
        pts = np.vstack([gp, er.generic_points(v, 2000, 41, grow=0.1)])
        eid = g.embed(pts, tri)
        a = _check_update(g, eid, tri, len(gp))  # at rest
        assert np.abs(a[0][:len(gp)] - np.float32(gp)).max() <= 2 * np.spacing(np.float32(np.abs(gp).max()))
        for _ in range(3):
            g.set_uniform_force(1, -300.0)
            g.do_timestep()
        assert np.abs(g.get_q_state()[0]).max() > 0
        b = _check_update(g, eid, tri, len(gp))
        assert (b[0] != a[0]).any(), "the points move with the tets"
        c = g.embed_update(eid)
        assert b[0].tobytes() == c[0].tobytes() and b[1].tobytes() == c[1].tobytes(), "two updates without a step: identical bytes"
        # NULL pointers
        x, n_, i1 = g.embed_update(eid, positions=False, normals=False)
        assert x is None and n_ is None and np.array_equal(i1["aabb"], c[2]["aabb"])
        x, n_, _ = g.embed_update(eid, normals=False)
        assert n_ is None and x.tobytes() == c[0].tobytes()
        # an embedding without triangles
        e2 = g.embed(pts[len(gp):])
        x2, n2, _ = g.embed_update(e2)
        assert x2.tobytes() == c[0][len(gp):].tobytes() and not n2.any()
        g.close()


# ---- 6. other mesh changes ----
def test_resync_to_another_mesh_searches_every_point_again(gpu):
    v, t = er.jittered_cube()
    v2, t2, _ = delaunay_jittered(4, cellsize=0.1)  # the same box, another tessellation
    g = FemIntegrator(v, t, _fixed_of(v))
    pts = er.generic_points(v, 1000, 51)
    eid, info = g.embed(pts, info=True)
    before = g.embedding(eid)
    g.resync(v2, t2, _fixed_of(v2))
    after = g.embedding(eid)
    _, _, info2 = g.embed_update(eid)
    assert info2["n_locates"] == info["n_locates"] + 1
    assert info2["n_rebound"] == int((after["elements"] != before["elements"]).sum()) > 0
    assert np.array_equal(after["rest_xyz"], pts)
    twin = FemIntegrator(v2, t2, _fixed_of(v2))
    fresh = twin.embedding(twin.embed(after["rest_xyz"]))
    for key in ("elements", "vertices", "weights", "rest_xyz"):
        assert after[key].tobytes() == fresh[key].tobytes(), key
    _check_generic(v2, t2, pts, after, info2)
    a, b = g.embed_update(eid), twin.embed_update(0)
    assert a[0].tobytes() == b[0].tobytes()
    # a second read searches nothing
    g.embedding(eid)
    assert g.embed_update(eid)[2]["n_locates"] == info2["n_locates"]
    g.close(); twin.close()


# ---- 8. errors and lifetime ----
def test_errors_and_slots(gpu):
    v, t = er.jittered_cube()
    g = FemIntegrator(v, t, _fixed_of(v))
    L, pts = g._L, er.generic_points(v, 10, 61)
    tri = np.array([[0, 1, 2]], np.int32)

    def refused(call):
        with pytest.raises(fl.FbError) as e:
            call()
        return e.value.code == fl.FB_EINVAL

    assert refused(lambda: g.embed(np.zeros((0, 3))))
    for bad in (np.nan, np.inf, -np.inf):
        p = pts.copy()
        p[7, 1] = bad
        assert refused(lambda: g.embed(p))
    assert refused(lambda: g.embed(pts, np.array([[0, 1, 10]], np.int32)))
    assert refused(lambda: g.embed(pts, np.array([[0, -1, 2]], np.int32)))
    for bad_id in (-1, 0, 8, 100):  # (nothing is embedded yet)
        assert refused(lambda: g.embedding(bad_id)) and refused(lambda: g.embed_update(bad_id)) and refused(lambda: g.embed_release(bad_id))
        assert refused(lambda: g.time_embed(bad_id, 1))
    ids = [g.embed(pts, tri) for _ in range(8)]
    assert ids == list(range(8))
    assert refused(lambda: g.embed(pts))  # a ninth
    g.embed_release(3)
    assert refused(lambda: g.embedding(3))
    assert g.embed(pts[:5]) == 3 and g.embedding(3)["elements"].shape == (5,)
    assert np.array_equal(g.embedding(5)["elements"], g.embedding(0)["elements"])
    b0 = g.embedding(0)
    lo, up = g.time_embed(0, reps=2)
    phases = g.time_embed_search(0, reps=2)
    assert lo > 0 and up > 0 and len(phases) == 3 and min(phases) > 0 and g.embed_update(0)[2]["n_locates"] == 1
    for key, a in g.embedding(0).items():
        assert a.tobytes() == b0[key].tobytes(), "timing searches a scratch copy: the binding stands"
    g.close()


def test_a_handle_that_never_embeds_steps_the_same(gpu):
    v, t = truth_cube(6, 4, 4, 0.1)
    v, t = np.array(v, np.float64).reshape(-1, 3), np.array(t, np.int32).reshape(-1, 4)
    a, b = FemIntegrator(v, t, _fixed_of(v)), FemIntegrator(v, t, _fixed_of(v))
    eid = b.embed(er.generic_points(v, 300, 71))
    for _ in range(3):
        for g in (a, b):
            g.set_uniform_force(1, -300.0)
            g.do_timestep()
        b.embed_update(eid)
    for x, y in zip(a.get_q_state(), b.get_q_state()):
        assert x.tobytes() == y.tobytes()
    a.close(); b.close()


def test_deformable_forwards(gpu):
    v, t = truth_cube(5, 5, 5, 0.1)
    v, t = np.array(v, np.float64).reshape(-1, 3), np.array(t, np.int32).reshape(-1, 4)
    d = Deformable(v, t, np.nonzero(v[:, 0] == v[:, 0].min())[0])
    pts, tri = _triangle_grid(v.min(0), v.max(0), 6)
    eid = d.embed(pts, tri)
    d.timestep()
    xyz, nrm, info = d.embedded_mesh(eid)
    assert xyz.shape == nrm.shape == (36, 3) and info["n_triangles"] == 50 and info["n_external"] == 0


# ---- 5. cuts ----
import cutref as cr  # noqa: E402


def _cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    return np.array(v, np.float64).reshape(-1, 3), np.array(t, np.int32).reshape(-1, 4)


def _cut_case(mesh, blade):
    if mesh == "cube":
        v, t = _cube(6)
        fixed = _fixed_of(v)
        strip = cr.plane_strip(0.5 * (v.min(0) + v.max(0)) + [0.0013, 0.0007, 0.0003], (1.0, 0.013, 0.007)) if blade == "plane" else None
        if strip is None:  # the folded blade of the Delaunay cases, scaled into the cube
            strip = 0.5 * (v.min(0) + v.max(0)) + 0.14 * ci.folded_strip(4, 0.15, 45)
    else:
        v, t, fixed = ci.delaunay(400, 7)
        strip = cr.plane_strip((0.013, 0.007, 0.003), (1.0, 0.013, 0.007)) if blade == "plane" else ci.folded_strip(4, 0.15, 45)
    return v, t, fixed, strip


def _follow_and_check(g, eid, strip, mode):
    """one cut of g with embedding eid live: the binding after it equal to embedref.follow_cut fed from the cut's read-back"""
    x_old, t_old = g.read_mesh()
    before = g.embedding(eid)
    i0 = g.embed_update(eid)[2]
    info, delta = g.cut(strip, mode=mode)
    if info["status"] != fl.FB_CUT_DONE:
        return info, before, before
    x_new, t_new = g.read_mesh()
    after = g.embedding(eid)
    i1 = g.embed_update(eid)[2]
    ref = er.follow_cut(t_old, before, delta, x_new, t_new, mode == "bake")
    rb = ref["rebound"]
    assert rb.sum() > 0 and ref["margin"][rb].min() >= MARGIN, "every re-bound point is generic, by choice of seed"
    assert np.array_equal(after["elements"], ref["elements"]) and np.array_equal(after["vertices"], ref["vertices"])
    assert after["weights"][~rb].tobytes() == before["weights"][~rb].tobytes(), "kept points: the same bits"
    assert (np.abs(after["weights"][rb] - ref["weights"][rb]).max(axis=1) <= ref["bound"][rb]).all()
    scale = np.abs(x_new).max()
    assert np.abs(after["rest_xyz"] - ref["rest_xyz"]).max() <= 8 * er.U * scale
    if mode == "carry":
        assert after["rest_xyz"][~rb].tobytes() == before["rest_xyz"][~rb].tobytes()
    assert i1["n_rebound"] == i0["n_rebound"] + int(rb.sum()) and i1["n_locates"] == i0["n_locates"]
    return info, before, after


@pytest.mark.parametrize("blade", ["plane", "folded"])
@pytest.mark.parametrize("mode", ["bake", "carry"])
@pytest.mark.parametrize("mesh", ["cube", "delaunay"])
def test_binding_follows_a_cut(gpu, mesh, mode, blade):
    v, t, fixed, strip = _cut_case(mesh, blade)
    for renumber in (OFF, ON):
        g = FemIntegrator(v, t, fixed, renumber=renumber, expect_cuts=True, cg_max_iter=50000)
        g.set_q_state(ci.smooth_displacement(v).reshape(-1), np.zeros(v.size))
        eid = g.embed(er.generic_points(v, 1200, 91, grow=0.05))
        info, _, after = _follow_and_check(g, eid, strip, mode)
        assert info["status"] == fl.FB_CUT_DONE, info
        # the update gathers through the new internal ids
        x0, _ = g.read_mesh()
        want = np.float32(er.positions(x0, g.get_q_state()[0], after["vertices"], after["weights"]))
        xyz = g.embed_update(eid)[0]
        assert (np.abs(xyz.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
        g.close()


def test_two_cuts_in_a_row_and_a_cut_that_changes_nothing(gpu):
    v, t = _cube(6)
    g = FemIntegrator(v, t, _fixed_of(v), expect_cuts=True)
    eid = g.embed(er.generic_points(v, 1200, 92, grow=0.05))
    c = 0.5 * (v.min(0) + v.max(0))
    b0 = g.embedding(eid)
    info, _ = g.cut(cr.plane_strip(c + [5.0, 0, 0], (1.0, 0.0, 0.0), half=0.1))
    assert info["status"] == fl.FB_CUT_NOTHING
    info, _ = g.cut(cr.plane_strip(c + [0.0013, 0.0007, 0.0003], (1.0, 0.013, 0.007)), modify=False)
    assert info["status"] == fl.FB_CUT_DRY
    b1 = g.embedding(eid)
    for key in b0:
        assert b0[key].tobytes() == b1[key].tobytes(), key
    # two cuts with no update between them (the reads inside _follow_and_check search nothing: a cut leaves no orphan)
    x_old, t_old = g.read_mesh()
    lo, ext = v.min(0), v.max(0) - v.min(0)
    i1, d1 = g.cut(cr.plane_strip(lo + ext * [0.32, 0.5, 0.5] + [0.0013, 0.0007, 0.0003], (1.0, 0.021, 0.013)), mode="carry")
    x_mid, t_mid = g.read_mesh()
    i2, d2 = g.cut(cr.plane_strip(lo + ext * [0.66, 0.5, 0.5] + [0.0013, 0.0007, 0.0003], (1.0, 0.042, 0.013)), mode="carry")
    assert i1["status"] == i2["status"] == fl.FB_CUT_DONE
    x_new, t_new = g.read_mesh()
    r1 = er.follow_cut(t_old, b0, d1, x_mid, t_mid, False)
    r2 = er.follow_cut(t_mid, r1, d2, x_new, t_new, False)
    after = g.embedding(eid)
    assert min(r1["margin"].min(), r2["margin"].min()) >= MARGIN
    assert np.array_equal(after["elements"], r2["elements"]) and np.array_equal(after["vertices"], r2["vertices"])
    moved = r1["rebound"] | r2["rebound"]
    assert after["weights"][~moved].tobytes() == b0["weights"][~moved].tobytes()
    # (a point re-bound twice carries the first cut's rounding into the second location: both bounds add)
    assert (np.abs(after["weights"] - r2["weights"]).max(axis=1) <= r1["bound"] + r2["bound"] + 4 * er.U).all()
    assert g.embed_update(eid)[2]["n_rebound"] == int(r1["rebound"].sum() + r2["rebound"].sum())
    g.close()


def test_after_a_cut_and_split_every_point_is_on_its_side(gpu):
    v, t = _cube(6)
    g = FemIntegrator(v, t, _fixed_of(v), expect_cuts=True)
    pts = er.generic_points(v, 1500, 93, grow=0.0)
    eid = g.embed(pts)
    c, nrm = 0.5 * (v.min(0) + v.max(0)) + [0.0013, 0.0007, 0.0003], np.array([1.0, 0.013, 0.007])
    strip = cr.plane_strip(c, nrm)
    info, _ = g.cut(strip, mode="carry")
    assert info["status"] == fl.FB_CUT_DONE and g.parts()["n_parts"] == 2
    b = g.embedding(eid)
    side = (pts - c) @ nrm > 0
    g.split_parts(strip[:4], 0.01)
    labels = g.node_parts()
    b2 = g.embedding(eid)
    for key in ("elements", "vertices", "weights"):
        assert b[key].tobytes() == b2[key].tobytes()
    lab = labels[b2["vertices"]]
    assert (lab == lab[:, :1]).all(), "the four nodes of a point's element carry one label"
    assert len(set(zip(lab[:, 0].tolist(), side.tolist()))) == 2, "... and that label is the side of the blade the point is on"
    xyz = g.embed_update(eid)[0]
    assert np.abs(np.abs((xyz - np.float32(pts)) @ (nrm / np.linalg.norm(nrm))) - 0.01).max() < 1e-5, "the points went apart with their parts"
    g.close()


# ---- 6. other changes in place ----
def test_delta_and_detach_leave_orphans_that_are_searched_once(gpu):
    from fembrain_amd.meshgen import synthetic_cut
    v, t = _cube(6)
    fixed = _fixed_of(v)
    for renumber in (OFF, ON):
        g = FemIntegrator(v, t, fixed, renumber=renumber, expect_cuts=True)
        # (points inside the body: a point outside keeps the element it has, where a new search could prefer the centre of an added one)
        pts = er.generic_points(v, 1200, 94, grow=0.0)
        eid, info = g.embed(pts, info=True)
        before = g.embedding(eid)
        v2, t2, delta = synthetic_cut(v, t)
        g.resync_delta(delta, fixed)
        after = g.embedding(eid)
        i2 = g.embed_update(eid)[2]
        assert i2["n_locates"] == info["n_locates"] + 1
        g.embedding(eid)
        assert g.embed_update(eid)[2]["n_locates"] == i2["n_locates"], "searched once"
        twin = FemIntegrator(v2, t2, fixed)
        fresh = twin.embedding(twin.embed(after["rest_xyz"]))
        for key in ("elements", "vertices", "weights", "rest_xyz"):
            assert after[key].tobytes() == fresh[key].tobytes(), (renumber, key)
        gone = np.isin(before["elements"], np.concatenate([delta["removed"], delta["changed_ids"]]))
        assert gone.any() and after["weights"][~gone].tobytes() == before["weights"][~gone].tobytes()
        twin.close()
        g.close()
    # a part taken out of the parent
    g = FemIntegrator(v, t, fixed, expect_cuts=True)
    eid, info = g.embed(pts, info=True)
    c = 0.5 * (v.min(0) + v.max(0)) + [0.0013, 0.0007, 0.0003]
    assert g.cut(cr.plane_strip(c, (1.0, 0.013, 0.007)), mode="carry")[0]["status"] == fl.FB_CUT_DONE
    piece, _, _ = g.detach_part(1, remove=True)
    after = g.embedding(eid)
    i2 = g.embed_update(eid)[2]
    assert i2["n_locates"] == info["n_locates"] + 1
    x2, t2 = g.read_mesh()
    twin = FemIntegrator(x2, t2, fixed)
    fresh = twin.embedding(twin.embed(after["rest_xyz"]))
    for key in ("elements", "vertices", "weights", "rest_xyz"):
        assert after[key].tobytes() == fresh[key].tobytes(), key
    with pytest.raises(fl.FbError):
        piece.embedding(eid)  # embeddings stay with the parent
    piece.close(); twin.close(); g.close()


# ---- 7. the polygonizer's surface, handed over on the device ----
def test_embed_from_poly_equals_embed_of_the_read_back_surface(gpu):
    from fembrain_amd.blobtree import sphere_blob
    from fembrain_amd.poly import GpuPoly
    coarse, fine = GpuPoly(sphere_blob()), GpuPoly(sphere_blob())
    xyz, tets = coarse.run_tetrahedralizer(0.14)
    sx, _, st = fine.run(0.07)          # a grid twice as fine: about 20^3 points
    assert len(sx) > 500 and len(st) > 1000
    fixed = fixed_vertices_to_dofs(np.nonzero(xyz[:, 1] < xyz[:, 1].min() + 0.2)[0].astype(np.int32))
    g = FemIntegrator.from_poly(coarse, fixed)
    a, ia = g.embed_from_poly(fine, info=True)
    b, ib = g.embed(sx.astype(np.float64), st.astype(np.int32), info=True)
    ba, bb = g.embedding(a), g.embedding(b)
    for key in ("elements", "vertices", "weights", "rest_xyz"):
        assert ba[key].tobytes() == bb[key].tobytes(), key
    ref = er.bind(g.verts, g.tets, sx.astype(np.float64))
    # (whatever the restatement says: the coarse tets cover the cells the surface crosses, but a vertex may sit on the hull of the tets up to rounding)
    assert ia["n_external"] == ib["n_external"] == ref["n_external"]
    assert ia["n_points"] == len(sx) and ia["n_triangles"] == len(st)
    for _ in range(2):
        g.set_uniform_force(1, -300.0)
        g.do_timestep()
    ua, ub = g.embed_update(a), g.embed_update(b)
    assert ua[0].tobytes() == ub[0].tobytes() and ua[1].tobytes() == ub[1].tobytes() and np.array_equal(ua[2]["aabb"], ub[2]["aabb"])
    assert np.abs(np.linalg.norm(ua[1], axis=1) - 1.0).max() < 1e-5, "every vertex of the surface has a normal"
    # a polygonizer without a surface is refused
    with pytest.raises(fl.FbError) as e:
        g.embed_from_poly(coarse)
    assert e.value.code == fl.FB_EINVAL
    g.close(); coarse.close(); fine.close()


# ---- a sharded handle (child processes, as tests/test_fem_surface_gpu.py runs its own) ----
def _shard_child(rank, world, shm_name, q):
    import ctypes as C
    try:
        from test_sharded_gpu import _mesh
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed, splits = _mesh(6, world)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
        codes = []
        for call in (lambda: g.embed(np.asarray(v, np.float64).reshape(-1, 3)[:5]), lambda: g.embedding(0), lambda: g.embed_update(0)):
            try:
                call()
                codes.append(fl.FB_OK)
            except fl.FbError as e:
                codes.append(e.code)
        g.close()
        L.fb_comm_destroy(comm)
        q.put((rank, codes))
    except Exception as e:
        q.put((rank, repr(e)))
        q.close()
        q.join_thread()
        os._exit(1)


def test_sharded_handle_is_refused(gpu):
    from test_fem_surface_gpu import _run_children
    name = "fbembed%d" % os.getpid()
    got = _run_children(_shard_child, [(r, 2, name) for r in range(2)])
    assert sorted(got) == [(0, [fl.FB_EINVAL] * 3), (1, [fl.FB_EINVAL] * 3)], got
