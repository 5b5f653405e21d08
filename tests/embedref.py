"""The binding rule of fb_fem_embed (include/fembrain_hip.h, "Embedded point sets") restated in numpy, by brute force: every point
against every element, fp64, in the operation order of the header's rule -- the weights w_i = D_i / D_0 from 4 x 4 determinants expanded
into four 3 x 3 ones, the lowest-numbered element with four weights >= 0, else the element with the closest centre (strict <,
ascending).  Elementwise numpy arithmetic does not fuse multiply and add, so the same expression gives the same bits as a C evaluation
without contraction.

Also here: what the tests need to tell a GENERIC point (decided far from any rounding) from a degenerate one, and how far two correct
evaluations of a weight may differ."""
import numpy as np

U = 2.0 ** -52


def _det3_terms(a, b, c):
    """the six signed products of the 3 x 3 determinant with rows a, b, c (broadcast over leading axes), in summation order"""
    return (-a[..., 2] * b[..., 1] * c[..., 0], a[..., 1] * b[..., 2] * c[..., 0], a[..., 2] * b[..., 0] * c[..., 1],
            -a[..., 0] * b[..., 2] * c[..., 1], -a[..., 1] * b[..., 0] * c[..., 2], a[..., 0] * b[..., 1] * c[..., 2])


def _det3(a, b, c):
    t = _det3_terms(a, b, c)
    return ((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5]


def tet_det(a, b, c, d):
    """determinant of [a 1; b 1; c 1; d 1]: -det(b, c, d) + det(a, c, d) - det(a, b, d) + det(a, b, c), left to right"""
    return ((-_det3(b, c, d) + _det3(a, c, d)) - _det3(a, b, d)) + _det3(a, b, c)


def tet_det_abs(a, b, c, d):
    """the sum of the absolute values of the 24 products tet_det adds up"""
    s = 0.0
    for rows in ((b, c, d), (a, c, d), (a, b, d), (a, b, c)):
        for t in _det3_terms(*rows):
            s = s + np.abs(t)
    return s


def weights_in(verts, tets, points, elements):
    """(n, 4) weights of point k in element elements[k], and the (n,) forward error bound of weight_bound"""
    v = np.asarray(verts, np.float64)[np.asarray(tets)[elements]]  # (n, 4, 3)
    p = np.asarray(points, np.float64)
    a, b, c, d = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        d0 = tet_det(a, b, c, d)
        di = np.stack([tet_det(p, b, c, d), tet_det(a, p, c, d), tet_det(a, b, p, d), tet_det(a, b, c, p)], axis=1)
        w = di / d0[:, None]
        s0 = tet_det_abs(a, b, c, d)
        si = np.stack([tet_det_abs(p, b, c, d), tet_det_abs(a, p, c, d), tet_det_abs(a, b, p, d), tet_det_abs(a, b, c, p)], axis=1)
        # w = D_i / D_0 with each determinant off by at most 16 u times the sum of the absolute values of its products (24 products of
        # two roundings each and 23 additions: the longest chain through one product is 2 + 7 roundings, 16 rounds that up and covers a
        # fused evaluation, which only drops roundings) and one more rounding for the division:
        # |dw| <= 16 u (S_i + |w| S_0) / |D_0|, the largest of the four taken for the point
        bound = 16.0 * U * (si + np.abs(w) * s0[:, None]) / np.abs(d0)[:, None]
    return w, bound.max(axis=1)


def all_weights(verts, tets, points, chunk=256):
    """(n_points, n_tets, 4): every point in every element"""
    verts, tets, points = np.asarray(verts, np.float64), np.asarray(tets), np.asarray(points, np.float64)
    n, m = len(points), len(tets)
    out = np.empty((n, m, 4))
    ids = np.arange(m)
    for s in range(0, n, chunk):
        k = min(chunk, n - s)
        w, _ = weights_in(verts, tets, np.repeat(points[s:s + k], m, axis=0), np.tile(ids, k))
        out[s:s + k] = w.reshape(k, m, 4)
    return out


def centres(verts, tets):
    v = np.asarray(verts, np.float64)[np.asarray(tets)]
    return (((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]) * (1.0 / 4)


def centre_distances(verts, tets, points):
    d = np.asarray(points, np.float64)[:, None, :] - centres(verts, tets)[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def bind(verts, tets, points, zero_threshold=0.0, tol=0.0, W=None):
    """The rule by brute force.  dict of elements (n,), vertices (n, 4), weights (n, 4), external (n,) bool, zeroed (n,) bool,
    n_external, n_zeroed, bound (n,) (weight_bound of the chosen element) and containing: per point the ids of the elements whose four
    weights are all >= -tol (what a degenerate point may legitimately bind to).  W: all_weights of the same arguments, where the caller has them."""
    verts, tets, points = np.asarray(verts, np.float64), np.asarray(tets), np.asarray(points, np.float64)
    W = all_weights(verts, tets, points) if W is None else W
    with np.errstate(invalid="ignore"):
        inside = (W >= 0).all(axis=2)  # (a flat element: NaN or infinite weights compare false)
        near = (W >= -tol).all(axis=2)
    has = inside.any(axis=1)
    first = inside.argmax(axis=1)
    closest = centre_distances(verts, tets, points).argmin(axis=1)  # (argmin: the first of equal minima, as strict < in ascending order)
    elements = np.where(has, first, closest).astype(np.int32)
    w, bound = weights_in(verts, tets, points, elements)
    vertices = tets[elements].astype(np.int32)
    zeroed = np.zeros(len(points), bool)
    if zero_threshold > 0:
        d = verts[vertices] - points[:, None, :]
        dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1)
        zeroed = dist > zero_threshold
        w = np.where(zeroed[:, None], 0.0, w)
    return dict(elements=elements, vertices=vertices, weights=w, external=~has, zeroed=zeroed, n_external=int((~has).sum()),
                n_zeroed=int(zeroed.sum()), bound=bound, containing=[np.nonzero(r)[0] for r in near])


def margin(verts, tets, points, W=None):
    """(n,) how far each point's binding is from depending on rounding: the smallest |w| of the point over ALL elements (a sign that
    could flip changes which elements contain it), and for a point no element contains also the relative gap between its two closest
    centres, (d2 - d1) / d2 -- the smaller of the two."""
    verts, tets, points = np.asarray(verts, np.float64), np.asarray(tets), np.asarray(points, np.float64)
    W = all_weights(verts, tets, points) if W is None else W
    with np.errstate(invalid="ignore"):
        m = np.nanmin(np.abs(W).reshape(len(points), -1), axis=1)
        external = ~(W >= 0).all(axis=2).any(axis=1)
    if external.any() and len(tets) > 1:
        d = np.sort(centre_distances(verts, tets, points[external]), axis=1)
        m[external] = np.minimum(m[external], (d[:, 1] - d[:, 0]) / d[:, 1])
    return m


def weight_bound(verts, tets, points, elements):
    """(n,) forward error bound of the weights of point k in elements[k]: 16 * 2^-52 * (S_i + |w_i| S_0) / |D_0|, S the sum of the
    absolute values of the products a determinant adds up; the largest of the point's four.  It covers fused multiply-adds."""
    return weights_in(verts, tets, points, elements)[1]


def positions(verts, q, vertices, weights):
    """fp64 ((w0 p0 + w1 p1) + w2 p2) + w3 p3 with p = x0 + q: what fb_fem_embed_update rounds to float"""
    p = (np.asarray(verts, np.float64).reshape(-1, 3) + np.asarray(q, np.float64).reshape(-1, 3))[vertices]  # (n, 4, 3)
    w = np.asarray(weights, np.float64)[:, :, None]
    return ((w[:, 0] * p[:, 0] + w[:, 1] * p[:, 1]) + w[:, 2] * p[:, 2]) + w[:, 3] * p[:, 3]


def normals(xyz64, triangles):
    """per point the normalised fp64 sum, in ascending triangle order, of the unit normals of its triangles; zero where there is none"""
    xyz64, triangles = np.asarray(xyz64, np.float64), np.asarray(triangles).reshape(-1, 3)
    p = xyz64[triangles]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.sqrt((n * n).sum(axis=1))
    ok = ln > 0
    n[ok] /= ln[ok][:, None]
    n[~ok] = 0.0
    out = np.zeros_like(xyz64)
    for t in range(len(triangles)):  # ascending: the order of every point's additions
        for c in range(3):
            out[triangles[t, c]] += n[t]
    ln = np.sqrt((out * out).sum(axis=1))
    ok = ln > 0
    out[ok] /= ln[ok][:, None]
    out[~ok] = 0.0
    return out


# ---- inputs the tests share ----

def jittered_cube(n=4, jitter=0.2, seed=7):
    """an n^3-node cube of 6 (n - 1)^3 tets with its inner nodes moved by up to ``jitter`` of a cell; (verts, tets)"""
    from fembrain_amd.meshgen import truth_cube
    v, t = truth_cube(n, n, n, 0.1)
    v = np.array(v, np.float64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(axis=0), v.max(axis=0)
    inner = ((v > lo + 1e-9) & (v < hi - 1e-9)).all(axis=1)
    v[inner] += (rng.random((int(inner.sum()), 3)) - 0.5) * 2 * jitter * 0.1
    return v, np.array(t, np.int32).reshape(-1, 4)


def generic_points(verts, n, seed, grow=0.2):
    """n seeded points in the box of the mesh grown by ``grow`` of its extent (half on every side), each coordinate a float32 value (held
    as float64): a fixture stores them in half the bytes, exactly"""
    verts = np.asarray(verts, np.float64)
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    ext = hi - lo
    rng = np.random.default_rng(seed)
    return np.float32(lo - 0.5 * grow * ext + rng.random((n, 3)) * (1 + grow) * ext).astype(np.float64)


def degenerate_points(verts, tets, n_nodes=10):
    """nodes, and the centroid of the first element's face (0, 1, 2): points that lie in several elements up to rounding"""
    verts, tets = np.asarray(verts, np.float64), np.asarray(tets)
    ids = np.linspace(0, len(verts) - 1, n_nodes).astype(int)
    f = verts[tets[0, :3]]
    return np.vstack([verts[ids], ((f[0] + f[1]) + f[2])[None, :] / 3.0])


# ---- a binding carried across a cut (fb_fem_cut with a live embedding) ----

_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def cut_pieces(tets_old, delta):
    """per removed parent (ascending, delta['removed']) the first of its pieces in delta['added'] and their number: 4 where three of its
    edges were cut, 6 where four were -- the pieces are appended by ascending parent"""
    t = np.asarray(tets_old, np.int64)
    en = np.asarray(delta["edge_nodes"], np.int64).reshape(-1, 2)
    cut = set((int(a), int(b)) for a, b in en)
    cnt = []
    for e in np.asarray(delta["removed"], np.int64):
        k = sum((min(int(t[e, a]), int(t[e, b])), max(int(t[e, a]), int(t[e, b]))) in cut for a, b in _EDGES)
        assert k in (3, 4), (e, k)
        cnt.append(4 if k == 3 else 6)
    cnt = np.array(cnt, np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64) if len(cnt) else np.zeros(0, np.int64)
    assert int(cnt.sum()) == len(np.asarray(delta["added"]).reshape(-1, 4))
    return off, cnt


def follow_cut(tets_old, binding, delta, x_new, tets_new, bake, zeroed=None):
    """The rule of the header for a cut: a point in a kept element gets the element's new id (the kept elements before it) and keeps
    weights and vertices; a point in a subdivided element is located at sum w_i x_i over the parent's nodes in the rest shape AFTER the cut
    (x_new) and bound to the lowest-numbered piece that contains that location, else the piece with the closest centre, with that piece's
    weights.  bake: the rest shape moved, so rest_xyz of every point is sum w_i x_i in it.
    binding: dict of elements, vertices, weights, rest_xyz before the cut.  Returns the same after it, plus rebound (n,) bool, bound (n,)
    (weight_bound, re-bound points) and margin (n,) (the smallest |w| of a re-bound point over the pieces of its parent; inf elsewhere)."""
    tets_old, tets_new, x_new = np.asarray(tets_old), np.asarray(tets_new), np.asarray(x_new, np.float64)
    el, vt, w = binding["elements"].copy(), binding["vertices"].copy(), binding["weights"].copy()
    loc = binding["rest_xyz"].copy()
    n = len(el)
    zeroed = np.zeros(n, bool) if zeroed is None else zeroed
    removed = np.asarray(delta["removed"], np.int64)
    stays = np.ones(len(tets_old), np.int64)
    stays[removed] = 0
    pos = np.cumsum(stays) - stays
    n_kept = int(stays.sum())
    assert np.array_equal(tets_new[:n_kept], tets_old[stays == 1])
    off, cnt = cut_pieces(tets_old, delta)
    parent_index = {int(e): j for j, e in enumerate(removed)}
    where = positions(x_new, np.zeros(x_new.size), vt, w)  # every point in the new rest shape, through its OLD binding
    rebound = np.array([int(e) in parent_index for e in el])
    if bake:
        loc[~zeroed] = where[~zeroed]
    else:
        loc[rebound & ~zeroed] = where[rebound & ~zeroed]
    bound, marg = np.zeros(n), np.full(n, np.inf)
    for k in np.nonzero(rebound)[0]:
        j = parent_index[int(el[k])]
        ids = n_kept + off[j] + np.arange(cnt[j])
        p = np.repeat(loc[k][None, :], len(ids), axis=0)
        wk, bk = weights_in(x_new, tets_new, p, ids)
        inside = (wk >= 0).all(axis=1)
        marg[k] = np.abs(wk).min()
        if inside.any():
            m = int(inside.argmax())
        else:
            m = int(centre_distances(x_new, tets_new[ids], loc[k][None, :])[0].argmin())
        el[k], vt[k], w[k], bound[k] = ids[m], tets_new[ids[m]], (0.0 if zeroed[k] else wk[m]), bk[m]
    el[~rebound] = pos[el[~rebound]]
    return dict(elements=el.astype(np.int32), vertices=vt.astype(np.int32), weights=w, rest_xyz=loc, rebound=rebound, bound=bound, margin=marg)
