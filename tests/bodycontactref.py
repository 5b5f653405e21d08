"""The rule of fb_fem_body_contact (include/fembrain_hip.h, "Contact between two bodies") restated in numpy, by brute force: every surface
vertex of one body against every element and every boundary face of the other, in the operation order of the device functions
(body_contact.hip closest_on_triangle, embed_grid.hip.h bary and centre_distance), the same tie rules, the same summation order.
Elementwise numpy arithmetic does not fuse multiply and add, so in float64 the same expression gives the same bits as the kernels, which
are built without contraction.  ``dtype=np.longdouble`` evaluates the same sequence in the wider format: the spread between the two is what
a last-place difference of a division or a root could cost (``spread``).

Also here: the two margins that tell a contact decided far from any rounding from a degenerate one."""
import numpy as np

import embedref
import surfref

A_INTO_B, B_INTO_A = 1, 2


def dot3(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def closest_on_triangle(p, a, b, c):
    """(closest point (..., 3), v (...), w (...)): Ericson 5.1.5, regions in the book's order -- vertex A, vertex B, edge AB, vertex C, edge
    AC, edge BC, interior.  Every region's expression is evaluated for every entry and the first region that applies is taken."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot3(ab, ap), dot3(ac, ap)
    bp = p - b
    d3, d4 = dot3(ab, bp), dot3(ac, bp)
    cp = p - c
    d5, d6 = dot3(ab, cp), dot3(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / ((va + vb) + vc)
        v_in, w_in = vb * denom, vc * denom
        q, v, w = (a + ab * v_in[..., None]) + ac * w_in[..., None], v_in, w_in
        regions = [
            ((d1 <= 0) & (d2 <= 0), np.broadcast_to(a, q.shape), zero, zero),
            ((d3 >= 0) & (d4 <= d3), np.broadcast_to(b, q.shape), one, zero),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + v_ab[..., None] * ab, v_ab, zero),
            ((d6 >= 0) & (d5 <= d6), np.broadcast_to(c, q.shape), zero, one),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + w_ac[..., None] * ac, zero, w_ac),
            ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + w_bc[..., None] * (c - b), 1.0 - w_bc, w_bc),
        ]
    for cond, rq, rv, rw in reversed(regions):
        q = np.where(cond[..., None], rq, q)
        v = np.where(cond, rv, v)
        w = np.where(cond, rw, w)
    return q, v, w


def distance(p, q):
    d = p - q
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def all_weights(x, tets, points, dtype=np.float64, chunk=128):
    """(n_points, n_tets, 4) weights D_i / D_0 of every point in every element at the positions x"""
    x, points = np.asarray(x, dtype), np.asarray(points, dtype)
    v = x[np.asarray(tets, np.int64)]
    a, b, c, d = v[None, :, 0], v[None, :, 1], v[None, :, 2], v[None, :, 3]
    out = np.empty((len(points), len(tets), 4), dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        d0 = embedref.tet_det(a, b, c, d)
        for s in range(0, len(points), chunk):
            p = points[s:s + chunk, None, :]
            di = np.stack([embedref.tet_det(p, b, c, d), embedref.tet_det(a, p, c, d), embedref.tet_det(a, b, p, d), embedref.tet_det(a, b, c, p)], axis=2)
            out[s:s + chunk] = di / d0[..., None]
    return out


def direction(xp, vids_p, xt, tets_t, faces_t, stiffness, depth_cap=0.0, dtype=np.float64):
    """One direction of the rule: the surface vertices ``vids_p`` (ascending) of the body at positions xp against the body at xt with
    elements tets_t and boundary faces faces_t.  Returns a dict: candidates (vertex ids), in_contact (bool per candidate), and per
    contact, ascending vertex, node / element / face / closest / bary / depth (= d before the cap) / force (on the vertex's node; zero for
    a degenerate contact) / degenerate; per CANDIDATE contain_margin, per contact gap (see ``generic``)."""
    xp, xt = np.asarray(xp, dtype).reshape(-1, 3), np.asarray(xt, dtype).reshape(-1, 3)
    vids_p, tets_t, faces_t = np.asarray(vids_p, np.int64), np.asarray(tets_t, np.int64).reshape(-1, 4), np.asarray(faces_t, np.int64).reshape(-1, 3)
    empty = dict(candidates=np.zeros(0, np.int64), in_contact=np.zeros(0, bool), contain_margin=np.zeros(0), node=np.zeros(0, np.int64), element=np.zeros(0, np.int64),
                 face=np.zeros(0, np.int64), closest=np.zeros((0, 3), dtype), bary=np.zeros((0, 3), dtype), depth=np.zeros(0, dtype), force=np.zeros((0, 3), dtype),
                 degenerate=np.zeros(0, bool), gap=np.zeros(0), boxes_meet=False)
    if not len(vids_p) or not len(tets_t) or not len(faces_t):
        return empty
    pts = xp[vids_p]
    lo, hi = xt.min(axis=0), xt.max(axis=0)
    slo, shi = pts.min(axis=0), pts.max(axis=0)
    if not (np.maximum(lo, slo) <= np.minimum(hi, shi)).all():
        return empty
    cand = ((pts >= lo) & (pts <= hi)).all(axis=1)
    cids, cp = vids_p[cand], pts[cand]
    W = all_weights(xt, tets_t, cp, dtype)
    with np.errstate(invalid="ignore"):
        inside = (W >= 0).all(axis=2)
        smallest = np.where(np.isfinite(W).all(axis=2), W.min(axis=2), -np.inf)
    contain_margin = np.abs(smallest.max(axis=1)).astype(np.float64) if len(cids) else np.zeros(0)
    has = inside.any(axis=1)
    elem = inside.argmax(axis=1)[has]
    node, p = cids[has], cp[has]
    tri = xt[faces_t]  # (F, 3, 3)
    q, v, w = closest_on_triangle(p[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
    d = distance(p[:, None, :], q)
    with np.errstate(invalid="ignore"):
        d = np.where(d < np.finfo(np.float64).max, d, np.inf)  # (a distance that is not a number never wins)
    face = d.argmin(axis=1) if len(node) else np.zeros(0, np.int64)  # (argmin: the first of equal minima, the lowest face)
    k = np.arange(len(node))
    c, bv, bw, dist = q[k, face], v[k, face], w[k, face], d[k, face]
    bary = np.stack([(1.0 - bv) - bw, bv, bw], axis=1) if len(node) else np.zeros((0, 3), dtype)
    degenerate = ~(dist > 0)
    depth = np.minimum(dist, dtype(depth_cap)) if depth_cap > 0 else dist
    with np.errstate(divide="ignore", invalid="ignore"):
        force = (dtype(stiffness) * depth)[:, None] * ((c - p) / dist[:, None])
    force = np.where(degenerate[:, None], dtype(0), force)
    # the gap between the winning distance and the best distance to a DIFFERENT closest point (further than 1e-9 away)
    other = distance(q, c[:, None, :]) > 1e-9
    gap = (np.where(other, d, np.inf).min(axis=1) - dist).astype(np.float64) if len(node) else np.zeros(0)
    return dict(candidates=cids, in_contact=has, contain_margin=contain_margin, node=node, element=elem, face=face, closest=c, bary=bary, depth=dist, force=force,
                degenerate=degenerate, gap=gap, boxes_meet=True)


def surface_of(rest, tets):
    """(faces (F, 3), vertex_ids): the boundary as fb_fem_surface builds it, from the REST positions (they decide the winding)"""
    faces, _ = surfref.vectorised(rest, tets)
    return faces, surfref.vertex_ids(faces)


def body_contact(rest_a, tets_a, cur_a, rest_b, tets_b, cur_b, stiffness, depth_cap=0.0, directions=A_INTO_B | B_INTO_A, fa0=None, fb0=None, dtype=np.float64):
    """The whole call.  rest_*: what the surfaces are built on; cur_* = x0 + q.  Returns dict(dirs=(a into b, b into a) of ``direction``'s
    dicts (None: not asked), fa, fb the two force vectors (n, 3) after the call, started from fa0 / fb0 (zero), force_on_a / force_on_b the
    sums of all contributions in the rule's order, max_depth the largest depth that entered a force)."""
    cur_a, cur_b = np.asarray(cur_a, dtype).reshape(-1, 3), np.asarray(cur_b, dtype).reshape(-1, 3)
    faces_a, vids_a = surface_of(rest_a, tets_a)
    faces_b, vids_b = surface_of(rest_b, tets_b)
    fa = np.zeros_like(cur_a) if fa0 is None else np.array(fa0, dtype).reshape(-1, 3)
    fb = np.zeros_like(cur_b) if fb0 is None else np.array(fb0, dtype).reshape(-1, 3)
    on_a, on_b, max_depth = np.zeros(3, dtype), np.zeros(3, dtype), 0.0
    dirs = [None, None]
    for k, bit in enumerate((A_INTO_B, B_INTO_A)):
        if not directions & bit:
            continue
        (xp, vp, fp, on_p), (xt, tt, ft, fct, on_t) = ((cur_a, vids_a, fa, on_a), (cur_b, tets_b, fb, faces_b, on_b)) if k == 0 else \
                                                      ((cur_b, vids_b, fb, on_b), (cur_a, tets_a, fa, faces_a, on_a))
        r = direction(xp, vp, xt, tt, fct, stiffness, depth_cap, dtype)
        dirs[k] = r
        for i in range(len(r["node"])):  # ascending surface vertex; inside a contact the corners 0, 1, 2
            if r["degenerate"][i]:
                continue
            F = r["force"][i]
            fp[r["node"][i]] += F
            on_p += F
            for corner in range(3):
                contribution = (-F) * r["bary"][i, corner]
                ft[fct[r["face"][i], corner]] += contribution
                on_t += contribution
            dep = float(r["depth"][i])
            max_depth = max(max_depth, min(dep, depth_cap) if depth_cap > 0 else dep)
    return dict(dirs=tuple(dirs), fa=fa, fb=fb, force_on_a=on_a, force_on_b=on_b, max_depth=max_depth, faces_a=faces_a, faces_b=faces_b, vids_a=vids_a, vids_b=vids_b)


def generic(r, extent, tol=1e-9):
    """(per candidate, per contact) bool: the decision lies outside rounding -- containment margin >= tol, gap >= tol * extent of the body.
    A contact whose candidate is not generic is not generic either."""
    cand_ok = r["contain_margin"] >= tol
    contact_ok = cand_ok[r["in_contact"]] & (r["gap"] >= tol * extent)
    return cand_ok, contact_ok


def spread(ref64, refld):
    """The largest difference between two evaluations of the same call, relative to stiffness * max_depth given by the caller: returns the
    largest absolute difference of the per-contact forces and the two force vectors (the contact sets must agree)."""
    worst = 0.0
    for r64, rld in zip(ref64["dirs"], refld["dirs"]):
        if r64 is None:
            continue
        assert np.array_equal(r64["node"], rld["node"]) and np.array_equal(r64["face"], rld["face"])
        if len(r64["node"]):
            worst = max(worst, float(np.abs(r64["force"].astype(np.longdouble) - rld["force"]).max()))
    for key in ("fa", "fb"):
        worst = max(worst, float(np.abs(ref64[key].astype(np.longdouble) - refld[key]).max()))
    return worst


# ---- inputs the tests share ----

def two_cubes(shape_a, shape_b, offset):
    """truth cubes a = (nx, ny, nz, cell) and b, a shifted so that its lower corner sits at b's lower corner plus the offset"""
    from fembrain_amd.meshgen import truth_cube
    va, ta = truth_cube(*shape_a)
    vb, tb = truth_cube(*shape_b)
    va = va + (vb.min(axis=0) + np.asarray(offset, np.float64) - va.min(axis=0))[None, :]
    return np.ascontiguousarray(va), ta, vb, tb


SHAPES = {
    "two_way": ((4, 4, 4, 0.1), (6, 3, 6, 0.1), (0.1291, 0.1637, 0.0559)),
    "many_onto_one": ((18, 3, 18, 0.025), (4, 3, 4, 0.2), (0.0713, 0.3637, 0.0591)),
    "deep": ((3, 3, 3, 0.05), (10, 10, 10, 0.1), (0.4137, 0.3871, 0.4319)),
}
