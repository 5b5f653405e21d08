"""A numpy restatement of fb_fem_cut's rules (include/fembrain_hip.h, fembrain_amd/csrc/subdivide.h), written for the tests from the rules
themselves -- not a transcription of the reference's subdivision tables.

Cut edges: every unique mesh edge, oriented from its lower to its higher node id, tested in fp64 against each usable quad of the strip
(triangle {q0,q2,q1}, then {q2,q3,q1}) with IntersectSegmentTriangle's operations in their order; cut iff an odd number of quads hit it,
t of the last hit.  Cases: A = the three edges at one node (4 pieces), B = four edges with the uncut two opposite (6 pieces), anything
else unhandled.  Cut edge k of the (lo, hi)-sorted list gets nodes N + 2k (lo's side) and N + 2k + 1 (hi's side).  Prisms split by the
lowest-global-id rule; piece vertex order fixed by the sign of the piece in the parent's barycentric frame, split points at midpoints.
"""
import itertools

import numpy as np

EPS = float(np.float32(0.0001))  # EPSILON (a float constant) as a double
EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def edge_of(i, j):
    return EDGES.index((min(i, j), max(i, j)))


def code_at(n):
    return sum(1 << e for e, (a, b) in enumerate(EDGES) if n in (a, b))


CASE_A = {code_at(n): n for n in range(4)}                                             # code -> isolated node
CASE_B = {63 ^ (1 << edge_of(0, x)) ^ (1 << (5 - edge_of(0, x))): x for x in (1, 2, 3)}  # code -> the node sharing the uncut edge with 0


def usable_quads(strip):
    p = np.asarray(strip, np.float64).reshape(-1, 3)
    assert len(p) >= 4 and len(p) % 2 == 0
    out = []
    for i in range((len(p) - 2) // 2):
        q = p[2 * i:2 * i + 4]
        d1, d2, d3 = q[1] - q[0], q[2] - q[0], q[3] - q[2]
        l1 = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2]
        l2 = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]
        l3 = d3[0] * d3[0] + d3[1] * d3[1] + d3[2] * d3[2]
        if l1 * l2 < EPS or l3 < EPS:
            continue
        out.append(q)
    return out


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def segments(plo, phi):
    d = phi - plo
    ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):  # (a zero-length edge, e.g. between unwelded twins: 0 * inf, not taken)
        inv = 1.0 / ln
        rd = np.where((ln != 0.0)[:, None], d * inv[:, None], d)
    return rd, ln


def segment_triangle(s0, rd, ln, p0, p1, p2):
    """IntersectSegmentTriangle, vectorised over segments: (hit, t)"""
    e1, e2 = p1 - p0, p2 - p0
    q = _cross(rd, e2[None, :])
    a = _dot(e1[None, :], q)
    ok = ~(np.abs(a) < EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 1.0 / a
        s = s0 - p0[None, :]
        u = f * _dot(s, q)
        ok &= ~(u < 0.0)
        r = _cross(s, e1[None, :])
        v = f * _dot(rd, r)
        ok &= ~((v < 0.0) | ((u + v) > 1.0))
        t = f * _dot(e2[None, :], r)
    ok &= (t >= 0.0) & (t <= ln)
    return ok, t


def cut_edges(pos, lo, hi, quads):
    """odd-count rule over the quads: (cut mask, t of the last hit)"""
    s0 = pos[lo]
    rd, ln = segments(s0, pos[hi])
    odd = np.zeros(len(lo), bool)
    tl = np.zeros(len(lo))
    for q in quads:
        h1, t1 = segment_triangle(s0, rd, ln, q[0], q[2], q[1])
        h2, t2 = segment_triangle(s0, rd, ln, q[2], q[3], q[1])
        hit = h1 | h2
        odd ^= hit
        tl = np.where(hit, np.where(h1, t1, t2), tl)
    return odd, tl


def prism_tets(ids):
    """the lowest-global-id split of prism v0 v1 v2 | v3 v4 v5 (vi - v(i+3) lateral): 3 tets as positions 0..5"""
    m = int(np.argmin(ids))
    layer, rot = m // 3, m % 3
    w = [((j // 3 + layer) & 1) * 3 + (j % 3 + rot) % 3 for j in range(6)]
    wid = [ids[k] for k in w]
    if min(wid[1], wid[5]) < min(wid[2], wid[4]):
        t = [(0, 1, 2, 5), (0, 1, 5, 4), (0, 4, 5, 3)]
    else:
        t = [(0, 1, 2, 4), (0, 4, 2, 5), (0, 4, 5, 3)]
    return [tuple(w[k] for k in tt) for tt in t]


# a piece vertex: ("n", i) old local node, ("s", i, j, side) split point of edge (i, j) on side's side
def _bary(tok):
    b = np.zeros(4)
    if tok[0] == "n":
        b[tok[1]] = 1.0
    else:
        b[tok[1]] = b[tok[2]] = 0.5
    return b[1:]


def orient(toks):
    b = [_bary(t) for t in toks]
    d = np.linalg.det(np.array([b[1] - b[0], b[2] - b[0], b[3] - b[0]]))
    assert d != 0.0
    return list(toks) if d > 0 else [toks[0], toks[1], toks[3], toks[2]]


def _S(i, j, side):
    return ("s", min(i, j), max(i, j), side)


def piece_tokens(code):
    """the pieces of a case A / B element as (kind, tokens): 'tet' (4 tokens) or 'prism' (6)"""
    if code in CASE_A:
        a = CASE_A[code]
        r = [k for k in range(4) if k != a]
        return [("tet", [("n", a)] + [_S(a, x, a) for x in r]), ("prism", [_S(a, x, x) for x in r] + [("n", x) for x in r])]
    pa, pb = 0, CASE_B[code]
    pc, pd = [k for k in (1, 2, 3) if k != pb]
    s1 = [("n", pa), _S(pa, pc, pa), _S(pa, pd, pa), ("n", pb), _S(pb, pc, pb), _S(pb, pd, pb)]
    s2 = [("n", pc), _S(pa, pc, pc), _S(pb, pc, pc), ("n", pd), _S(pa, pd, pd), _S(pb, pd, pd)]
    return [("prism", s1), ("prism", s2)]


def tet_vol6(p):
    return np.linalg.det(np.array([p[1] - p[0], p[2] - p[0], p[3] - p[0]]))


def cut(x0, tets, strip, q=None, mode="bake"):
    """the expected result of fb_fem_cut on a mesh with rest positions x0 and displacement q: dict(status, counts..., removed, added,
    new_xyz, edge_nodes, edge_frac, codes)"""
    x0 = np.asarray(x0, np.float64).reshape(-1, 3)
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    q = np.zeros_like(x0) if q is None else np.asarray(q, np.float64).reshape(-1, 3)
    pos = x0 + q
    quads = usable_quads(strip)
    N = len(x0)
    out = dict(n_quads=len(quads), status=0, n_cut_edges=0, n_case_a=0, n_case_b=0, n_unhandled=0, removed=np.zeros(0, np.int32),
               added=np.zeros((0, 4), np.int32), new_xyz=np.zeros((0, 3)), edge_nodes=np.zeros((0, 2), np.int32), edge_frac=np.zeros(0),
               unhandled_ids=np.zeros(0, np.int32), codes=np.zeros(len(t), np.int32))
    if not quads:
        return out
    lo = np.minimum(t[:, [a for a, b in EDGES]], t[:, [b for a, b in EDGES]])
    hi = np.maximum(t[:, [a for a, b in EDGES]], t[:, [b for a, b in EDGES]])
    keys = lo * (1 << 32) + hi
    uk, inv = np.unique(keys.reshape(-1), return_inverse=True)
    ulo, uhi = uk >> 32, uk & 0xffffffff
    cutm, tt = cut_edges(pos, ulo, uhi, quads)
    codes = (cutm[inv].reshape(-1, 6) * (1 << np.arange(6))).sum(1).astype(np.int32)
    out["codes"] = codes
    cut_ids = np.nonzero(codes)[0]
    isa = np.isin(codes, list(CASE_A))
    isb = np.isin(codes, list(CASE_B))
    out["n_case_a"], out["n_case_b"] = int(isa.sum()), int(isb.sum())
    unh = cut_ids[~(isa | isb)[cut_ids]]
    out["n_unhandled"] = len(unh)
    if len(cut_ids) == 0:
        return out
    if len(unh):
        out["status"] = 2
        out["unhandled_ids"] = unh[:64].astype(np.int32)
        return out
    ck = uk[cutm]
    ct = tt[cutm]
    K = len(ck)
    clo, chi = (ck >> 32).astype(np.int64), (ck & 0xffffffff).astype(np.int64)
    rd, ln = segments(pos[clo], pos[chi])
    frac = ct / ln
    if mode == "bake":
        x = pos[clo] + rd * ct[:, None]
        rest = pos
    else:
        x = x0[clo] + frac[:, None] * (x0[chi] - x0[clo])
        rest = x0
    new_xyz = np.repeat(x, 2, axis=0)
    kidx = {int(k): i for i, k in enumerate(ck)}

    def tok_id(g, tok):
        if tok[0] == "n":
            return int(g[tok[1]])
        a, b = int(g[tok[1]]), int(g[tok[2]])
        l, h = min(a, b), max(a, b)
        k = kidx[l * (1 << 32) + h]
        return N + 2 * k + (1 if int(g[tok[3]]) == h else 0)

    allpos = np.concatenate([rest, new_xyz])
    added, ratios = [], []
    for e in cut_ids:
        g = t[e]
        pv = tet_vol6(allpos[g])
        for kind, toks in piece_tokens(int(codes[e])):
            if kind == "tet":
                sets = [toks]
            else:
                ids = [tok_id(g, tk) for tk in toks]
                sets = [[toks[k] for k in tt4] for tt4 in prism_tets(ids)]
            for s in sets:
                s = orient(s)
                ids = [tok_id(g, tk) for tk in s]
                added.append(ids)
                ratios.append(tet_vol6(allpos[ids]) / pv)
    out.update(status=1, n_cut_edges=K, removed=cut_ids.astype(np.int32), added=np.array(added, np.int32).reshape(-1, 4), new_xyz=new_xyz,
               edge_nodes=np.repeat(np.stack([clo, chi], 1), 2, axis=0).astype(np.int32), edge_frac=np.repeat(frac, 2),
               min_volume_ratio=float(np.min(ratios)), ratios=np.array(ratios))
    return out


def plane_strip(point, normal, half=10.0):
    """one planar quad through `point` with normal `normal`, spanning +-half in two directions"""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    c = np.asarray(point, np.float64)
    return np.array([c - half * a - half * b, c - half * a + half * b, c + half * a - half * b, c + half * a + half * b])


def face_components(tets):
    """connected components of the elements under face adjacency"""
    t = np.asarray(tets, np.int64)
    m = len(t)
    faces = np.sort(np.concatenate([t[:, [1, 2, 3]], t[:, [0, 2, 3]], t[:, [0, 1, 3]], t[:, [0, 1, 2]]]), axis=1)
    owner = np.tile(np.arange(m), 4)
    order = np.lexsort(faces.T[::-1])
    fs, os_ = faces[order], owner[order]
    same = np.all(fs[1:] == fs[:-1], axis=1)
    parent = np.arange(m)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in np.nonzero(same)[0]:
        a, b = find(os_[i]), find(os_[i + 1])
        if a != b:
            parent[a] = b
    roots = np.array([find(i) for i in range(m)])
    return roots


def max_face_share(tets):
    t = np.asarray(tets, np.int64)
    faces = np.sort(np.concatenate([t[:, [1, 2, 3]], t[:, [0, 2, 3]], t[:, [0, 1, 3]], t[:, [0, 1, 2]]]), axis=1)
    _, cnt = np.unique(faces, axis=0, return_counts=True)
    return int(cnt.max())


def all_prism_orders_positive():
    """every one of the 720 orders of a prism's six ids gives 3 positive tets (unit right prism)"""
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float64)
    for perm in itertools.permutations(range(6)):
        tets = prism_tets(list(perm))
        vols = [tet_vol6(P[list(tt)]) for tt in tets]
        if not all(abs(v) > 0 for v in vols) or abs(sum(abs(v) for v in vols) - 3.0) > 1e-12:
            return False
    return True
