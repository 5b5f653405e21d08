"""An independent checker for the result of fb_fem_cut, in plain numpy and fractions.  It knows the contract of the delta (include/fembrain_hip.h:
removed parents ascending, 4 or 6 pieces per parent in that order, two coincident nodes per cut edge numbered by sorted unique edge) but none
of the piece tables or the prism rule of tests/cutref.py: partition, conformity, sides and split points are stated as properties of the
cut mesh, so a restatement and a device that share a wrong table both fail here.

``check_cut`` raises AssertionError with the first property that does not hold.
"""
from fractions import Fraction

import numpy as np

EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
_FACES = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))

# Item 4, the split points against exact rational arithmetic.  SPLIT_MEASURED is the largest distance between tests/cutref.py's split
# points and the exact plane / edge intersections, taken normal to the blade (split_errors), divided by the largest coordinate magnitude among the blade's corners and the mesh,
# over every planar cut of tests/test_fem_cut_checks.py (the inputs of the GPU file); test_split_tolerance_is_four_times_the_measured_error
# measures it again and keeps the constant honest.  The device must equal cutref bit for bit, so this bounds the restatement.
SPLIT_MEASURED = 3.1e-16  # measured: 3.094e-16 (a 1,500-point Delaunay mesh under a smooth displacement, blade corners at |x| = 14)
SPLIT_TOL = 4 * SPLIT_MEASURED


def vol6(x, t):
    p = x[t]
    return np.einsum("ij,ij->i", p[:, 1] - p[:, 0], np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]))


def _faces(t):
    """(sorted node triples (4m, 3), owning element (4m,))"""
    t = np.asarray(t, np.int64)
    return np.sort(np.concatenate([t[:, list(f)] for f in _FACES]), axis=1), np.tile(np.arange(len(t)), 4)


def _face_keys(f, n):
    return (f[:, 0] * n + f[:, 1]) * n + f[:, 2]


def parent_codes(tets, delta):
    """6-bit cut code of every removed parent, from the delta's edge list alone (bit e: local edge EDGES[e] is a cut edge)"""
    t = np.asarray(tets, np.int64).reshape(-1, 4)[np.asarray(delta["removed"], np.int64)]
    en = np.asarray(delta["edge_nodes"], np.int64).reshape(-1, 2)[::2]
    big = 1 << 32
    cut = en[:, 0] * big + en[:, 1]
    codes = np.zeros(len(t), np.int64)
    for e, (a, b) in enumerate(EDGES):
        k = np.minimum(t[:, a], t[:, b]) * big + np.maximum(t[:, a], t[:, b])
        codes |= np.isin(k, cut).astype(np.int64) << e
    return codes


def coverage(tets, delta):
    """item 5: the set of (code, rank of the caller id of local node 0, 1, 2, 3 inside the element) over the removed parents"""
    rem = np.asarray(delta["removed"], np.int64)
    if len(rem) == 0:
        return set()
    t = np.asarray(tets, np.int64).reshape(-1, 4)[rem]
    ranks = np.argsort(np.argsort(t, axis=1), axis=1)
    return set(map(tuple, np.concatenate([parent_codes(tets, delta)[:, None], ranks], axis=1).tolist()))


def groups(code):
    """the two node groups a code leaves connected through uncut edges, or None when the code is not such a two-sided pattern"""
    comp = list(range(4))
    for e, (a, b) in enumerate(EDGES):
        if not code >> e & 1:
            ca, cb = comp[a], comp[b]
            comp = [ca if c == cb else c for c in comp]
    ids = sorted(set(comp))
    if len(ids) != 2:
        return None
    g = [frozenset(i for i in range(4) if comp[i] == c) for c in ids]
    for e, (a, b) in enumerate(EDGES):  # every cut edge joins the two groups
        if bool(code >> e & 1) != ((a in g[0]) != (b in g[0])):
            return None
    return g


ALL_PAIRS = 7 * 24  # the 4 + 3 two-sided codes times the 24 rank orders of four ids


def exact_split(a, b, tri):
    """the point of segment a -> b on the plane through the three points of tri, in Fractions: (t from a, point)"""
    F = Fraction
    a, b = [F(float(c)) for c in a], [F(float(c)) for c in b]
    p0, p1, p2 = ([F(float(c)) for c in p] for p in tri)
    u = [p1[i] - p0[i] for i in range(3)]
    w = [p2[i] - p0[i] for i in range(3)]
    n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
    d = [b[i] - a[i] for i in range(3)]
    den = sum(n[i] * d[i] for i in range(3))
    t = sum(n[i] * (p0[i] - a[i]) for i in range(3)) / den
    return t, [a[i] + t * d[i] for i in range(3)]


def split_errors(pos, delta, strip, rest=None):
    """item 4 for a planar one-quad strip: per cut edge the distance between the delta's node and the exact intersection of the edge (at the
    positions pos the blade met) with the plane of the quad's triangle {q0, q2, q1} or {q2, q3, q1}, whichever is nearer (the two planes
    differ by the rounding of the fourth corner).  rest: CARRY, the node lies at the same exact fraction of the edge in the rest positions.
    The routine's rounding moves the point ALONG the edge, by its error normal to the blade over the cosine between edge and normal (an edge
    that meets the blade at two degrees moves thirty times as far as one that meets it squarely), so the distance is reported times that
    cosine: the error normal to the blade.  Returns (those distances, errors of edge_frac, scale = the largest coordinate magnitude
    involved, which the roundings are relative to)."""
    q = np.asarray(strip, np.float64).reshape(-1, 3)
    assert len(q) == 4, "the exact split points are defined for one planar quad"
    tris = ((q[0], q[2], q[1]), (q[2], q[3], q[1]))
    en = np.asarray(delta["edge_nodes"], np.int64).reshape(-1, 2)[::2]
    xyz = np.asarray(delta["new_xyz"], np.float64).reshape(-1, 3)[::2]
    frac = np.asarray(delta["edge_frac"], np.float64)[::2]
    dist, ferr = np.zeros(len(en)), np.zeros(len(en))
    nrm = np.cross(q[2] - q[0], q[1] - q[0])
    nrm /= np.linalg.norm(nrm)
    dd = pos[en[:, 1]] - pos[en[:, 0]]
    cos = np.abs(dd @ nrm) / np.linalg.norm(dd, axis=1)
    for k, (lo, hi) in enumerate(en):
        best = None
        for tri in tris:
            t, pt = exact_split(pos[lo], pos[hi], tri)
            if rest is not None:
                r0, r1 = [Fraction(float(c)) for c in rest[lo]], [Fraction(float(c)) for c in rest[hi]]
                pt = [r0[i] + t * (r1[i] - r0[i]) for i in range(3)]
            d2 = sum((Fraction(float(xyz[k][i])) - pt[i]) ** 2 for i in range(3))
            if best is None or d2 < best[0]:
                best = (d2, t)
        dist[k] = float(best[0]) ** 0.5
        ferr[k] = abs(float(Fraction(float(frac[k])) - best[1]))
    scale = max(float(np.abs(q).max()), float(np.abs(pos).max()), 0.0 if rest is None else float(np.abs(rest).max()))
    return dist * cos, ferr, scale


def check_cut(pos, tets, delta, strip=None, plane=None, rest=None, split_tol=None, components=None):
    """pos: the node positions the blade met (rest + displacement).  rest: the rest positions when the cut was a CARRY (the pieces then live
    in the rest shape); None for BAKE (they live in pos).  delta: what fb_fem_cut / cutref.cut returned with status DONE or DRY.
    plane = (point, normal) for a planar strip across the whole body: adds the side-of-plane checks and, with strip (its one quad), the
    exact split points.  components: the number of face-connected components the cut mesh must have, when the caller knows it.
    Returns the coverage set of the cut."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    shape = pos if rest is None else np.asarray(rest, np.float64).reshape(-1, 3)
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    N = len(pos)
    rem = np.asarray(delta["removed"], np.int64)
    add = np.asarray(delta["added"], np.int64).reshape(-1, 4)
    nx = np.asarray(delta["new_xyz"], np.float64).reshape(-1, 3)
    en = np.asarray(delta["edge_nodes"], np.int64).reshape(-1, 2)
    fr = np.asarray(delta["edge_frac"], np.float64)
    assert len(rem) and np.all(np.diff(rem) > 0) and rem[0] >= 0 and rem[-1] < len(t), "removed ids ascend inside the element list"
    # ---- the node list: two coincident copies per cut edge, numbered by sorted unique (lo, hi) ----
    K = len(nx) // 2
    assert len(nx) == 2 * K == len(en) == len(fr) and K > 0
    assert np.array_equal(nx[0::2], nx[1::2]), "the two copies of a split point differ"
    assert np.array_equal(en[0::2], en[1::2]) and np.array_equal(fr[0::2], fr[1::2])
    e1 = en[0::2]
    assert np.all(e1[:, 0] < e1[:, 1]) and e1.min() >= 0 and e1.max() < N, "cut edges run from the lower to the higher old id"
    assert np.all(np.diff(e1[:, 0] * (1 << 32) + e1[:, 1]) > 0), "new nodes are numbered by sorted unique edge"
    assert np.all((fr >= 0) & (fr <= 1))
    assert add.min() >= 0 and add.max() < N + 2 * K
    assert np.array_equal(np.unique(add[add >= N]) - N, np.arange(2 * K)), "every new node is used by a piece"
    allx = np.concatenate([shape, nx])
    # ---- 1. partition ----
    codes = parent_codes(t, delta)
    nbits = np.array([bin(int(c)).count("1") for c in codes])
    assert np.all((nbits == 3) | (nbits == 4)), "a removed parent with %s cut edges" % sorted(set(nbits.tolist()))
    npieces = np.where(nbits == 3, 4, 6)
    first = np.concatenate([[0], np.cumsum(npieces)])
    assert first[-1] == len(add), "%d pieces for parents whose codes need %d" % (len(add), first[-1])
    pv = vol6(shape, t[rem])
    cv = vol6(allx, add)
    owner = np.repeat(np.arange(len(rem)), npieces)
    pp = shape[t[rem]]
    edge2 = np.zeros(len(rem))
    for a, b in EDGES:
        edge2 = np.maximum(edge2, ((pp[:, a] - pp[:, b]) ** 2).sum(1))
    # a split point is rounded to an ulp or two of its coordinates (2.2e-16 |x|) and moves 6 V of a piece by at most that times twice a
    # face area (<= edge^2); 1e-13 |x| edge^2 is some twenty such roundings over the split points of the six pieces, plus the sum's own
    vtol = 1e-13 * np.abs(pp).max(axis=(1, 2)) * edge2 + 1e-12 * np.abs(pv)
    assert np.all(pv != 0)
    sgn = np.sign(pv)
    rev = cv * sgn[owner] < -vtol[owner]
    assert not rev.any(), "piece %d (of parent %d) is reversed" % (np.argmax(rev), rem[owner[np.argmax(rev)]])
    sums = np.bincount(owner, weights=cv, minlength=len(rem))
    worst = np.abs(sums - pv) - vtol
    assert np.all(worst <= 0), "the pieces of parent %d sum to %r of its volume" % (rem[np.argmax(worst)], (sums / pv)[np.argmax(worst)])
    # ---- 3. sides ----
    old_side = None
    if plane is not None:
        old_side = np.sign((pos - np.asarray(plane[0], np.float64)) @ np.asarray(plane[1], np.float64))
    tr = t[rem]
    for i in range(len(rem)):
        g = groups(int(codes[i]))
        assert g is not None, "parent %d: code %d is neither case A nor case B" % (rem[i], codes[i])
        gid = [frozenset(int(tr[i][j]) for j in grp) for grp in g]
        if old_side is not None:
            s = [set(old_side[list(grp)].tolist()) for grp in gid]
            assert len(s[0]) == 1 and len(s[1]) == 1 and s[0] != s[1] and 0.0 not in s[0] | s[1], "parent %d: the groups are not the plane's sides" % rem[i]
        seen = set()
        for p in add[first[i]:first[i + 1]]:
            old = [int(n) for n in p if n < N]
            assert old, "a piece of parent %d has no old node" % rem[i]
            mine = [grp for grp in gid if old[0] in grp]
            assert len(mine) == 1 and all(n in mine[0] for n in old), "a piece of parent %d holds old nodes of both sides (or of another element)" % rem[i]
            seen.add(mine[0])
            news = [int(n) - N for n in p if n >= N]
            assert len(set(k // 2 for k in news)) == len(news), "both copies of one split point in a piece"
            for k in news:
                lo, hi = int(en[k][0]), int(en[k][1])
                assert (lo in mine[0]) != (hi in mine[0]), "a piece of parent %d uses a split point that is not on its parent's cut edges" % rem[i]
                assert k % 2 == (0 if lo in mine[0] else 1), "parent %d: node %d is the other side's copy of edge (%d, %d)" % (rem[i], k + N, lo, hi)
        assert len(seen) == 2
    # ---- 2. conformity ----
    keep = np.ones(len(t), bool)
    keep[rem] = False
    t2 = np.concatenate([t[keep], add])
    M = N + 2 * K
    f2, own2 = _faces(t2)
    k2 = _face_keys(f2, M)
    order = np.argsort(k2, kind="stable")
    _, start, cnt = np.unique(k2[order], return_index=True, return_counts=True)
    assert cnt.max() <= 2, "a face shared by %d elements" % cnt.max()
    f0, _ = _faces(t)
    u0, c0 = np.unique(_face_keys(f0, M), return_counts=True)
    assert c0.max() <= 2
    boundary0 = u0[c0 == 1]
    single = f2[order][start[cnt == 1]]
    single = single[(single < N).any(axis=1)]   # (a): a face of new nodes only lies on the blade
    if len(single):
        # (b): the old nodes and both ends of the cut edge of every new node are the three corners of one face that had one owner
        ends = np.where((single < N)[:, :, None], np.repeat(single[:, :, None], 2, axis=2), en[np.maximum(single - N, 0)]).reshape(-1, 6)
        corners = [sorted(set(r)) for r in ends.tolist()]
        assert all(len(c) == 3 for c in corners), "an open face that lies in no face of its parent"
        inb = np.isin(_face_keys(np.array(corners, np.int64), M), boundary0)
        assert np.all(inb), "%d open faces lie inside faces that two elements shared before the cut (a quad split by different diagonals)" % (~inb).sum()
    if old_side is not None:
        # every element of the cut mesh lies on one side, and no face joins the two
        s2 = np.where(t2 < N, old_side[np.minimum(t2, N - 1)], np.nan)
        lo_s, hi_s = np.nanmin(s2, axis=1), np.nanmax(s2, axis=1)
        assert np.all(lo_s == hi_s) and np.all(lo_s != 0), "an element with old nodes on both sides of the plane"
        o = own2[order]
        pair = start[cnt == 2]
        assert np.all(lo_s[o[pair]] == lo_s[o[pair + 1]]), "a face joins elements of opposite sides"
    if components is not None:
        import cutref
        assert len(np.unique(cutref.face_components(t2))) == components
    # ---- 4. split points ----
    if plane is not None and strip is not None:
        dist, _, scale = split_errors(pos, delta, strip, rest)
        tol = (SPLIT_TOL if split_tol is None else split_tol) * scale
        assert dist.max() <= tol, "split point %d is %g from the exact intersection (allowed %g)" % (np.argmax(dist), dist.max(), tol)
    return coverage(t, delta)
