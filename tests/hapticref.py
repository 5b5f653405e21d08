"""numpy restatements of the haptic probe's picking and volume (fb_fem_pick_vertex / fb_fem_pick_box / fb_fem_volume), written in the
operation orders include/fembrain_hip.h names, so that the device results can be compared bit for bit.  The spread's restatement is
``fembrain_amd.fem.spread_haptic_forces``."""
import numpy as np


def positions(x0, q=None):
    """x0 + q, one fp64 add per coordinate"""
    p = np.asarray(x0, np.float64).reshape(-1, 3)
    return p.copy() if q is None else p + np.asarray(q, np.float64).reshape(-1, 3)


def pick_vertex(p, wpos):
    """(index, position, d) of VolMesh::findClosestVertex: d = dx*dx + dy*dy + dz*dz, the lowest index of the smallest d"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    w = np.asarray(wpos, np.float64)
    dx, dy, dz = p[:, 0] - w[0], p[:, 1] - w[1], p[:, 2] - w[2]
    d = (dx * dx + dy * dy) + dz * dz
    best = -1
    for i in range(len(d)):            # the reference's loop: a strict "<" keeps the first of equal minima
        if best < 0 or d[i] < d[best]:
            best = i
    return best, p[best].copy(), float(d[best])


def pick_box(p, lo, hi):
    """(ascending indices, positions) of the nodes with lo <= p <= hi on all three axes"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    inside = (p[:, 0] >= lo[0]) & (p[:, 0] <= hi[0]) & (p[:, 1] >= lo[1]) & (p[:, 1] <= hi[1]) & (p[:, 2] >= lo[2]) & (p[:, 2] <= hi[2])
    ids = np.nonzero(inside)[0].astype(np.int32)
    return ids, p[ids].copy()


def element_volumes(p, tets):
    """|u . (v x w)| / 6 per element, u, v, w = p0 - p3, p1 - p3, p2 - p3, as u0 (v1 w2 - v2 w1) + u1 (v2 w0 - v0 w2) + u2 (v0 w1 - v1 w0)"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    u, v, w = p[t[:, 0]] - p[t[:, 3]], p[t[:, 1]] - p[t[:, 3]], p[t[:, 2]] - p[t[:, 3]]
    a = u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1])
    b = u[:, 1] * (v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2])
    c = u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0])
    return np.abs((a + b) + c) / 6.0


def node_pattern(n_nodes, tets):
    """(bptr, bcol) of the node-level stiffness pattern: row i lists, ascending, i and every node that shares an element with it"""
    rows = [{i} for i in range(n_nodes)]
    for t in np.asarray(tets, np.int64).reshape(-1, 4):
        for a in t:
            rows[int(a)].update(int(b) for b in t)
    bptr = np.zeros(n_nodes + 1, np.int32)
    bptr[1:] = np.cumsum([len(r) for r in rows])
    bcol = np.array([c for r in rows for c in sorted(r)], np.int32)
    return bptr, bcol


def spread_by_levels(n_nodes, tets, indices, forces, size, ext_forces, batch=32):
    """The device's formulation of the spread (fembrain_amd/csrc/haptic.hip), restated: direct adds over all sources first (the first
    occurrence of an id adds its later duplicates in order), then per batch of sources a level per (source, node) found by size-1
    sweeps over the element list -- an element with a node of level j-1 gives j to its nodes without a level -- and one pass over the
    nodes that adds mag[level] * f_s for s ascending.  Adds in place; must equal ``spread_haptic_forces`` bit for bit."""
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    f = np.asarray(forces, np.float64).reshape(-1, 3)
    ids = [int(i) for i in indices]
    out = ext_forces.reshape(-1, 3)
    for s, i in enumerate(ids):
        if i in ids[:s]:
            continue
        for k in range(s, len(ids)):
            if ids[k] == i:
                out[i] += f[k]
    mag = [1.0] + [1.0 * (size - j) / float(size) for j in range(1, size)]
    for base in range(0, len(ids), batch):
        chunk = ids[base:base + batch]
        level = np.full((len(chunk), n_nodes), 0xFF, np.uint8)
        for s, i in enumerate(chunk):
            level[s, i] = 0
        for j in range(1, size):
            for s in range(len(chunk)):
                lv = level[s][t]                                  # (the sweep reads the array it writes: a node that gets j in this
                hit = (lv == j - 1).any(axis=1)                    # sweep never reads as j-1, so the order inside a sweep is immaterial)
                nodes = t[hit][lv[hit] == 0xFF]
                level[s, nodes] = j
        for node in range(n_nodes):
            for s in range(len(chunk)):
                lv = int(level[s, node])
                if 1 <= lv <= size - 1:
                    out[node] += mag[lv] * f[base + s]
    return ext_forces
