"""numpy restatement of the reference's three routines on disjoint mesh parts, with the ordering rules of fb_fem_parts:

- ``VolMesh::get_disjoint_parts`` (src/deformable/VolMesh.cpp:915-965): face-connected components of the element list, numbered in
  ascending order of their smallest element (it starts every part at ``*setCells.begin()``), cells ascending inside a part;
- ``CuttableMesh::splitParts`` (src/deformable/CuttableMesh.cpp:553-626), applied to the rest positions;
- one iteration of ``CuttableMesh::convertDisjointPartsToMeshes`` (:628-698): a part as a mesh, nodes in order of first use.

Plain and slow on purpose: what test_parts_gpu.py compares the device against, itself pinned by test_parts_host.py.
"""
import numpy as np


def face_pairs(tets):
    """(a, b) element pairs: consecutive carriers of every face (an equal sorted triple of node ids)"""
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    m = len(t)
    faces = np.sort(np.concatenate([t[:, [1, 2, 3]], t[:, [0, 2, 3]], t[:, [0, 1, 3]], t[:, [0, 1, 2]]]), axis=1)
    owner = np.tile(np.arange(m), 4)
    order = np.lexsort((owner, faces[:, 2], faces[:, 1], faces[:, 0]))
    fs, ow = faces[order], owner[order]
    same = np.nonzero(np.all(fs[1:] == fs[:-1], axis=1))[0]
    return ow[same], ow[same + 1]


def roots(tets):
    """per element the smallest element id of its face-connected component.  Labels fall to the smaller neighbour and jump to their
    label's label until nothing changes: the fixed point is constant on a component and, as a label never exceeds its element, is the
    component's smallest element."""
    m = len(np.asarray(tets).reshape(-1, 4))
    a, b = face_pairs(tets)
    lab = np.arange(m)
    while True:
        was = lab.copy()
        low = np.minimum(lab[a], lab[b])
        np.minimum.at(lab, a, low)
        np.minimum.at(lab, b, low)
        lab = lab[lab]
        if np.array_equal(lab, was):
            return lab


def element_volumes(x0, tets):
    """|u . (v x w)| / 6 with u, v, w = p0 - p3, p1 - p3, p2 - p3 (fb_fem_volume's expression)"""
    p = np.asarray(x0, np.float64).reshape(-1, 3)[np.asarray(tets, np.int64).reshape(-1, 4)]
    u, v, w = p[:, 0] - p[:, 3], p[:, 1] - p[:, 3], p[:, 2] - p[:, 3]
    det = (u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1]) + u[:, 1] * (v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2])) + u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0])
    return np.abs(det) / 6.0


def parts(x0, tets, n_nodes=None):
    """Everything fb_fem_parts / fb_fem_read_parts report: dict of n_parts, largest_part, n_shared_nodes, n_unused_nodes, element_part,
    node_part, elements, nodes, first_element, volume"""
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    n = len(np.asarray(x0).reshape(-1, 3)) if n_nodes is None else int(n_nodes)
    first, element_part = np.unique(roots(t), return_inverse=True)
    element_part = element_part.reshape(-1)
    k = len(first)
    node_part = np.full(n, k, np.int64)
    np.minimum.at(node_part, t.reshape(-1), np.repeat(element_part, 4))
    used = node_part < k
    pairs = np.unique(np.stack([np.repeat(element_part, 4), t.reshape(-1)], axis=1), axis=0)   # (part, node), once each
    nodes = np.bincount(pairs[:, 0], minlength=k)
    uses = np.bincount(pairs[:, 1], minlength=n)
    elements = np.bincount(element_part, minlength=k)
    vol = element_volumes(x0, t)
    return dict(n_parts=k, largest_part=int(np.argmax(elements)), n_shared_nodes=int((uses > 1).sum()), n_unused_nodes=int((~used).sum()),
                element_part=element_part.astype(np.int32), node_part=np.where(used, node_part, -1).astype(np.int32),
                elements=elements.astype(np.int32), nodes=nodes.astype(np.int32), first_element=first.astype(np.int32),
                volume=np.array([vol[element_part == j].sum() for j in range(k)]))


def split(x0, q, tets, quad, dist):
    """CuttableMesh::splitParts on the rest positions: dict of n_front_parts, n_back_parts, n_straddling_parts, shift (3,), sign (n,) (+1 a
    node of front parts only, -1 of back parts only, 0 otherwise), moved (n,) bool (the rest position changed), n_nodes_moved and x0 after"""
    x0 = np.asarray(x0, np.float64).reshape(-1, 3)
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    qd = np.asarray(quad, np.float64).reshape(4, 3)
    a, b = qd[1] - qd[0], qd[2] - qd[0]
    cr = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    nrm = cr / np.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2])
    shift = nrm * float(dist)
    c = (((qd[0] + qd[1]) + qd[2]) + qd[3]) * 0.25
    pos = x0 + np.asarray(q, np.float64).reshape(-1, 3)
    cen = (((pos[t[:, 0]] + pos[t[:, 1]]) + pos[t[:, 2]]) + pos[t[:, 3]]) * 0.25 - c
    dot = (cen[:, 0] * nrm[0] + cen[:, 1] * nrm[1]) + cen[:, 2] * nrm[2]
    front = dot > 0
    _, element_part = np.unique(roots(t), return_inverse=True)
    element_part = element_part.reshape(-1)
    k = int(element_part.max()) + 1
    n_front = np.bincount(element_part, weights=front, minlength=k).astype(np.int64)
    n_el = np.bincount(element_part, minlength=k)
    is_front, is_back = n_front == n_el, n_front == 0
    in_front, in_back = np.zeros(len(x0), bool), np.zeros(len(x0), bool)
    in_front[t[is_front[element_part]].reshape(-1)] = True
    in_back[t[is_back[element_part]].reshape(-1)] = True
    sign = in_front.astype(np.int64) - in_back.astype(np.int64)
    after = x0.copy()
    after[sign > 0] = x0[sign > 0] + shift
    after[sign < 0] = x0[sign < 0] - shift
    moved = np.any(after != x0, axis=1)
    return dict(n_front_parts=int(is_front.sum()), n_back_parts=int(is_back.sum()), n_straddling_parts=int(k - is_front.sum() - is_back.sum()),
                shift=shift, sign=sign, moved=moved, n_nodes_moved=int(moved.sum()), x0=after, min_distance=float(np.abs(dot).min()))


def extract(x0, tets, element_part, k):
    """part k as a mesh: (element_ids ascending, node_ids in order of first use, rest_xyz, tets_local) -- mapNodes of
    convertDisjointPartsToMeshes, cell by cell and corner by corner"""
    x0 = np.asarray(x0, np.float64).reshape(-1, 3)
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    ids = np.nonzero(np.asarray(element_part) == k)[0]
    local, order, cells = {}, [], []
    for e in ids:
        for n in t[e]:
            n = int(n)
            if n not in local:
                local[n] = len(order)
                order.append(n)
            cells.append(local[n])
    order = np.array(order, np.int32)
    return ids.astype(np.int32), order, x0[order], np.array(cells, np.int32).reshape(-1, 4)
