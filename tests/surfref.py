"""Restatement of the reference's render surface of a tet mesh, written from its cited lines; the yardstick of the fb_fem_surface tests.

* ``literal`` / ``vectorised``: SurfaceMesh::setupFromTetMesh (src/deformable/SurfaceMesh.cpp:141-213) -- every face that belongs to an odd
  number of elements, wound by the sign of the element's determinant (:165, :180-190), with the vertex order that insert / erase / insert
  on the std::set leaves (the last occurrence, :168-178), listed in the order of the sorted vertex triple (:200-207).
* ``normals``: VolMeshRender::sync (src/deformable/VolMeshRender.cpp:74-112) without the flip towards the camera (:83-91).
* ``aabb``: SurfaceMesh::updateAABB (SurfaceMesh.cpp:354-373) over the float positions of the surface vertices.

The properties at the end use none of the above, so that a misreading shared by the restatement and the code under test still shows."""
import numpy as np

FACES_POS = ((1, 2, 3), (2, 0, 3), (3, 0, 1), (1, 0, 2))   # det >= 0 (SurfaceMesh.cpp:181-184)
FACES_NEG = ((3, 2, 1), (3, 0, 2), (1, 0, 3), (2, 0, 1))   # det < 0  (:186-189)


def determinants(x, tets):
    v = np.asarray(x, np.float64).reshape(-1, 3)[np.asarray(tets, np.int64).reshape(-1, 4)]
    a, b, c = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], v[:, 3] - v[:, 0]
    cr = np.stack([b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]], axis=1)
    return (a[:, 0] * cr[:, 0] + a[:, 1] * cr[:, 1]) + a[:, 2] * cr[:, 2]


def literal(x, tets):
    """(faces (F, 3), face_tets (F,)): a dict toggled face by face exactly as PROCESS_FACE3 does, read out in sorted-key order"""
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    det = determinants(x, tets)
    s = {}
    for e, t in enumerate(tets):
        for f in (FACES_POS if det[e] >= 0 else FACES_NEG):
            tri = (int(t[f[0]]), int(t[f[1]]), int(t[f[2]]))
            k = tuple(sorted(tri))
            if k in s:
                del s[k]
            else:
                s[k] = (tri, e)
    keys = sorted(s)
    return (np.array([s[k][0] for k in keys], np.int64).reshape(-1, 3), np.array([s[k][1] for k in keys], np.int64))


def vectorised(x, tets):
    """the same by a stable lexsort: runs of equal sorted triples, odd counts survive with their last entry"""
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    det = determinants(x, tets)
    loc = np.where((det >= 0)[:, None, None], np.array(FACES_POS)[None], np.array(FACES_NEG)[None])
    tri = np.take_along_axis(tets[:, None, :].repeat(4, 1), loc, axis=2).reshape(-1, 3)
    key = np.sort(tri, 1)
    order = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))   # stable: element order inside a run
    ks = key[order]
    new = np.ones(len(ks), bool)
    new[1:] = (ks[1:] != ks[:-1]).any(1)
    start = np.nonzero(new)[0]
    end = np.append(start[1:], len(ks))
    last = order[end[(end - start) % 2 == 1] - 1]
    return tri[last], last // 4


def vertex_ids(faces):
    return np.unique(np.asarray(faces, np.int64))


def normals(pos, faces, ids=None):
    """(unit normals (V, 3) fp64 -- (0, 0, 0) where the sum has no length --, |sum| (V,)) of the nodes ``ids`` (default: vertex_ids(faces)):
    the fp64 sum, in ascending face order, of the unit normals (p1 - p0) x (p2 - p0) / |..| of the node's faces"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = vertex_ids(faces) if ids is None else np.asarray(ids, np.int64)
    fn = np.cross(pos[faces[:, 1]] - pos[faces[:, 0]], pos[faces[:, 2]] - pos[faces[:, 0]])
    fn = fn / np.linalg.norm(fn, axis=1)[:, None]
    s = np.zeros((len(pos), 3))
    corner_face = np.repeat(np.arange(len(faces)), 3)       # corners in face order: np.add.at adds in this order
    np.add.at(s, faces.reshape(-1), fn[corner_face])
    s = s[ids]
    length = np.linalg.norm(s, axis=1)
    return np.where(length[:, None] > 0, s / np.where(length > 0, length, 1.0)[:, None], 0.0), length


def aabb(xyz32):
    xyz32 = np.asarray(xyz32, np.float32).reshape(-1, 3)
    return np.stack([xyz32.min(0), xyz32.max(0)])


# ---- properties that use nothing of the above ----
def closed_and_oriented(faces):
    """every directed edge occurs once and its opposite once"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fw = np.sort(de[:, 0] * (1 << 32) + de[:, 1])
    bw = np.sort(de[:, 1] * (1 << 32) + de[:, 0])
    return len(np.unique(fw)) == len(fw) and np.array_equal(fw, bw)


def enclosed_volume(pos, faces):
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->", pos[f[:, 0]], np.cross(pos[f[:, 1]], pos[f[:, 2]])) / 6)


def element_volume(pos, tets):
    return float(np.abs(determinants(pos, tets)).sum() / 6)


def euler(faces):
    """V - E + F of a closed surface (E = 3 F / 2)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return len(np.unique(f)) - 3 * len(f) // 2 + len(f)


def read_obj(path):
    v, vn, f = [], [], []
    with open(path) as fh:
        for line in fh:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                v.append([float(t) for t in w[1:4]])
            elif w[0] == "vn":
                vn.append([float(t) for t in w[1:4]])
            elif w[0] == "f":
                f.append([int(t.split("/")[0]) - 1 for t in w[1:4]])
    return np.array(v, np.float32).reshape(-1, 3), np.array(vn, np.float32).reshape(-1, 3), np.array(f, np.int64).reshape(-1, 3)
