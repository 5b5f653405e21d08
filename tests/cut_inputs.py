"""The meshes and blades of tests/test_fem_cut_unstructured_gpu.py, kept apart so that tests/test_fem_cut_checks.py can run the restatement
(tests/cutref.py) through the independent checker (tests/cutchecks.py) on the same inputs without a GPU."""
import os

import numpy as np

import cutref as cr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHIPPED = ("beam3", "disc", "pyramid", "peanut", "dumbel", "dumbelclose", "eggshell", "implicit_sphere")
# face-connected components before a cut (peanut and dumbel hold two bodies, implicit_sphere is an unwelded soup of cells)
SHIPPED_BODIES = dict(beam3=1, disc=1, pyramid=1, peanut=2, dumbel=2, dumbelclose=1, eggshell=1)


def delaunay(n, seed):
    """Delaunay tetrahedra of n random points of [-1, 1]^3 in scipy's mixed orientations (the points come in random order: no id order
    follows the geometry); slivers below 1e-7 of volume dropped.  Returns (points, tets, fixed DOFs = the nodes with x < -0.8)."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, size=(n, 3))
    t = Delaunay(pts).simplices.astype(np.int32)
    t = t[rng.permutation(len(t))]
    vol = np.einsum("ij,ij->i", pts[t[:, 1]] - pts[t[:, 0]], np.cross(pts[t[:, 2]] - pts[t[:, 0]], pts[t[:, 3]] - pts[t[:, 0]])) / 6
    t = np.ascontiguousarray(t[np.abs(vol) > 1e-7])
    assert (vol > 1e-7).any() and (vol < -1e-7).any()
    fixed = np.nonzero(pts[:, 0] < -0.8)[0]
    return pts, t, (3 * fixed[:, None] + np.arange(3)[None, :]).reshape(-1).astype(np.int32)


def random_planes(seed, k, centre=(0.0, 0.0, 0.0), spread=0.3, half=10.0):
    """k planes (point, unit normal, strip) through random points within `spread` of `centre`"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.asarray(centre, np.float64) + rng.uniform(-spread, spread, 3)
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        out.append((p, n, cr.plane_strip(p, n, half=half)))
    return out


def shipped(name):
    """(vertices, tets, fixed DOFs) of tests/golden/fem_<name>.npz"""
    d = np.load(os.path.join(GOLDEN, "fem_%s.npz" % name))
    fv = np.sort(d["fixed_vertices"].astype(np.int64))
    return d["verts"].astype(np.float64), np.ascontiguousarray(d["tets"], np.int32), (3 * fv[:, None] + np.arange(3)[None, :]).reshape(-1).astype(np.int32)


def shipped_planes(name, v, k=3):
    """k random planes near the centroid of a shipped mesh (within a tenth of its extent), wide enough to cross all of it"""
    ext = float((v.max(0) - v.min(0)).max())
    return random_planes(100 + SHIPPED.index(name), k, centre=v.mean(0), spread=0.1 * ext, half=4.0 * ext)


def folded_strip(n_quads, fold, seed, half=10.0):
    """a strip of n_quads quads through a random point near the origin whose sections turn by `fold` radians (alternating sign plus a drift,
    so the blade is neither planar nor a regular zigzag) about the strip's long axis.  Long sections: the folds lie inside [-1, 1]^3 only
    for the middle ones, the outer sections leave the body."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.2, 0.2, 3)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)                       # the fold axis (rails run along it)
    b = np.cross(a, rng.normal(size=3))
    b /= np.linalg.norm(b)
    m = n_quads + 1                              # rails
    step = np.full(n_quads, 0.5)
    step[0] = step[-1] = half                    # the outer sections reach beyond the body
    ang = np.cumsum(np.concatenate([[0.0], fold * (-1.0) ** np.arange(n_quads - 1) + 0.1 * fold]))
    pts = [np.zeros(3)]
    for i in range(n_quads):
        d = np.cos(ang[i]) * b + np.sin(ang[i]) * np.cross(a, b)
        pts.append(pts[-1] + step[i] * d)
    pts = np.array(pts)
    pts += c - pts[m // 2]
    return np.concatenate([np.stack([p - half * a, p + half * a]) for p in pts])


def v_strip(a, half=10.0):
    """two wings from an apex line outside the body (x = -1.6, along z), a and -0.7 a radians off the x axis: many edges cross both"""
    apex = np.array([-1.6, 0.02, 0.0])
    z = np.array([0.0, 0.0, 1.0])

    def wing(ang):
        return apex + half * np.array([np.cos(ang), np.sin(ang), 0.0])
    rails = (wing(a), apex, wing(-0.7 * a))
    return np.concatenate([np.stack([r - half * z, r + half * z]) for r in rails])


def ending_blade(half=0.45):
    """a blade that ends inside the body: cells with one or two cut edges (UNHANDLED)"""
    return cr.plane_strip((0.03, -0.02, 0.05), (0.3, 1.0, 0.2), half=half)


def smooth_displacement(v, scale=0.02):
    """a smooth displacement field for the CPU runs (the GPU tests take the displacement of loaded steps instead)"""
    return scale * np.stack([np.sin(2.1 * v[:, 1] + 0.3), np.cos(1.7 * v[:, 2] - 0.2) * v[:, 0], np.sin(1.3 * v[:, 0] * v[:, 1])], axis=1)


def cut_mesh(x, t, delta):
    """the mesh after a cut's delta (meshgen.apply_delta for a delta without elements changed in place)"""
    keep = np.ones(len(t), bool)
    keep[np.asarray(delta["removed"], np.int64)] = False
    return (np.concatenate([np.asarray(x, np.float64).reshape(-1, 3), np.asarray(delta["new_xyz"], np.float64).reshape(-1, 3)]),
            np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32)[keep], np.asarray(delta["added"], np.int32).reshape(-1, 4)])))


# ---- the cases of the GPU file ----
DELAUNAY_CASES = ((1500, 5, 11, 4), (400, 7, 12, 2), (3000, 9, 13, 1))   # (points, mesh seed, plane seed, planes)
FOLD_MESH = (600, 3)
FOLDED_CASES = tuple((nq, fold, 40 + 4 * i + j) for i, nq in enumerate((2, 4, 8)) for j, fold in enumerate((0.05, 0.15, 0.3, 0.5)))
V_CASES = (0.05, 0.2)
UNIT_TET = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
# blades that touch nodes of a 7^3 cube (through its middle node / node plane) and the unhandled cells the restatement counts
TOUCHING_NORMALS = (((1.0, 0.0, 0.0), 156), ((1.0, 0.013, 0.007), 10), ((1.0, 1.0, 0.0), 175), ((1.0, 1.0, 1.0), 116))


def touching_blade(v, normal):
    """a plane through the middle node of a lattice"""
    xs = [np.unique(v[:, k]) for k in range(3)]
    return cr.plane_strip([x[len(x) // 2] for x in xs], normal, half=10.0)
