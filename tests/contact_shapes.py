"""Two-body inputs for fb_fem_body_contact / fb_fem_self_contact away from the lattice: bodies whose faces lie oblique to the grid that
searches them, reentrant edges and a reentrant vertex, faces of mixed and of wildly different size, a body one cell thick, and faces of
zero area.  numpy / scipy only; pinned without a GPU by tests/test_contact_shapes_ref.py, run on the device by
tests/test_contact_shapes_gpu.py.

What the pairs of axis-aligned cubes of bodycontactref.SHAPES cannot reach: a point inside a convex body is never closest to an edge or
a vertex of its boundary, so of closest_on_triangle's seven regions only the interior ever was the answer; and every face of a lattice is
congruent and aligned with the cells of the face grid, so the ring search's pruning (face_search.hip.h) never met an R of several face
sizes, cells of very different counts, a grid one or two cells thick or faces oblique to it.

  rotated       cube(6) 0.1, and a cube(4) 0.1 turned by ROT about its centre, its centre (0.31, 0.05, 0.02) from b's
  notch_vertex  cube(7) 0.1 without the octant above 0.3 on all three axes: a reentrant vertex with three reentrant edges; a, a turned
                cube(4) 0.05, sits across that vertex -- edge and vertex winners
  notch_edge    the same with the notch on x and y only (an L-prism): edge winners
  jittered      meshgen.delaunay_jittered(7, seed=2) and a turned delaunay_jittered(5, seed=1) pushed into its side
  graded_near   Delaunay tetrahedra of 500 points u^3 (u uniform in the unit cube, 150 of them laid on the sides through the origin) and
                the eight corners: R is nine times the median face; a small turned cube in the dense corner
  graded_far    the same b, the same a in the sparse far corner, where each side of the unit cube is two faces: the winners are the
                largest faces and their closest points lie near a corner of them, up to 0.87 R from the centroid the grid binned
  plate         cube(13, 13, 2) 0.05, one cell thick, and a turned cube(3) 0.04 sunk half-way into it
  collapsed     notch_vertex with, in the CURRENT positions of b only, the reentrant vertex's node moved onto its neighbour along a
                reentrant edge: boundary faces of zero area, elements of zero volume

Every case is (rest_a, tets_a, cur_a, rest_b, tets_b, cur_b); a is the small body and pushes into b.  Each is computed once, cached, and
its arrays are read-only.

On the turn.  A winner on an edge shares its closest point with the face across that edge: both are at the same distance and the lower
face wins where the two computed distances are equal bits -- as they are on the lattice's own edges, where both faces form the point
from the same operands.  On the oblique edges that ``collapsed`` makes they may differ in the last place, and then the last place
decides.  Device and reference are the same operations, so they decide alike either way; but ROT's angle is one at which the float64
reference and the same reference in np.longdouble pick the same face for every contact of every case (test_contact_shapes_ref.py), so
that nothing here hangs on a rounding.  At 0.7 radians two contacts of ``collapsed`` did."""
import functools

import numpy as np

import bodycontactref as B
from fembrain_amd.meshgen import delaunay_jittered, truth_cube

CASES = ("rotated", "notch_vertex", "notch_edge", "jittered", "graded_near", "graded_far", "plate", "collapsed")
NOTCH = 0.3            # the notch begins here, from b's lower corner
GRADED_SEED, GRADED_ON_SIDES = 7, 150


def rotation(axis=(0.36, 0.48, 0.8), angle=0.5):
    """Rodrigues' matrix: `angle` radians about `axis` -- a turn that brings no face of a lattice parallel to a coordinate plane"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


ROT = rotation()


def _centre(v):
    return 0.5 * (v.min(axis=0) + v.max(axis=0))


def turned(v, centre, rot=ROT):
    """v turned by rot about the centre of its box, that centre then placed at `centre`"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    return np.ascontiguousarray((v - _centre(v)[None, :]) @ rot.T + np.asarray(centre, np.float64)[None, :])


def without_unused(v, t):
    """the mesh without the nodes no element uses, the others in their old order"""
    used = np.unique(t)
    new = np.full(len(v), -1, np.int64)
    new[used] = np.arange(len(used))
    return np.ascontiguousarray(v[used]), np.ascontiguousarray(new[t].astype(np.int32))


def notched(axes):
    """truth_cube(7, 7, 7, 0.1) without the elements whose centroid lies above NOTCH (from the lower corner) on every axis of `axes`"""
    v, t = truth_cube(7, 7, 7, 0.1)
    c = v[t].mean(axis=1) - v.min(axis=0)[None, :]
    return without_unused(v, t[~(c[:, list(axes)] > NOTCH).all(axis=1)])


def graded(seed=GRADED_SEED):
    """Delaunay tetrahedra of 500 points u^3 (u uniform in the unit cube) plus the eight corners; volumes below 1e-9 dropped, positive
    orientation.  The first GRADED_ON_SIDES points are laid on the three sides through the origin (point i: coordinate i mod 3 set to 0),
    so that the BOUNDARY is graded as the volume is: left inside, the cloud's hull is some forty large faces (R max / median 1.8) and no
    face is small anywhere."""
    from scipy.spatial import Delaunay
    pts = np.random.default_rng(seed).uniform(size=(500, 3)) ** 3
    on = np.arange(GRADED_ON_SIDES)
    pts[on, on % 3] = 0.0
    corners = np.array([[i, j, k] for i in (0.0, 1.0) for j in (0.0, 1.0) for k in (0.0, 1.0)])
    pts = np.concatenate([pts, corners])
    t = Delaunay(pts).simplices.astype(np.int32)
    vol = np.einsum("ij,ij->i", pts[t[:, 1]] - pts[t[:, 0]], np.cross(pts[t[:, 2]] - pts[t[:, 0]], pts[t[:, 3]] - pts[t[:, 0]])) / 6
    keep = np.abs(vol) >= 1e-9
    t, vol = t[keep], vol[keep]
    t[vol < 0] = t[vol < 0][:, [0, 2, 1, 3]]
    return without_unused(pts, t)


def _build(name):
    if name == "rotated":
        vb, tb = truth_cube(6, 6, 6, 0.1)
        va, ta = truth_cube(4, 4, 4, 0.1)
        return va, ta, turned(va, _centre(vb) + (0.31, 0.05, 0.02)), vb, tb, vb
    if name in ("notch_vertex", "notch_edge", "collapsed"):
        vb, tb = notched((0, 1, 2) if name != "notch_edge" else (0, 1))
        va, ta = truth_cube(4, 4, 4, 0.05)
        cur_b = vb
        if name == "collapsed":
            lo = vb.min(axis=0)
            corner = np.nonzero(np.abs(vb - (lo + NOTCH)[None, :]).max(axis=1) < 1e-9)[0]
            onto = np.nonzero(np.abs(vb - (lo + (NOTCH, NOTCH, NOTCH + 0.1))[None, :]).max(axis=1) < 1e-9)[0]
            assert len(corner) == 1 and len(onto) == 1
            cur_b = vb.copy()
            cur_b[corner[0]] = vb[onto[0]]
        return va, ta, turned(va, vb.min(axis=0) + (0.27, 0.26, 0.25)), vb, tb, cur_b
    if name == "jittered":
        vb, tb, _ = delaunay_jittered(7, seed=2)
        va, ta, _ = delaunay_jittered(5, seed=1)
        return va, ta, turned(va, _centre(vb) + (0.33, 0.04, -0.03)), vb, tb, vb
    if name in ("graded_near", "graded_far"):
        vb, tb = graded()
        va, ta = truth_cube(4, 4, 4, 0.02)
        return va, ta, turned(va, (0.034, 0.041, 0.037) if name == "graded_near" else (0.94, 0.93, 0.92)), vb, tb, vb
    if name == "plate":
        vb, tb = truth_cube(13, 13, 2, 0.05)
        va, ta = truth_cube(3, 3, 3, 0.04)
        return va, ta, turned(va, _centre(vb) + (0.113, -0.071, 0.025)), vb, tb, vb
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """(rest_a, tets_a, cur_a, rest_b, tets_b, cur_b) of a case of CASES: built once, read-only"""
    ra, ta, ca, rb, tb, cb = _build(name)
    # a handle holds rest and q = cur - rest and forms rest + q: the case's current positions are those, to the bit
    ca, cb = ra + (ca - ra), rb + (cb - rb)
    assert np.array_equal(ra + (ca - ra), ca) and np.array_equal(rb + (cb - rb), cb)
    out = []
    for x, dtype, width in ((ra, np.float64, 3), (ta, np.int32, 4), (ca, np.float64, 3), (rb, np.float64, 3), (tb, np.int32, 4), (cb, np.float64, 3)):
        x = np.array(x, dtype).reshape(-1, width)
        x.flags.writeable = False
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def union(name):
    """a and b of a case as ONE mesh, a's nodes and elements first (as selfcontactref.union): (rest, tets, cur, n_nodes_a, n_tets_a)"""
    ra, ta, ca, rb, tb, cb = case(name)
    out = [np.concatenate([ra, rb]), np.concatenate([ta, tb + len(ra)]).astype(np.int32), np.concatenate([ca, cb])]
    for x in out:
        x.flags.writeable = False
    return out[0], out[1], out[2], len(ra), len(ta)


@functools.lru_cache(maxsize=None)
def reference(name, stiffness=1000.0, longdouble=False):
    """bodycontactref.body_contact of a case with ``extent`` as the tests' _reference adds it: computed once, never changed"""
    ra, ta, ca, rb, tb, cb = case(name)
    ref = B.body_contact(ra, ta, ca, rb, tb, cb, stiffness, dtype=np.longdouble if longdouble else np.float64)
    ref["extent"] = (float((cb.max(axis=0) - cb.min(axis=0)).max()), float((ca.max(axis=0) - ca.min(axis=0)).max()))
    return ref


# ---- what the census counts ----

def regions(bary):
    """(interior, edge, vertex) winners among the weight triples bary (k, 3), by the number of weights that are exactly zero: none, one,
    two.  The vertex returns and the edges AB and AC write their zeros as constants; on the edge BC the first weight is (1 - (1 - w)) - w,
    which is zero only where 1 - w is formed without a rounding -- such a winner counts as interior where it is not.  Device and reference
    form the same weights, so the counts are compared, not interpreted."""
    zeros = (np.asarray(bary).reshape(-1, 3) == 0).sum(axis=1)
    return int((zeros == 0).sum()), int((zeros == 1).sum()), int((zeros >= 2).sum())


def face_radii(cur, faces):
    """per boundary face the largest centroid-to-vertex distance at the positions cur: the ring search's R is their maximum"""
    tri = np.asarray(cur, np.float64)[np.asarray(faces, np.int64)]
    return np.linalg.norm(tri - tri.mean(axis=1, keepdims=True), axis=2).max(axis=1)


def share_of_R_needed(cur_p, d, cur_t, faces):
    """per contact of the direction d (of bodycontactref.direction) (|g - p| - depth) / R, g the winner's centroid: the share of R that
    the ring search's D = best_d + R must keep for the winner's cell to be visited at all (the cell it adds on every side aside).  Near
    0 the winner would be found with any R; near 1 the coverage argument of face_search.hip.h is used in full."""
    cur_t, faces = np.asarray(cur_t, np.float64), np.asarray(faces, np.int64)
    g = cur_t[faces[d["face"]]].mean(axis=1)
    return (np.linalg.norm(g - np.asarray(cur_p, np.float64)[d["node"]], axis=1) - np.asarray(d["depth"], np.float64)) / face_radii(cur_t, faces).max()


def zero_area_faces(cur, faces):
    """the boundary faces whose area at the positions cur is exactly zero"""
    tri = np.asarray(cur, np.float64)[np.asarray(faces, np.int64)]
    return np.nonzero((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) == 0).all(axis=1))[0]


def left_out(r, extent):
    """how many candidates of a direction bodycontactref.generic leaves out (as the GPU tests' _compare counts them)"""
    cand_ok, contact_ok = B.generic(r, extent)
    return int((~cand_ok).sum()) + int((~contact_ok & cand_ok[r["in_contact"]]).sum())


def overlap_cells_spanned(cur_p, vids_p, cur_t, tets_t, nudge=0.0):
    """The containment grid of one direction of fb_fem_body_contact restated on the host (body_contact.hip run_direction, face_search.hip.h
    make_grid): the elements of T whose padded box meets the overlap O of P's surface box and T's node box are binned into a grid of about
    one cell per such element over O.  Returns (n_tets,) the cells each element's padded box overlaps, clamped into the grid; 0 for an
    element that does not meet O.  Above 64 (kEmbedWideCells) an element is not walked cell by cell but goes to the overflow list.
    nudge: added to every cell coordinate before it is floored, in cells -- what a rule that rounds otherwise than this one could give."""
    cur_p, cur_t, tets_t = np.asarray(cur_p, np.float64), np.asarray(cur_t, np.float64), np.asarray(tets_t, np.int64)
    pts = cur_p[np.asarray(vids_p, np.int64)]
    tlo, thi = cur_t.min(axis=0), cur_t.max(axis=0)
    olo, ohi = np.maximum(pts.min(axis=0), tlo), np.minimum(pts.max(axis=0), thi)
    pad = float(np.ldexp((thi - tlo).max(), -30))
    v = cur_t[tets_t]
    a, b = v.min(axis=1) - pad, v.max(axis=1) + pad
    meets = ((a <= ohi[None, :]) & (b >= olo[None, :])).all(axis=1)
    m = int(meets.sum())
    lo, hi = olo - pad, ohi + pad
    ext = hi - lo
    hcell = float(np.cbrt(ext.prod() / max(m, 1)))
    dim = [int(min(1024, max(1, np.ceil(e / hcell)))) if hcell > 0 else 1 for e in ext]
    while dim[0] * dim[1] * dim[2] > max(64, 8 * m):
        k = 0 if dim[0] >= dim[1] and dim[0] >= dim[2] else 1 if dim[1] >= dim[2] else 2
        dim[k] = (dim[k] + 1) // 2
    dim = np.array(dim, np.int64)
    inv = dim / ext
    c0 = np.clip(np.floor((a - lo) * inv - nudge), 0, dim - 1)
    c1 = np.clip(np.floor((b - lo) * inv + nudge), 0, dim - 1)
    return np.where(meets, np.prod(np.maximum(c1 - c0, 0) + 1, axis=1), 0).astype(np.int64)
