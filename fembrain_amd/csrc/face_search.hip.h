// What the two contact units (body_contact.hip, self_contact.hip) share of the search for the closest boundary face, each written once:
// the positions pass, the closest point of a triangle, the grid rule, the grid of face centroids and its build, what a search knows of
// its points, the two searches (k_face_scan, k_face_ring) over the faces a point may take, the record a search leaves (bc_finish), and
// the host's side of all that.  The force stage that follows a search is contact_force.hip.h.
// The units are built with -ffp-contract=off: one function is one sequence of roundings wherever it is called.
//
// The closest face, one wavefront per contact (k_face_ring).  The faces of the searched body T are binned by CENTROID into a grid over
// T's current box; their nine current coordinates are stored grouped by cell, faces ascending inside a cell, a plane per coordinate, so a
// run of cells along x is one contiguous range that the lanes stride over with coalesced loads.  Each lane keeps its minimum under the
// key (d, face) and wf_best folds them whenever a lane has improved.  R is the largest centroid-to-vertex distance over all faces, folded
// once per build and widened by 2^-40.
//  1. Shells of cells around the point's cell until one holds a face, then one more: a candidate (best_d, best_f).  At most kShells
//     shells: a point deeper inside takes the bound of the box instead, best_d = m (1 + 2^-40) with m its least distance to a side of the
//     grid's box along an axis and no face attached.  (A point inside the body leaves the body no later than the box on its way along an
//     axis, and where it leaves lies a boundary face: a face within m exists.  Nothing rests on that: see the last point below.)
//  2. Every cell the box [p - D, p + D] overlaps, D = (best_d + R) (1 + 2^-40), widened by one cell on every side, layer by layer and in a
//     layer 64 rows at a time -- a lane per row forms the x-range that is left of D after the row's distance in y and z, the wavefront
//     walks the rows that hold a face.  best_d tightens as it goes; a row's range formed under an earlier, larger best_d is a superset.
// Why no face outside the visited cells can have a distance <= best_d:
//  - Let f be a face whose COMPUTED distance d(p, f) is <= best_d.  Its computed closest point c lies, up to a few roundings of a
//    coordinate, in the triangle, and a triangle lies within the largest centroid-to-vertex distance of its centroid (the distance from a
//    point is convex, so its maximum over the triangle is at a vertex): |c - g| <= R for the centroid g as the grid binned it, the
//    roundings covered by R's widening.  The exact |c - p| is at most d (1 + 2^-50).  So |g - p| <= best_d + R < D, and so is each of
//    |g_x - p_x|, |g_y - p_y|, |g_z - p_z|.
//  - From here on the argument is embed_closest.hip's with g in the place of the centre: cell_clamped is monotone, so from g_k >= p_k - D
//    follows cell(g_k) >= cell(p_k - D) wherever p_k - D is formed exactly; its one rounding, relative to a coordinate of the box, is
//    below 2^-13 of a cell (embed_ring_covers has checked it: a body it does not cover scans), and a whole cell on either side covers
//    that.  A centroid whose computed cell on the axis y is j lies in the slab of j widened by 2^-10 of a cell (slab_gap), the first and
//    the last cell of an axis are taken as unbounded outward, so the clamps need no argument; a row with g_y^2 + g_z^2 > D^2 (1 + 2^-40)
//    holds no such centroid, and in any other row g lies in the x-range of the root of the difference.
//  - Tightening best_d only removes faces that could no longer win under (d, face): a face with d == best_d and a lower index is still
//    inside, because every comparison above is <=.
//  - The argument needs best_d to be an upper bound of the answer's distance at every moment.  A best_d with a face attached is one.  The
//    bound of the box is one whenever some face has a computed distance <= it; the search then ends with that face or a better one, found
//    in cells the argument covers.  If no face has -- a boundary that is not closed, a rounding at the box's side -- the search ends
//    without a face, and such a point is flagged and scanned like one past its budget.
// Every loop is bounded by numbers the host knows: the shells by the largest dim, the rows by dim[1] dim[2], a row by the face count; a
// point that has tested more than `budget` faces stops, is flagged, and k_face_scan -- every face for the flagged points, the whole path
// for a body the proof does not cover, and the test twin -- finds the same (d, face): closest_on_triangle and centre_distance are one
// sequence of roundings on the same operands, and (d, face) is a total order.  The winner's closest point and weights are formed again
// from the face itself by bc_finish, for both paths alike.  Nothing spins.
//
// The searches are written over an exclusion: what a point may not take.  Two bodies exclude nothing (NoExclusion: the test and the vote
// below are compiled out); a body against itself excludes by node or by part (FaceExclusion).  The coverage argument above shows that no
// face OUTSIDE the visited cells has a computed distance <= best_d.  Skipping faces inside visited cells removes candidates and touches
// none of its steps.  What changes under an exclusion is where best_d comes from:
//  - the shells look for their first candidate among the faces the point may take (a range "holds a face" only if it holds such a one,
//    a vote of the lanes): a surface vertex's own cell is full of its own faces, and stopping at them would leave the second phase
//    without a bound;
//  - the bound of the box, m, no longer implies that a face the point MAY TAKE lies within m -- the face where the point leaves the body
//    may be its own.  Nothing rested on that implication before and nothing does now: a search that ends without a face is flagged and
//    k_face_scan decides, as for a point past its budget.  A contact for which the scan finds no face either has none left, and
//    self_contact.hip drops it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include "body_contact.h"
#include "device_prims.hip.h"
#include "embed_grid.hip.h"
#include "launch.hip.h"
#include "plan_device.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

__device__ __forceinline__ double dot3(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// The closest point of the triangle (a, b, c) to p (Ericson 5.1.5), and its weights v on b and w on c.  The regions in the book's order:
// vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, interior.
__device__ __forceinline__ void closest_on_triangle(const double* p, const double* a, const double* b, const double* c, double* out, double* v_out, double* w_out) {
  const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]}, ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  if (d1 <= 0.0 && d2 <= 0.0) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; *v_out = 0.0; *w_out = 0.0; return; }
  const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
  const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; *v_out = 1.0; *w_out = 0.0; return; }
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double v = d1 / (d1 - d3);
    out[0] = a[0] + v * ab[0]; out[1] = a[1] + v * ab[1]; out[2] = a[2] + v * ab[2];
    *v_out = v; *w_out = 0.0;
    return;
  }
  const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; *v_out = 0.0; *w_out = 1.0; return; }
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double w = d2 / (d2 - d6);
    out[0] = a[0] + w * ac[0]; out[1] = a[1] + w * ac[1]; out[2] = a[2] + w * ac[2];
    *v_out = 0.0; *w_out = w;
    return;
  }
  const double va = d3 * d6 - d5 * d4;
  if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
    const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    out[0] = b[0] + w * (c[0] - b[0]); out[1] = b[1] + w * (c[1] - b[1]); out[2] = b[2] + w * (c[2] - b[2]);
    *v_out = 1.0 - w; *w_out = w;
    return;
  }
  const double denom = 1.0 / ((va + vb) + vc);
  const double v = vb * denom, w = vc * denom;
  out[0] = (a[0] + ab[0] * v) + ac[0] * w; out[1] = (a[1] + ab[1] * v) + ac[1] * w; out[2] = (a[2] + ab[2] * v) + ac[2] * w;
  *v_out = v; *w_out = w;
}

// the distance of p from the triangle: what both searches compare
__device__ __forceinline__ double triangle_distance(const double* p, const double* a, const double* b, const double* c) {
  double q[3], v, w;
  closest_on_triangle(p, a, b, c, q, &v, &w);
  return centre_distance(p, q);
}

__device__ __forceinline__ double wg_max_double(double v) {
  static_assert(kWaves == 4, "written for four wavefronts");
  v = wf_max(v);
  __shared__ double sh[kWaves];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
  __syncthreads();
  return r;
}

// ---- positions ----

// A thread per node (internal order): x0 + q, and the workgroup's box of them; a value that is not finite makes the box infinite
__global__ __launch_bounds__(kB) void k_contact_positions(int n_nodes, const double* __restrict__ x0, const double* __restrict__ q, double* __restrict__ cur,
                                                          double* __restrict__ part) {
  const int i = blockIdx.x * kB + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n_nodes) {
    const size_t b = 3 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double v = x0[b + k] + q[b + k];
      cur[b + k] = v;
      const bool ok = fabs(v) <= DBL_MAX;  // (false for a NaN, which fmin / fmax would have passed over)
      lo[k] = ok ? v : -INFINITY;
      hi[k] = ok ? v : INFINITY;
    }
  }
  wg_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

// ---- the face grid ----

__device__ __forceinline__ void load_face(const int* __restrict__ faces_int, int n_nodes, const double* __restrict__ cur, int f, double (*v)[3]) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int nd = faces_int[3 * (size_t)f + k];
    if ((unsigned)nd >= (unsigned)n_nodes) nd = 0;
    const double* p = cur + 3 * (size_t)nd;
    v[k][0] = p[0]; v[k][1] = p[1]; v[k][2] = p[2];
  }
}

// A thread per face: (cell of its centroid, face), the cell's count, and the workgroup's largest centroid-to-vertex distance
__global__ __launch_bounds__(kB) void k_bc_face_keys(int nf, const int* __restrict__ faces_int, int n_nodes, const double* __restrict__ cur, GridDev g, uint32_t* __restrict__ keys,
                                                     uint32_t* __restrict__ vals, int* __restrict__ cnt, double* __restrict__ r_part) {
  const int f = blockIdx.x * kB + threadIdx.x;
  double r = 0.0;
  if (f < nf) {
    double v[3][3], c[3];
    load_face(faces_int, n_nodes, cur, f, v);
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = ((v[0][k] + v[1][k]) + v[2][k]) * (1.0 / 3);
    r = fmax(fmax(centre_distance(c, v[0]), centre_distance(c, v[1])), centre_distance(c, v[2]));
    if (!(r >= 0.0)) r = INFINITY;  // (a coordinate that is not a number: every search of this body widens to the whole grid)
    const int cell = (cell_clamped(g, 2, c[2]) * g.dim[1] + cell_clamped(g, 1, c[1])) * g.dim[0] + cell_clamped(g, 0, c[0]);
    keys[f] = (uint32_t)cell;
    vals[f] = (uint32_t)f;
    atomicAdd(cnt + cell, 1);
  }
  r = wg_max_double(r);
  if (threadIdx.x == 0) r_part[blockIdx.x] = r;
}

// one workgroup: R, widened
__global__ __launch_bounds__(kB) void k_bc_R_final(int n_part, const double* __restrict__ r_part, double* __restrict__ out) {
  double r = 0.0;
  for (int b = threadIdx.x; b < n_part; b += kB) r = fmax(r, r_part[b]);
  r = wg_max_double(r);
  if (threadIdx.x == 0) *out = r * kRingGrow;
}

// A thread per sorted entry: the nine coordinates of its face, a plane each
__global__ __launch_bounds__(kB) void k_bc_face_store(int nf, const int* __restrict__ f_face, const int* __restrict__ faces_int, int n_nodes, const double* __restrict__ cur,
                                                      double* __restrict__ tri) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= nf) return;
  int f = f_face[j];
  if ((unsigned)f >= (unsigned)nf) f = 0;
  double v[3][3];
  load_face(faces_int, n_nodes, cur, f, v);
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int c = 0; c < 3; c++) tri[(size_t)(3 * k + c) * nf + j] = v[k][c];
}

// ---- the closest face ----

// what a search knows of its points and of the body it searches
struct SearchDev {
  int n_contacts;
  const int *hit, *cand, *vnode, *vertex_ids, *c_elem;  // contact -> candidate -> surface vertex of P -> node; the containing element
  int n_cand, nv, n_nodes_p;
  const double* cur_p;
  int nf, n_nodes_t;
  const int* faces_int;
  const double* cur_t;
};
struct FaceDev {
  const int *cell_start, *face;
  const double *tri, *R;
};
constexpr int kShells = 2;  // shells of the ring search's first phase (a resting contact is a fraction of a cell deep)

// the point of contact t, its surface vertex (-1: an index out of range)
__device__ __forceinline__ int contact_point(const SearchDev& S, int t, double* p) {
  const int h = S.hit[t];
  const int vr = (unsigned)h < (unsigned)S.n_cand ? S.cand[h] : -1;
  const int nd = (unsigned)vr < (unsigned)S.nv ? S.vnode[vr] : -1;
  if ((unsigned)nd >= (unsigned)S.n_nodes_p) return -1;
  p[0] = S.cur_p[3 * (size_t)nd]; p[1] = S.cur_p[3 * (size_t)nd + 1]; p[2] = S.cur_p[3 * (size_t)nd + 2];
  return vr;
}

// One lane: the record of contact t from the winning face, formed again from the face itself
__device__ __forceinline__ void bc_finish(const SearchDev& S, int t, int vr, const double* p, int bf, long long tested, bool add_tested, BodyContactRec* __restrict__ rec) {
  BodyContactRec r;
  r.c[0] = r.c[1] = r.c[2] = 0.0; r.b[0] = r.b[1] = r.b[2] = 0.0; r.d = 0.0; r.f[0] = r.f[1] = r.f[2] = 0.0;
  r.tested = add_tested ? rec[t].tested + tested : tested;
  r.node = vr >= 0 ? S.vertex_ids[vr] : -1;
  r.elem = vr >= 0 ? S.c_elem[S.hit[t]] : -1;
  r.face = -1;
  r.far = 0;
  if (vr >= 0 && (unsigned)bf < (unsigned)S.nf) {
    double v[3][3], bv, bw;
    load_face(S.faces_int, S.n_nodes_t, S.cur_t, bf, v);
    closest_on_triangle(p, v[0], v[1], v[2], r.c, &bv, &bw);
    r.d = centre_distance(p, r.c);
    r.b[0] = (1.0 - bv) - bw; r.b[1] = bv; r.b[2] = bw;
    r.face = bf;
  }
  rec[t] = r;
}

// What a point may not take.  Two bodies: nothing
struct NoExclusion {
  static constexpr bool kExcludes = false;
  __device__ __forceinline__ constexpr int key_of(int) const { return 0; }
  __device__ __forceinline__ constexpr bool operator()(int, int) const { return false; }
};
// A body against itself: the faces of the point's own node (FB_SELF_CONTACT_ANY) or part (FB_SELF_CONTACT_OTHER_PARTS)
struct FaceExclusion {
  static constexpr bool kExcludes = true;
  int mode, nf;
  const int *faces_int, *face_part;  // [3 faces] internal nodes | [faces] OTHER_PARTS: the part of the face's element
  const int* p_key;                  // [surface vertices]
  __device__ __forceinline__ int key_of(int vr) const { return vr >= 0 ? p_key[vr] : -1; }
  __device__ __forceinline__ bool operator()(int key, int f) const {
    if ((unsigned)f >= (unsigned)nf) return true;
    if (mode == FB_SELF_CONTACT_OTHER_PARTS) return face_part[f] == key;
    const size_t b = 3 * (size_t)f;
    return faces_int[b] == key || faces_int[b + 1] == key || faces_int[b + 2] == key;
  }
};

// One wavefront per contact, every face of T in its own order, lanes striding.  only_far: the points the ring search flagged, the others
// keep their records.
template <class Ex>
__global__ __launch_bounds__(kB) void k_face_scan(SearchDev S, Ex ex, int only_far, BodyContactRec* __restrict__ rec) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = blockIdx.x * kWaves + wave;
  if (t >= S.n_contacts) return;
  if (only_far && rec[t].far == 0) return;  // (the same in every lane)
  double p[3] = {0.0, 0.0, 0.0};
  const int vr = contact_point(S, t, p);
  const int key = ex.key_of(vr);
  double bd = DBL_MAX;
  int bf = INT_MAX;
  if (vr >= 0)
    for (int f = lane; f < S.nf; f += 64) {
      if (ex(key, f)) continue;
      double v[3][3];
      load_face(S.faces_int, S.n_nodes_t, S.cur_t, f, v);
      const double d = triangle_distance(p, v[0], v[1], v[2]);
      if (d < DBL_MAX && Lowest()(d, f, bd, bf)) { bd = d; bf = f; }
    }
  wf_best<int, Lowest>(bd, bf);
  if (lane == 0) bc_finish(S, t, vr, p, bf, (long long)S.nf, only_far != 0, rec);
}

// One wavefront per contact through the face grid.  Everything that decides a branch is the same in every lane: the ranges come from
// cell_start, the best pair is folded over the wavefront whenever a lane has improved it, and whether a range held a face the point
// may take is a vote of the lanes (without an exclusion: whether the range is not empty, no vote).
template <class Ex>
__global__ __launch_bounds__(kB) void k_face_ring(SearchDev S, Ex ex, GridDev g, FaceDev fg, long long budget, BodyContactRec* __restrict__ rec) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = blockIdx.x * kWaves + wave;
  if (t >= S.n_contacts) return;
  double p[3] = {0.0, 0.0, 0.0};
  const int vr = contact_point(S, t, p);
  const int key = ex.key_of(vr);
  long long tested = 0;
  bool far = false;
  double bd = DBL_MAX;
  int bf = INT_MAX;
  if (vr >= 0) {
    const double R = *fg.R;
    const size_t nf = (size_t)S.nf;
    // the range [j0, j1) of the sorted faces (a run of cells along x): every lane its share, the best pair folded; true where the range
    // held a face the point may take
    auto scan_range = [&](int j0, int j1) {
      bool improved = false, seen = false;
      for (int j = j0 + lane; j < j1; j += 64) {
        const int f = fg.face[j];
        if (ex(key, f)) continue;  // (one gather ahead of the nine coordinates, which an excluded face does not load)
        seen = true;
        const double a[3] = {fg.tri[j], fg.tri[nf + j], fg.tri[2 * nf + j]}, b[3] = {fg.tri[3 * nf + j], fg.tri[4 * nf + j], fg.tri[5 * nf + j]},
                     c[3] = {fg.tri[6 * nf + j], fg.tri[7 * nf + j], fg.tri[8 * nf + j]};
        const double d = triangle_distance(p, a, b, c);
        if (d < DBL_MAX && Lowest()(d, f, bd, bf)) { bd = d; bf = f; improved = true; }
      }
      if (__any(improved)) wf_best<int, Lowest>(bd, bf);
      if (j1 > j0) tested += j1 - j0;
      if (tested > budget) far = true;
      if constexpr (Ex::kExcludes) return __any(seen) != 0;
      return j1 > j0;
    };
    // ... of the cells x0c .. x1c of the row that begins at cell `row`
    auto scan_cells = [&](int row, int x0c, int x1c) { return scan_range(max(fg.cell_start[row + x0c], 0), min(fg.cell_start[row + x1c + 1], S.nf)); };
    int pc[3], rmax = 0;
    double to_box = DBL_MAX;  // the least distance from p to a side of the grid's box along an axis
#pragma unroll
    for (int k = 0; k < 3; k++) {
      pc[k] = cell_clamped(g, k, p[k]);
      rmax = max(rmax, max(pc[k], g.dim[k] - 1 - pc[k]));
      to_box = fmin(to_box, fmin(p[k] - g.lo[k], g.hi[k] - p[k]));
    }
    // 1. shells until one holds a face the point may take, and the one after it; no further than kShells, behind which the bound of the
    // box stands in
    int stop = -1;
    for (int r = 0; r <= min(rmax, kShells) && !far; r++) {
      bool got = false;
      const int z1 = min(pc[2] + r, g.dim[2] - 1), y1 = min(pc[1] + r, g.dim[1] - 1), xa = pc[0] - r, xb = pc[0] + r;
      for (int z = max(pc[2] - r, 0); z <= z1 && !far; z++)
        for (int y = max(pc[1] - r, 0); y <= y1 && !far; y++) {
          const int row = (z * g.dim[1] + y) * g.dim[0];
          if (z == pc[2] - r || z == pc[2] + r || y == pc[1] - r || y == pc[1] + r) {  // a row of the shell's faces: all of it
            got |= scan_cells(row, max(xa, 0), min(xb, g.dim[0] - 1));
          } else {  // its two ends
            if (xa >= 0) got |= scan_cells(row, xa, xa);
            if (xb < g.dim[0] && !far) got |= scan_cells(row, xb, xb);
          }
        }
      if (got && stop < 0) stop = r + 1;
      if (r == stop) break;
    }
    if (bf == INT_MAX && to_box >= 0.0 && to_box < DBL_MAX) bd = to_box * kRingGrow;  // (no face attached: any face at a distance <= bd takes its place)
    // 2. every cell that could hold the centroid of a face at a distance <= best_d
    if (!far) {
      const double D0 = (bd + R) * kRingGrow;
      const bool none = !(D0 < DBL_MAX);  // (no bound below DBL_MAX, or an R that is not finite: the whole grid)
      const double h[3] = {1.0 / g.inv[0], 1.0 / g.inv[1], 1.0 / g.inv[2]};
      const int z0 = none ? 0 : max(cell_clamped(g, 2, p[2] - D0) - 1, 0), z1 = none ? g.dim[2] - 1 : min(cell_clamped(g, 2, p[2] + D0) + 1, g.dim[2] - 1);
      const int y0 = none ? 0 : max(cell_clamped(g, 1, p[1] - D0) - 1, 0), y1 = none ? g.dim[1] - 1 : min(cell_clamped(g, 1, p[1] + D0) + 1, g.dim[1] - 1);
      for (int z = z0; z <= z1 && !far; z++) {
        const double gz = slab_gap(g, 2, z, h[2], p[2]);
        int ya = y0, yb = y1;  // the rows of this layer that are left of D after its distance in z: the x-range's argument with g_y = 0
        {
          const double D = (bd + R) * kRingGrow, D2 = D * D * kRingGrow;
          if (D2 < DBL_MAX) {
            if (gz * gz > D2) continue;
            const double rem = sqrt(D2 - gz * gz) * kRingGrow;
            ya = max(y0, cell_clamped(g, 1, p[1] - rem) - 1);
            yb = min(y1, cell_clamped(g, 1, p[1] + rem) + 1);
          }
        }
        // 64 rows at a time: a lane per row forms the row's range under the best_d of this moment (a tighter one later in the batch would
        // only have shortened it), and the wavefront walks the rows that hold a face -- deep inside a body most rows hold none
        for (int yc = ya; yc <= yb && !far; yc += 64) {
          const int y = yc + lane;
          int j0 = 0, j1 = 0;
          if (y <= yb) {
            int xa = 0, xb = g.dim[0] - 1;
            bool skip = false;
            const double D = (bd + R) * kRingGrow, D2 = D * D * kRingGrow;
            if (D2 < DBL_MAX) {  // (else the square is out of range: the whole row)
              const double gy = slab_gap(g, 1, y, h[1], p[1]);
              const double g2 = gy * gy + gz * gz;
              if (g2 > D2) {
                skip = true;
              } else {
                const double rem = sqrt(D2 - g2) * kRingGrow;
                xa = max(cell_clamped(g, 0, p[0] - rem) - 1, 0);
                xb = min(cell_clamped(g, 0, p[0] + rem) + 1, g.dim[0] - 1);
              }
            }
            if (!skip) {
              const int row = (z * g.dim[1] + y) * g.dim[0];
              j0 = max(fg.cell_start[row + xa], 0);
              j1 = min(fg.cell_start[row + xb + 1], S.nf);
            }
          }
          unsigned long long rows = __ballot(j1 > j0);
          while (rows != 0ull && !far) {
            const int l = __ffsll((long long)rows) - 1;
            rows &= rows - 1ull;
            scan_range(__shfl(j0, l), __shfl(j1, l));
          }
        }
      }
    }
    if (bf == INT_MAX) far = true;  // (no face the point may take within the bound -- a boundary that is not closed, a rounding at the box's side: the scan decides)
  }
  if (lane == 0) {
    bc_finish(S, t, vr, p, far ? INT_MAX : bf, tested, false, rec);
    if (far) rec[t].far = 1;
  }
}

// ---- host ----

// the stages of fb_fem_time_*_contact: events around each, on the calling handle's stream
struct Stages {
  hipEvent_t* ev = nullptr;
  hipStream_t s = nullptr;
  double* seconds = nullptr;  // null: not timing
  int begin() {
    if (seconds) FB_HIP(hipEventRecord(ev[0], s));
    return FB_OK;
  }
  int end(int stage) {
    if (!seconds) return FB_OK;
    FB_HIP(hipEventRecord(ev[1], s));
    FB_HIP(hipEventSynchronize(ev[1]));
    float ms = 0;
    FB_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    seconds[stage] += ms * 1e-3;
    return FB_OK;
  }
};
int stage_events(FaceSearchWork& F) {
  for (auto& e : F.ev_t)
    if (!e) FB_HIP(hipEventCreate(&e));
  return FB_OK;
}

// FEMBRAIN_BODY_CONTACT / FEMBRAIN_SELF_CONTACT, read at every call: FB_BODY_CONTACT_SCAN / _RING, 0 where it is not set
int path_knob(const char* env_name) {
  const char* env = getenv(env_name);
  if (!env || !*env) return FB_BODY_CONTACT_NONE;
  if (!strcmp(env, "scan")) return FB_BODY_CONTACT_SCAN;
  if (!strcmp(env, "ring")) return FB_BODY_CONTACT_RING;
  return FB_BODY_CONTACT_NONE;
}

// FEMBRAIN_*_CONTACT_BUDGET: the faces one point may test on the ring path (default: a point that has tested as many faces as a scan
// tests gains nothing from going on)
long long budget_knob(const char* env_name, long long nf) {
  const char* env = getenv(env_name);
  return env && *env ? std::max(0LL, atoll(env)) : nf;
}

// a grid of the order of one cell per item over the box [lo - pad, hi + pad] (embed_grid_build's rule)
GridDev make_grid(const double* lo, const double* hi, double pad, long long n_items) {
  GridDev g;
  memset(&g, 0, sizeof(g));
  double ext[3], vol = 1.0;
  for (int k = 0; k < 3; k++) {
    g.lo[k] = lo[k] - pad; g.hi[k] = hi[k] + pad;
    ext[k] = g.hi[k] - g.lo[k];
    vol *= ext[k];
  }
  g.pad = pad;
  const double hcell = std::cbrt(vol / (double)std::max<long long>(n_items, 1));
  long long cells = 1;
  for (int k = 0; k < 3; k++) {
    const double d = hcell > 0.0 ? std::ceil(ext[k] / hcell) : 1.0;
    g.dim[k] = d >= 1024.0 ? 1024 : d >= 1.0 ? (int)d : 1;
    cells *= g.dim[k];
  }
  const long long cell_cap = std::max<long long>(64, 8LL * n_items);
  while (cells > cell_cap) {
    const int k = g.dim[0] >= g.dim[1] && g.dim[0] >= g.dim[2] ? 0 : g.dim[1] >= g.dim[2] ? 1 : 2;
    g.dim[k] = (g.dim[k] + 1) / 2;
    cells = (long long)g.dim[0] * g.dim[1] * g.dim[2];
  }
  for (int k = 0; k < 3; k++) g.inv[k] = g.dim[k] / ext[k];
  return g;
}

bool grid_covered(const GridDev& g) {
  EmbedGrid G;
  for (int k = 0; k < 3; k++) { G.lo[k] = g.lo[k]; G.hi[k] = g.hi[k]; G.dim[k] = g.dim[k]; }
  return embed_ring_covers(G);
}

// The face grid of a body over fgrid: its faces sorted by the cell of their centroid, their coordinates in that order, R
int build_face_grid(hipStream_t s, PlanWorkspace& ws, FaceSearchWork& F, const int* faces_int, int nf, int n_nodes, const double* cur, const GridDev& fgrid) {
  const int n_cells = fgrid.dim[0] * fgrid.dim[1] * fgrid.dim[2], nbf = blocks_for(nf);
  FB_TRY(F.f_cnt.reserve((size_t)n_cells + 1)); FB_TRY(F.f_start.reserve((size_t)n_cells + 1)); FB_TRY(F.f_face.reserve((size_t)nf));
  FB_TRY(F.f_tri.reserve((size_t)9 * nf)); FB_TRY(F.f_R.reserve((size_t)nbf + 1));
  FB_HIP(hipMemsetAsync(F.f_cnt.p, 0, sizeof(int) * ((size_t)n_cells + 1), s));
  FB_TRY(ws.keys.reserve(((size_t)nf + 1) / 2)); FB_TRY(ws.keys_s.reserve(((size_t)nf + 1) / 2)); FB_TRY(ws.vals.reserve((size_t)nf));
  uint32_t* ck = reinterpret_cast<uint32_t*>(ws.keys.p);
  uint32_t* ck_s = reinterpret_cast<uint32_t*>(ws.keys_s.p);
  FB_TRY(launch_1d(k_bc_face_keys, nf, s, nf, faces_int, n_nodes, cur, fgrid, ck, ws.vals.p, F.f_cnt.p, F.f_R.p));
  FB_TRY(launch_grid(k_bc_R_final, dim3(1), s, nbf, F.f_R.p, F.f_R.p + nbf));
  FB_TRY(sort_pairs(ws.temp, s, ck, ck_s, ws.vals.p, reinterpret_cast<uint32_t*>(F.f_face.p), (size_t)nf, (unsigned)bits_of(n_cells)));
  FB_TRY(exclusive_scan(ws.temp, s, F.f_cnt.p, F.f_start.p, 0, (size_t)n_cells + 1));
  FB_TRY(launch_1d(k_bc_face_store, nf, s, nf, F.f_face.p, faces_int, n_nodes, cur, F.f_tri.p));
  return FB_OK;
}

// The closest faces of S's contacts into F.rec: through the grid build_face_grid left, then every face for the points the ring gave up
// (past their budget or without a face; a wavefront of any other returns at once) -- or every face for every point
template <class Ex>
int search_faces(hipStream_t s, FaceSearchWork& F, const SearchDev& S, const Ex& ex, bool ring, const GridDev& fgrid, long long budget) {
  FB_TRY(F.rec.reserve((size_t)S.n_contacts));
  if (ring) {
    const FaceDev fg = {F.f_start.p, F.f_face.p, F.f_tri.p, F.f_R.p + blocks_for(S.nf)};
    FB_TRY(launch_waves(k_face_ring<Ex>, S.n_contacts, s, S, ex, fgrid, fg, budget, F.rec.p));
  }
  return launch_waves(k_face_scan<Ex>, S.n_contacts, s, S, ex, ring ? 1 : 0, F.rec.p);
}

}  // namespace
}  // namespace fb
