// Penalty contact between two handles on one device (body_contact.h), hand-written for gfx950.
//
// The rule is the header's (include/fembrain_hip.h, "Contact between two bodies"): the surface vertices of one body (P) that lie inside an
// element of the other (T) are pushed to the closest point of T's boundary, and the face that holds it is pushed back.  Per direction:
//  - candidates: a thread per surface vertex of P, the closed box of T's nodes, one compaction;
//  - containment: the elements of T whose current box meets the overlap of the two bodies' boxes -- a resting contact touches a thin layer,
//    and a large body does not pay a whole-mesh grid per step -- are binned into a grid over that overlap with the cell functions of
//    embed_grid.hip.h (an element over more than kEmbedWideCells cells goes to an overflow list, as in embed.hip); a thread per candidate
//    walks its cell, elements ascending, with embed's weight function: the first that contains it is the lowest;
//  - closest face: below;
//  - forces: a thread per contact forms F and adds it to its own node of P (the contacts of a direction are different nodes); the three
//    corners of the face in T become records (node, 3 contact + corner), sorted stably by node, and a thread per node's segment adds them
//    in record order -- ascending contact, corners 0 1 2 -- onto the value the vector had.  No floating-point atomics.
// Node ids cross from the caller's numbering to the handles' internal orders here: the surface's vnode / faces_int index the internal
// arrays, its vertex_ids / face order are what the caller reads.
//
// The closest face, one wavefront per contact (k_bc_ring).  The faces of T are binned by CENTROID into a grid over T's current box; their
// nine current coordinates are stored grouped by cell, faces ascending inside a cell, a plane per coordinate, so a run of cells along x
// is one contiguous range that the lanes stride over with coalesced loads.  Each lane keeps its minimum under the key (d, face) and
// wf_best folds them whenever a lane has improved.  R is the largest centroid-to-vertex distance over all faces, folded once per build
// and widened by 2^-40.
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
// point that has tested more than `budget` faces stops, is flagged, and k_bc_scan -- every face for the flagged points, the whole path
// for a body the proof does not cover, and the test twin -- finds the same (d, face): closest_on_triangle and centre_distance are one
// sequence of roundings on the same operands, and (d, face) is a total order.  The winner's closest point and weights are formed again
// from the face itself by bc_finish, for both paths alike.  Nothing spins.
// (closest_on_triangle, the grid rule, the face grid's kernels, SearchDev and bc_finish live in face_search.hip.h: self_contact.hip's
// twins of the two searches use them too.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "contact_friction.hip.h"
#include "device_prims.hip.h"
#include "embed_grid.hip.h"
#include "face_search.hip.h"
#include "fem_handle.h"
#include "launch.hip.h"
#include "mesh_device.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

struct Box3 {
  double lo[3], hi[3];
};

// ---- positions and boxes ----

// A thread per node (internal order): x0 + q, and the workgroup's box of them
__global__ __launch_bounds__(kB) void k_bc_positions(int n_nodes, const double* __restrict__ x0, const double* __restrict__ q, double* __restrict__ cur, double* __restrict__ part) {
  const int i = blockIdx.x * kB + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n_nodes) {
    const size_t b = 3 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double v = x0[b + k] + q[b + k];
      cur[b + k] = v;
      lo[k] = hi[k] = v;
    }
  }
  wg_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

// A thread per surface vertex: the workgroup's box of their current positions
__global__ __launch_bounds__(kB) void k_bc_surface_box(int nv, const int* __restrict__ vnode, int n_nodes, const double* __restrict__ cur, double* __restrict__ part) {
  const int v = blockIdx.x * kB + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (v < nv) {
    const int nd = vnode[v];
    if ((unsigned)nd < (unsigned)n_nodes)
#pragma unroll
      for (int k = 0; k < 3; k++) lo[k] = hi[k] = cur[3 * (size_t)nd + k];
  }
  wg_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

// ---- candidates and containment ----

// A thread per surface vertex of P: inside the closed box of T's nodes
__global__ __launch_bounds__(kB) void k_bc_candidates(int nv, const int* __restrict__ vnode, int n_nodes, const double* __restrict__ cur, Box3 T, unsigned char* __restrict__ flag) {
  const int v = blockIdx.x * kB + threadIdx.x;
  if (v >= nv) return;
  const int nd = vnode[v];
  bool in = false;
  if ((unsigned)nd < (unsigned)n_nodes) {
    const double p[3] = {cur[3 * (size_t)nd], cur[3 * (size_t)nd + 1], cur[3 * (size_t)nd + 2]};
    in = in_box(p, T.lo, T.hi);
  }
  flag[v] = in ? 1 : 0;
}

// the box of element e at the current positions, padded
__device__ __forceinline__ void tet_box(const int4* __restrict__ tets, const double* __restrict__ cur, int e, double pad, double* a, double* b) {
  double v[4][3];
  load_tet(tets, cur, e, v);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    a[k] = fmin(fmin(v[0][k], v[1][k]), fmin(v[2][k], v[3][k])) - pad;
    b[k] = fmax(fmax(v[0][k], v[1][k]), fmax(v[2][k], v[3][k])) + pad;
  }
}

// A thread per element of T: its padded box meets the overlap box O
__global__ __launch_bounds__(kB) void k_bc_tet_flag(int n_tets, const int4* __restrict__ tets, const double* __restrict__ cur, Box3 O, double pad, unsigned char* __restrict__ flag) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  double a[3], b[3];
  tet_box(tets, cur, e, pad, a, b);
  bool meets = true;
#pragma unroll
  for (int k = 0; k < 3; k++) meets = meets && a[k] <= O.hi[k] && b[k] >= O.lo[k];
  flag[e] = meets ? 1 : 0;
}

// the cells of the grid over O that the padded box of element e overlaps (clamped into the grid: the element may reach beyond O)
__device__ __forceinline__ void tet_cells_clamped(const GridDev& g, const int4* __restrict__ tets, const double* __restrict__ cur, int e, int* c0, int* c1) {
  double a[3], b[3];
  tet_box(tets, cur, e, g.pad, a, b);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c0[k] = cell_clamped(g, k, a[k]);
    c1[k] = cell_clamped(g, k, b[k]);
    if (c1[k] < c0[k]) c1[k] = c0[k];
  }
}

// A thread per binned element: the cells it overlaps, 0 for one of the overflow list (one entry past the end: the scan leaves the total there)
__global__ __launch_bounds__(kB) void k_bc_tet_count(int m, int n_tets, const int* __restrict__ sel, GridDev g, const int4* __restrict__ tets, const double* __restrict__ cur,
                                                     int* __restrict__ cnt, unsigned char* __restrict__ wide_flag) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j > m) return;
  if (j == m) { cnt[j] = 0; return; }
  const int e = sel[j];
  if ((unsigned)e >= (unsigned)n_tets) { cnt[j] = 0; wide_flag[j] = 0; return; }
  int c0[3], c1[3];
  tet_cells_clamped(g, tets, cur, e, c0, c1);
  const long long n = (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  const bool wide = n > kEmbedWideCells;
  cnt[j] = wide ? 0 : (int)n;
  wide_flag[j] = wide ? 1 : 0;
}

__global__ __launch_bounds__(kB) void k_bc_tet_emit(int m, int n_tets, const int* __restrict__ sel, GridDev g, const int4* __restrict__ tets, const double* __restrict__ cur,
                                                    const int* __restrict__ cnt, const int* __restrict__ off, long long n_pairs, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= m || cnt[j] == 0) return;
  const int e = sel[j];
  if ((unsigned)e >= (unsigned)n_tets) return;
  int c0[3], c1[3];
  tet_cells_clamped(g, tets, cur, e, c0, c1);
  long long o = off[j];
  const long long end = o + cnt[j];
  for (int z = c0[2]; z <= c1[2]; z++)
    for (int y = c0[1]; y <= c1[1]; y++)
      for (int x = c0[0]; x <= c1[0]; x++) {
        if (o < 0 || o >= end || o >= n_pairs) return;
        keys[o] = (uint32_t)((z * g.dim[1] + y) * g.dim[0] + x);
        vals[o] = (uint32_t)e;
        o++;
      }
}

// A thread per candidate: the lowest element of T that contains it, or -1.  g.wide / g.n_wide: the overflow list, ascending.
__global__ __launch_bounds__(kB) void k_bc_contain(int n_cand, const int* __restrict__ cand, int nv, const int* __restrict__ vnode, int n_nodes_p, const double* __restrict__ cur_p,
                                                   GridDev g, long long n_pairs, int n_tets, const int4* __restrict__ tets, const double* __restrict__ cur_t, int* __restrict__ c_elem,
                                                   unsigned char* __restrict__ flag) {
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= n_cand) return;
  int best = INT_MAX;
  const int vr = cand[t];
  const int nd = (unsigned)vr < (unsigned)nv ? vnode[vr] : -1;
  if ((unsigned)nd < (unsigned)n_nodes_p) {
    const double p[3] = {cur_p[3 * (size_t)nd], cur_p[3 * (size_t)nd + 1], cur_p[3 * (size_t)nd + 2]};
    if (in_box(p, g.lo, g.hi)) {
      const int c = (cell_of(g, 2, p[2]) * g.dim[1] + cell_of(g, 1, p[1])) * g.dim[0] + cell_of(g, 0, p[0]);
      const int j0 = max(g.cell_lo[c], 0), j1 = (int)min((long long)g.cell_hi[c], n_pairs);
      for (int j = j0; j < j1; j++) {
        const int e = g.cell_elem[j];
        if ((unsigned)e >= (unsigned)n_tets) continue;
        double v[4][3], w[4];
        load_tet(tets, cur_t, e, v);
        if (bary(v, p, w)) { best = e; break; }
      }
    }
    for (int j = 0; j < g.n_wide; j++) {
      const int e = g.wide[j];
      if (e >= best) break;  // (the list ascends)
      if ((unsigned)e >= (unsigned)n_tets) continue;
      double v[4][3], w[4];
      load_tet(tets, cur_t, e, v);
      if (bary(v, p, w)) { best = e; break; }
    }
  }
  c_elem[t] = best == INT_MAX ? -1 : best;
  flag[t] = best == INT_MAX ? 0 : 1;
}

// ---- the closest face ----

// One wavefront per contact, every face of T in its own order, lanes striding.  only_far: the points the ring search flagged, the others
// keep their records.
__global__ __launch_bounds__(kB) void k_bc_scan(SearchDev S, int only_far, BodyContactRec* __restrict__ rec) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = blockIdx.x * kWaves + wave;
  if (t >= S.n_contacts) return;
  if (only_far && rec[t].far == 0) return;  // (the same in every lane)
  double p[3] = {0.0, 0.0, 0.0};
  const int vr = contact_point(S, t, p);
  double bd = DBL_MAX;
  int bf = INT_MAX;
  if (vr >= 0)
    for (int f = lane; f < S.nf; f += 64) {
      double v[3][3];
      load_face(S.faces_int, S.n_nodes_t, S.cur_t, f, v);
      const double d = triangle_distance(p, v[0], v[1], v[2]);
      if (d < DBL_MAX && Lowest()(d, f, bd, bf)) { bd = d; bf = f; }
    }
  wf_best<int, Lowest>(bd, bf);
  if (lane == 0) bc_finish(S, t, vr, p, bf, (long long)S.nf, only_far != 0, rec);
}

// One wavefront per contact through the face grid.  Everything that decides a branch is the same in every lane: the ranges come from
// cell_start, the best pair is folded over the wavefront whenever a lane has improved it.
__global__ __launch_bounds__(kB) void k_bc_ring(SearchDev S, GridDev g, FaceDev fg, long long budget, BodyContactRec* __restrict__ rec) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = blockIdx.x * kWaves + wave;
  if (t >= S.n_contacts) return;
  double p[3] = {0.0, 0.0, 0.0};
  const int vr = contact_point(S, t, p);
  long long tested = 0;
  bool far = false;
  double bd = DBL_MAX;
  int bf = INT_MAX;
  if (vr >= 0) {
    const double R = *fg.R;
    const size_t nf = (size_t)S.nf;
    // the range [j0, j1) of the sorted faces (a run of cells along x): every lane its share, the best pair folded
    auto scan_range = [&](int j0, int j1) {
      bool improved = false;
      for (int j = j0 + lane; j < j1; j += 64) {
        const double a[3] = {fg.tri[j], fg.tri[nf + j], fg.tri[2 * nf + j]}, b[3] = {fg.tri[3 * nf + j], fg.tri[4 * nf + j], fg.tri[5 * nf + j]},
                     c[3] = {fg.tri[6 * nf + j], fg.tri[7 * nf + j], fg.tri[8 * nf + j]};
        const int f = fg.face[j];
        const double d = triangle_distance(p, a, b, c);
        if (d < DBL_MAX && Lowest()(d, f, bd, bf)) { bd = d; bf = f; improved = true; }
      }
      if (__any(improved)) wf_best<int, Lowest>(bd, bf);
      if (j1 > j0) tested += j1 - j0;
      if (tested > budget) far = true;
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
    // 1. shells until one holds a face, and the one after it; no further than kShells, behind which the bound of the box stands in
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
    if (bf == INT_MAX) far = true;  // (no face within the bound -- a boundary that is not closed, a rounding at the box's side: the scan decides)
  }
  if (lane == 0) {
    bc_finish(S, t, vr, p, far ? INT_MAX : bf, tested, false, rec);
    if (far) rec[t].far = 1;
  }
}

// ---- forces ----

// A thread per contact: F, its addition to the point's own node of P, and the three records of the face's corners in T
__global__ __launch_bounds__(kB) void k_bc_force(SearchDev S, double stiffness, double depth_cap, BodyContactRec* __restrict__ rec, double* __restrict__ fext_p,
                                                 uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= S.n_contacts) return;
  double p[3] = {0.0, 0.0, 0.0};
  const int vr = contact_point(S, t, p);
  BodyContactRec r = rec[t];
  const bool push = vr >= 0 && (unsigned)r.face < (unsigned)S.nf && r.d > 0.0;
  if (push) {
    const double depth = depth_cap > 0.0 ? fmin(r.d, depth_cap) : r.d;
    const double sd = stiffness * depth;
    const int nd = S.vnode[vr];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      r.f[k] = sd * ((r.c[k] - p[k]) / r.d);
      fext_p[3 * (size_t)nd + k] += r.f[k];
    }
    rec[t].f[0] = r.f[0]; rec[t].f[1] = r.f[1]; rec[t].f[2] = r.f[2];
  } else {
    rec[t].d = 0.0;  // (nothing is pushed: degenerate)
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int nd = push ? S.faces_int[3 * (size_t)r.face + k] : S.n_nodes_t;
    if ((unsigned)nd >= (unsigned)S.n_nodes_t) nd = S.n_nodes_t;  // (no node: sorted behind every node, and skipped)
    keys[3 * (size_t)t + k] = (uint32_t)nd;
    vals[3 * (size_t)t + k] = (uint32_t)(3 * t + k);
  }
}

// k_bc_force under the friction law (contact_friction.hip.h): the same push test, own-node addition and records, F the law's total --
// normal force with damping, minus the friction -- from the velocities of the point's node in P and of the face's corners in T, read
// from the handles' own qvel arrays (internal order, as the positions).  side[t]: N, |t|, t, -f; zero for a contact that pushes nothing.
__global__ __launch_bounds__(kB) void k_bc_force_friction(SearchDev S, double stiffness, double depth_cap, FrictionLaw law, const double* __restrict__ qvel_p,
                                                          const double* __restrict__ qvel_t, BodyContactRec* __restrict__ rec, ContactFrictionRec* __restrict__ side,
                                                          double* __restrict__ fext_p, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= S.n_contacts) return;
  double p[3] = {0.0, 0.0, 0.0};
  const int vr = contact_point(S, t, p);
  const BodyContactRec r = rec[t];
  const bool push = vr >= 0 && (unsigned)r.face < (unsigned)S.nf && r.d > 0.0;
  ContactFrictionRec o = {0.0, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (push) {
    const int nd = S.vnode[vr];
    double vp[3], vt[3][3], F[3];
    node_velocity(qvel_p, S.n_nodes_p, nd, vp);
#pragma unroll
    for (int k = 0; k < 3; k++) node_velocity(qvel_t, S.n_nodes_t, S.faces_int[3 * (size_t)r.face + k], vt[k]);
    contact_friction_law(p, r.c, r.b, r.d, stiffness, depth_cap, law, vp, vt, F, o);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      fext_p[3 * (size_t)nd + k] += F[k];
      rec[t].f[k] = F[k];
    }
  } else {
    rec[t].d = 0.0;  // (nothing is pushed: degenerate)
  }
  side[t] = o;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int nd = push ? S.faces_int[3 * (size_t)r.face + k] : S.n_nodes_t;
    if ((unsigned)nd >= (unsigned)S.n_nodes_t) nd = S.n_nodes_t;  // (no node: sorted behind every node, and skipped)
    keys[3 * (size_t)t + k] = (uint32_t)nd;
    vals[3 * (size_t)t + k] = (uint32_t)(3 * t + k);
  }
}

// A thread per sorted record: the first of a node's segment does that node's additions in record order
__global__ __launch_bounds__(kB) void k_bc_segments(int n_rec, const uint32_t* __restrict__ keys_s, const uint32_t* __restrict__ vals_s, int n_contacts, int n_nodes_t,
                                                    const BodyContactRec* __restrict__ rec, double* __restrict__ fext_t) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_rec) return;
  const uint32_t node = keys_s[i];
  if (node >= (uint32_t)n_nodes_t || (i > 0 && keys_s[i - 1] == node)) return;
  double a[3] = {fext_t[3 * (size_t)node], fext_t[3 * (size_t)node + 1], fext_t[3 * (size_t)node + 2]};
  for (int k = i; k < n_rec && keys_s[k] == node; k++) {
    const uint32_t v = vals_s[k];
    const uint32_t t = v / 3u, corner = v % 3u;
    if (t >= (uint32_t)n_contacts) continue;
    const BodyContactRec& r = rec[t];
    if (!(r.d > 0.0)) continue;
    const double w = r.b[corner];
    a[0] += (-r.f[0]) * w; a[1] += (-r.f[1]) * w; a[2] += (-r.f[2]) * w;
  }
  fext_t[3 * (size_t)node] = a[0]; fext_t[3 * (size_t)node + 1] = a[1]; fext_t[3 * (size_t)node + 2] = a[2];
}

// ---- host ----

// one body as a direction sees it
struct Body {
  fb_fem_s* h;
  int n_nodes, n_tets;
  const double* cur;
  double node_box[6], surf_box[6];
  double* fext;
};

// the stages of fb_fem_time_body_contact: events around each, on the calling handle's stream
struct Stages {
  BodyContactWork* W = nullptr;
  hipStream_t s = nullptr;
  double* seconds = nullptr;  // null: not timing
  int begin() {
    if (seconds) FB_HIP(hipEventRecord(W->ev_t[0], s));
    return FB_OK;
  }
  int end(int stage) {
    if (!seconds) return FB_OK;
    FB_HIP(hipEventRecord(W->ev_t[1], s));
    FB_HIP(hipEventSynchronize(W->ev_t[1]));
    float ms = 0;
    FB_HIP(hipEventElapsedTime(&ms, W->ev_t[0], W->ev_t[1]));
    seconds[stage] += ms * 1e-3;
    return FB_OK;
  }
};

// FEMBRAIN_BODY_CONTACT, read at every call: FB_BODY_CONTACT_SCAN / _RING, 0 where it is not set
int path_knob() {
  const char* env = getenv("FEMBRAIN_BODY_CONTACT");
  if (!env || !*env) return FB_BODY_CONTACT_NONE;
  if (!strcmp(env, "scan")) return FB_BODY_CONTACT_SCAN;
  if (!strcmp(env, "ring")) return FB_BODY_CONTACT_RING;
  return FB_BODY_CONTACT_NONE;
}

int ensure_events(BodyContactWork& W) {
  if (!W.ev_in) FB_HIP(hipEventCreateWithFlags(&W.ev_in, hipEventDisableTiming));
  if (!W.ev_out) FB_HIP(hipEventCreateWithFlags(&W.ev_out, hipEventDisableTiming));
  for (auto& e : W.ev_t)
    if (!e) FB_HIP(hipEventCreate(&e));
  return FB_OK;
}

// current positions of a body and the boxes of its nodes and of its surface vertices, into boxes[12 which ..]
int body_boxes(hipStream_t s, BodyContactWork& W, fb_fem_s* h, int which) {
  const int n = h->plan.n_global, nv = h->surf.n_vertices;
  const int nb = blocks_for(n), nbv = blocks_for(nv);
  FB_TRY(W.cur[which].reserve((size_t)3 * n));
  FB_TRY(W.box_part.reserve((size_t)6 * std::max(nb, nbv)));
  FB_TRY(launch_1d(k_bc_positions, n, s, n, h->x0.p, h->q.p, W.cur[which].p, W.box_part.p));
  FB_TRY(launch_grid(k_box_final<double>, dim3(1), s, nb, W.box_part.p, W.boxes.p + 12 * which));
  FB_TRY(launch_1d(k_bc_surface_box, nv, s, nv, h->surf.vnode.p, n, W.cur[which].p, W.box_part.p));
  FB_TRY(launch_grid(k_box_final<double>, dim3(1), s, nbv, W.box_part.p, W.boxes.p + 12 * which + 6));
  return FB_OK;
}

struct DirResult {
  int n_candidates = 0, n_contacts = 0, path = FB_BODY_CONTACT_NONE, tet_grids = 0, face_grids = 0;
};

// One direction: the surface vertices of P against T.  s: the calling handle's stream; fext_p / fext_t: where the forces are added.
// law: null for the frictionless rule; else the friction call's, its side records into side_out.
int run_direction(hipStream_t s, BodyContactWork& W, PlanWorkspace& ws, const Body& P, const Body& T, const fb_fem_body_contact_params& prm, double* fext_p, double* fext_t,
                  Stages& tm, std::vector<BodyContactRec>& out, DirResult& res, const FrictionLaw* law = nullptr, std::vector<ContactFrictionRec>* side_out = nullptr) {
  out.clear();
  if (side_out) side_out->clear();
  const SurfaceWork& SP = P.h->surf;
  const SurfaceWork& ST = T.h->surf;
  const int nv = SP.n_vertices, nf = ST.n_faces;
  // the overlap of P's surface box and T's node box; where they do not meet the direction ends
  Box3 O, TB;
  bool meet = nv > 0 && nf > 0 && T.n_tets > 0;
  for (int k = 0; k < 3; k++) {
    O.lo[k] = std::max(P.surf_box[k], T.node_box[k]); O.hi[k] = std::min(P.surf_box[3 + k], T.node_box[3 + k]);
    TB.lo[k] = T.node_box[k]; TB.hi[k] = T.node_box[3 + k];
    if (!(O.lo[k] <= O.hi[k])) meet = false;
  }
  if (!meet) return FB_OK;
  double ext_max = 0.0;
  for (int k = 0; k < 3; k++) ext_max = std::max(ext_max, TB.hi[k] - TB.lo[k]);
  if (!(ext_max > 0.0)) ext_max = 1.0;
  const double pad = std::ldexp(ext_max, -30);  // (embed_grid_build's padding: far above the rounding of a determinant test)

  // ---- candidates, element grid, containment ----
  FB_TRY(tm.begin());
  FB_TRY(W.counts.reserve(4));
  FB_TRY(W.flag.reserve((size_t)std::max(std::max(nv, T.n_tets), 1)));
  FB_TRY(W.cand.reserve((size_t)nv));
  FB_TRY(launch_1d(k_bc_candidates, nv, s, nv, SP.vnode.p, P.n_nodes, P.cur, TB, W.flag.p));
  FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.cand.p, W.counts.p, (size_t)nv));
  int n_cand = 0;
  FB_TRY(W.counts.download(&n_cand, 1, s));  // a host wait
  if (n_cand < 0 || n_cand > nv) return fail(FB_EDEVICE, "body contact: %d candidates of %d surface vertices", n_cand, nv);
  res.n_candidates = n_cand;
  int n_contacts = 0;
  GridDev tg;
  memset(&tg, 0, sizeof(tg));
  if (n_cand > 0) {
    FB_TRY(W.sel.reserve((size_t)T.n_tets));
    FB_TRY(launch_1d(k_bc_tet_flag, T.n_tets, s, T.n_tets, T.h->tets.p, T.cur, O, pad, W.flag.p));
    FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.sel.p, W.counts.p + 1, (size_t)T.n_tets));
    int m = 0;
    FB_TRY(W.counts.download(&m, 1, s, 1));  // a host wait
    if (m < 0 || m > T.n_tets) return fail(FB_EDEVICE, "body contact: %d of %d elements binned", m, T.n_tets);
    if (m > 0) {
      tg = make_grid(O.lo, O.hi, pad, m);
      const int n_cells = tg.dim[0] * tg.dim[1] * tg.dim[2];
      FB_TRY(W.t_cnt.reserve((size_t)m + 1)); FB_TRY(W.t_off.reserve((size_t)m + 1));
      FB_TRY(W.cell_lo.reserve((size_t)n_cells)); FB_TRY(W.cell_hi.reserve((size_t)n_cells));
      FB_TRY(ws.vals_s.reserve((size_t)m));  // (the overflow list: the plan builder's array, as the sort's below)
      int* wide = reinterpret_cast<int*>(ws.vals_s.p);
      FB_TRY(launch_1d(k_bc_tet_count, m + 1, s, m, T.n_tets, W.sel.p, tg, T.h->tets.p, T.cur, W.t_cnt.p, W.flag.p));
      FB_TRY(exclusive_scan(ws.temp, s, W.t_cnt.p, W.t_off.p, 0, (size_t)m + 1));
      FB_TRY(select_flagged(ws.temp, s, W.sel.p, W.flag.p, wide, W.counts.p + 2, (size_t)m));
      int total = 0, n_wide = 0;
      FB_HIP(hipMemcpyAsync(&total, W.t_off.p + m, sizeof(int), hipMemcpyDeviceToHost, s));
      FB_HIP(hipMemcpyAsync(&n_wide, W.counts.p + 2, sizeof(int), hipMemcpyDeviceToHost, s));
      FB_HIP(hipStreamSynchronize(s));  // a host wait
      if (total < 0 || (long long)total > (long long)kEmbedWideCells * m || n_wide < 0 || n_wide > m)
        return fail(FB_EDEVICE, "body contact grid: %d pairs, %d wide elements out of range", total, n_wide);
      FB_HIP(hipMemsetAsync(W.cell_lo.p, 0, sizeof(int) * (size_t)n_cells, s));
      FB_HIP(hipMemsetAsync(W.cell_hi.p, 0, sizeof(int) * (size_t)n_cells, s));
      FB_TRY(W.cell_elem.reserve((size_t)std::max(total, 1)));
      if (total) {
        FB_TRY(ws.keys.reserve(((size_t)total + 1) / 2)); FB_TRY(ws.keys_s.reserve(((size_t)total + 1) / 2)); FB_TRY(ws.vals.reserve((size_t)total));
        uint32_t* ck = reinterpret_cast<uint32_t*>(ws.keys.p);
        uint32_t* ck_s = reinterpret_cast<uint32_t*>(ws.keys_s.p);
        FB_TRY(launch_1d(k_bc_tet_emit, m, s, m, T.n_tets, W.sel.p, tg, T.h->tets.p, T.cur, W.t_cnt.p, W.t_off.p, (long long)total, ck, ws.vals.p));
        FB_TRY(sort_pairs(ws.temp, s, ck, ck_s, ws.vals.p, reinterpret_cast<uint32_t*>(W.cell_elem.p), (size_t)total, (unsigned)bits_of(n_cells)));
        FB_TRY(launch_1d(k_run_bounds<>, (long long)total, s, total, ck_s, (uint32_t)n_cells, W.cell_lo.p, W.cell_hi.p));
      }
      tg.n_wide = n_wide;
      tg.cell_lo = W.cell_lo.p; tg.cell_hi = W.cell_hi.p; tg.cell_elem = W.cell_elem.p; tg.wide = wide;
      res.tet_grids = 1;
      FB_TRY(W.c_elem.reserve((size_t)n_cand)); FB_TRY(W.hit.reserve((size_t)n_cand));
      FB_TRY(launch_1d(k_bc_contain, n_cand, s, n_cand, W.cand.p, nv, SP.vnode.p, P.n_nodes, P.cur, tg, (long long)total, T.n_tets, T.h->tets.p, T.cur, W.c_elem.p, W.flag.p));
      FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.hit.p, W.counts.p + 3, (size_t)n_cand));
      FB_TRY(W.counts.download(&n_contacts, 1, s, 3));  // a host wait
      if (n_contacts < 0 || n_contacts > n_cand) return fail(FB_EDEVICE, "body contact: %d contacts of %d candidates", n_contacts, n_cand);
    }
  }
  FB_TRY(tm.end(1));
  res.n_contacts = n_contacts;
  if (n_contacts == 0) return FB_OK;

  // ---- the path, and the face grid where it is the ring's ----
  GridDev fgrid = make_grid(TB.lo, TB.hi, pad, nf);
  const int knob = path_knob();
  const bool ring = knob != FB_BODY_CONTACT_SCAN && grid_covered(fgrid);  // (default: the ring wherever its proof holds; DESIGN.md 3k has the table)
  res.path = ring ? FB_BODY_CONTACT_RING : FB_BODY_CONTACT_SCAN;
  long long budget = nf;  // (a point that has tested as many faces as a scan tests gains nothing from going on)
  if (const char* env = getenv("FEMBRAIN_BODY_CONTACT_BUDGET"))
    if (*env) budget = std::max(0LL, atoll(env));
  FB_TRY(tm.begin());
  if (ring) {
    const int n_cells = fgrid.dim[0] * fgrid.dim[1] * fgrid.dim[2], nbf = blocks_for(nf);
    FB_TRY(W.f_cnt.reserve((size_t)n_cells + 1)); FB_TRY(W.f_start.reserve((size_t)n_cells + 1)); FB_TRY(W.f_face.reserve((size_t)nf));
    FB_TRY(W.f_tri.reserve((size_t)9 * nf)); FB_TRY(W.f_R.reserve((size_t)nbf + 1));
    FB_HIP(hipMemsetAsync(W.f_cnt.p, 0, sizeof(int) * ((size_t)n_cells + 1), s));
    FB_TRY(ws.keys.reserve(((size_t)nf + 1) / 2)); FB_TRY(ws.keys_s.reserve(((size_t)nf + 1) / 2)); FB_TRY(ws.vals.reserve((size_t)nf));
    uint32_t* ck = reinterpret_cast<uint32_t*>(ws.keys.p);
    uint32_t* ck_s = reinterpret_cast<uint32_t*>(ws.keys_s.p);
    FB_TRY(launch_1d(k_bc_face_keys, nf, s, nf, ST.faces_int.p, T.n_nodes, T.cur, fgrid, ck, ws.vals.p, W.f_cnt.p, W.f_R.p));
    FB_TRY(launch_grid(k_bc_R_final, dim3(1), s, nbf, W.f_R.p, W.f_R.p + nbf));
    FB_TRY(sort_pairs(ws.temp, s, ck, ck_s, ws.vals.p, reinterpret_cast<uint32_t*>(W.f_face.p), (size_t)nf, (unsigned)bits_of(n_cells)));
    FB_TRY(exclusive_scan(ws.temp, s, W.f_cnt.p, W.f_start.p, 0, (size_t)n_cells + 1));
    FB_TRY(launch_1d(k_bc_face_store, nf, s, nf, W.f_face.p, ST.faces_int.p, T.n_nodes, T.cur, W.f_tri.p));
    res.face_grids = 1;
  }
  FB_TRY(tm.end(2));

  // ---- the closest faces ----
  FB_TRY(tm.begin());
  FB_TRY(W.rec.reserve((size_t)n_contacts));
  SearchDev S;
  S.n_contacts = n_contacts; S.hit = W.hit.p; S.cand = W.cand.p; S.vnode = SP.vnode.p; S.vertex_ids = SP.vertex_ids.p; S.c_elem = W.c_elem.p;
  S.n_cand = n_cand; S.nv = nv; S.n_nodes_p = P.n_nodes; S.cur_p = P.cur;
  S.nf = nf; S.n_nodes_t = T.n_nodes; S.faces_int = ST.faces_int.p; S.cur_t = T.cur;
  if (ring) {
    const FaceDev fg = {W.f_start.p, W.f_face.p, W.f_tri.p, W.f_R.p + blocks_for(nf)};
    FB_TRY(launch_waves(k_bc_ring, n_contacts, s, S, fgrid, fg, budget, W.rec.p));
    FB_TRY(launch_waves(k_bc_scan, n_contacts, s, S, 1, W.rec.p));  // (the points past their budget; a wavefront of any other returns at once)
  } else {
    FB_TRY(launch_waves(k_bc_scan, n_contacts, s, S, 0, W.rec.p));
  }
  FB_TRY(tm.end(3));

  // ---- forces ----
  FB_TRY(tm.begin());
  const size_t n_rec = (size_t)3 * n_contacts;
  FB_TRY(W.r_key.reserve(n_rec)); FB_TRY(W.r_key_s.reserve(n_rec)); FB_TRY(W.r_val.reserve(n_rec)); FB_TRY(W.r_val_s.reserve(n_rec));
  if (law) {
    FB_TRY(W.fric.reserve((size_t)n_contacts));
    FB_TRY(launch_1d(k_bc_force_friction, n_contacts, s, S, prm.stiffness, prm.depth_cap, *law, P.h->qvel.p, T.h->qvel.p, W.rec.p, W.fric.p, fext_p, W.r_key.p, W.r_val.p));
  } else {
    FB_TRY(launch_1d(k_bc_force, n_contacts, s, S, prm.stiffness, prm.depth_cap, W.rec.p, fext_p, W.r_key.p, W.r_val.p));
  }
  FB_TRY(sort_pairs(ws.temp, s, W.r_key.p, W.r_key_s.p, W.r_val.p, W.r_val_s.p, n_rec, (unsigned)bits_of((long long)T.n_nodes + 1)));
  FB_TRY(launch_1d(k_bc_segments, (long long)n_rec, s, (int)n_rec, W.r_key_s.p, W.r_val_s.p, n_contacts, T.n_nodes, W.rec.p, fext_t));
  out.resize((size_t)n_contacts);
  if (law && side_out) {
    side_out->resize((size_t)n_contacts);
    FB_HIP(hipMemcpyAsync(side_out->data(), W.fric.p, sizeof(ContactFrictionRec) * (size_t)n_contacts, hipMemcpyDeviceToHost, s));  // (the wait below covers it)
  }
  FB_TRY(W.rec.download(out.data(), (size_t)n_contacts, s));  // a host wait
  FB_TRY(tm.end(4));
  return FB_OK;
}

int check_pair(fb_fem_s* a, fb_fem_s* b, const fb_fem_body_contact_params* p) {
  if (a == b) return fail(FB_EINVAL, "fb_fem_body_contact: the two handles are the same (self-contact is not built)");
  if (a->plan.n_ranks > 1 || b->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_body_contact is for unsharded handles");
  if (a->prm.device != b->prm.device) return fail(FB_EINVAL, "fb_fem_body_contact: the handles are on devices %d and %d", a->prm.device, b->prm.device);
  if (!p) return fail(FB_EINVAL, "null body contact parameters");
  if (!std::isfinite(p->stiffness) || p->stiffness < 0.0) return fail(FB_EINVAL, "body contact stiffness %g", p->stiffness);
  if (!std::isfinite(p->depth_cap) || p->depth_cap < 0.0) return fail(FB_EINVAL, "body contact depth cap %g", p->depth_cap);
  if ((p->directions & (FB_BODY_A_INTO_B | FB_BODY_B_INTO_A)) == 0 || (p->directions & ~(FB_BODY_A_INTO_B | FB_BODY_B_INTO_A)) != 0)
    return fail(FB_EINVAL, "body contact directions %d", p->directions);
  if (a->plan.n_global <= 0 || b->plan.n_global <= 0 || a->plan.n_global >= (1 << 28) || b->plan.n_global >= (1 << 28))
    return fail(FB_EINVAL, "fb_fem_body_contact: %d and %d nodes", a->plan.n_global, b->plan.n_global);
  return FB_OK;
}

// add: into the two external force vectors, the result kept for fb_fem_read_body_contact; else into scratch, nothing kept (seconds: the stages).
// fr: null for the frictionless call; else the friction call's parameters, fout its info.
int body_contact(fb_fem_s* a, fb_fem_s* b, const fb_fem_body_contact_params& prm, bool add, double* seconds, fb_fem_body_contact_info* out,
                 const fb_fem_contact_friction_params* fr = nullptr, fb_fem_contact_friction_info* fout = nullptr) {
  BodyContactWork& W = a->bodyc;
  hipStream_t s = a->stream;
  // both surfaces belong to the current meshes (each is built on its own handle's stream, with its host waits)
  FB_TRY(surface_current(a));
  FB_TRY(surface_current(b));
  FB_TRY(ensure_events(W));
  // after what b has queued
  FB_HIP(hipEventRecord(W.ev_in, b->stream));
  FB_HIP(hipStreamWaitEvent(s, W.ev_in, 0));
  Stages tm;
  tm.W = &W; tm.s = s; tm.seconds = seconds;
  FB_TRY(tm.begin());
  const size_t n_boxes = fr ? 25 : 24;  // (the friction call: behind the boxes the flag of a velocity that is not finite, read in the same wait)
  FB_TRY(W.boxes.reserve(n_boxes));
  FB_TRY(body_boxes(s, W, a, 0));
  FB_TRY(body_boxes(s, W, b, 1));
  if (fr) {
    FB_HIP(hipMemsetAsync(W.boxes.p + 24, 0, sizeof(double), s));
    FB_TRY(launch_1d(k_cf_finite, 3LL * a->plan.n_global, s, 3LL * a->plan.n_global, a->qvel.p, W.boxes.p + 24));
    FB_TRY(launch_1d(k_cf_finite, 3LL * b->plan.n_global, s, 3LL * b->plan.n_global, b->qvel.p, W.boxes.p + 24));
  }
  double boxes[25];
  boxes[24] = 0.0;
  FB_TRY(W.boxes.download(boxes, n_boxes, s));  // a host wait
  FB_TRY(tm.end(0));
  Body A = {a, a->plan.n_global, a->plan.n_tets, W.cur[0].p, {}, {}, a->fext.p}, B = {b, b->plan.n_global, b->plan.n_tets, W.cur[1].p, {}, {}, b->fext.p};
  memcpy(A.node_box, boxes, sizeof(double) * 6); memcpy(A.surf_box, boxes + 6, sizeof(double) * 6);
  memcpy(B.node_box, boxes + 12, sizeof(double) * 6); memcpy(B.surf_box, boxes + 18, sizeof(double) * 6);
  for (int k = 0; k < 6; k++)
    if (!std::isfinite(A.node_box[k]) || !std::isfinite(B.node_box[k])) return fail(FB_EINVAL, "fb_fem_body_contact: a position of a body is not finite");
  if (boxes[24] != 0.0) return fail(FB_EINVAL, "fb_fem_body_contact_friction: a velocity of a body is not finite");
  if (!add) {
    FB_TRY(W.scratch[0].reserve((size_t)3 * A.n_nodes)); FB_TRY(W.scratch[1].reserve((size_t)3 * B.n_nodes));
    FB_TRY(W.scratch[0].zero(s)); FB_TRY(W.scratch[1].zero(s));
    A.fext = W.scratch[0].p; B.fext = W.scratch[1].p;
  }
  fb_fem_body_contact_info I;
  memset(&I, 0, sizeof(I));
  std::vector<BodyContactRec> recs[2];
  std::vector<ContactFrictionRec> side[2];
  fb_fem_contact_friction_info FI;
  memset(&FI, 0, sizeof(FI));
  const FrictionLaw law = {fr ? fr->mu : 0.0, fr ? fr->slip_speed : 0.0, fr ? fr->damping : 0.0};
  int rc = FB_OK;
  for (int dir = 0; dir < 2 && rc == FB_OK; dir++) {
    if (!(prm.directions & (dir == 0 ? FB_BODY_A_INTO_B : FB_BODY_B_INTO_A))) continue;
    const Body& P = dir == 0 ? A : B;
    const Body& T = dir == 0 ? B : A;
    DirResult R;
    rc = run_direction(s, W, a->plan_ws, P, T, prm, P.fext, T.fext, tm, recs[dir], R, fr ? &law : nullptr, fr ? &side[dir] : nullptr);
    if (rc != FB_OK) break;
    if (fr) friction_sums(recs[dir], side[dir], *fr, dir, FI);
    I.n_candidates[dir] = R.n_candidates; I.n_contacts[dir] = R.n_contacts;
    I.n_tet_grid_builds += R.tet_grids; I.n_face_grid_builds += R.face_grids;
    if (R.n_contacts > 0) I.path = R.path;
    double* on_p = dir == 0 ? I.force_on_a : I.force_on_b;
    double* on_t = dir == 0 ? I.force_on_b : I.force_on_a;
    for (const BodyContactRec& r : recs[dir]) {
      I.faces_tested += r.tested;
      if (!(r.d > 0.0)) { I.n_degenerate[dir]++; continue; }
      const double depth = prm.depth_cap > 0.0 ? std::min(r.d, prm.depth_cap) : r.d;
      I.max_depth = std::max(I.max_depth, depth);
      for (int k = 0; k < 3; k++) on_p[k] += r.f[k];
      for (int c = 0; c < 3; c++)
        for (int k = 0; k < 3; k++) on_t[k] += (-r.f[k]) * r.b[c];
    }
  }
  // what b queues from here on runs after this call (also after a failure: the kernels launched so far read b's arrays)
  const hipError_t e1 = hipEventRecord(W.ev_out, s);
  const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(b->stream, W.ev_out, 0) : e1;
  FB_TRY(rc);
  FB_HIP(e1);
  FB_HIP(e2);
  if (add) {
    W.host[0].swap(recs[0]); W.host[1].swap(recs[1]);
    W.info = I;
    if (fr) { W.fric_host[0].swap(side[0]); W.fric_host[1].swap(side[1]); }
  }
  if (out) *out = I;
  if (fr && fout) *fout = FI;
  return FB_OK;
}

}  // namespace
}  // namespace fb

// ---- the C ABI ----

int fb_fem_body_contact(fb_fem_t a, fb_fem_t b, const fb_fem_body_contact_params* p, fb_fem_body_contact_info* out) {
  CHECK_HANDLE(a);
  CHECK_HANDLE(b);
  FB_TRY(check_pair(a, b, p));
  return body_contact(a, b, *p, true, nullptr, out);
}

int fb_fem_body_contact_friction(fb_fem_t a, fb_fem_t b, const fb_fem_body_contact_params* p, const fb_fem_contact_friction_params* fr, fb_fem_body_contact_info* out,
                                 fb_fem_contact_friction_info* fout) {
  CHECK_HANDLE(a);
  CHECK_HANDLE(b);
  FB_TRY(check_pair(a, b, p));
  FB_TRY(check_friction(fr, "fb_fem_body_contact_friction"));
  return body_contact(a, b, *p, true, nullptr, out, fr, fout);
}

int fb_fem_read_body_contact_friction(fb_fem_t a, int direction, double* normal_force, double* slip3, double* friction3) {
  CHECK_HANDLE(a);
  if (direction != FB_BODY_A_INTO_B && direction != FB_BODY_B_INTO_A) return fail(FB_EINVAL, "fb_fem_read_body_contact_friction: direction %d", direction);
  read_friction(a->bodyc.fric_host[direction == FB_BODY_A_INTO_B ? 0 : 1], normal_force, slip3, friction3);
  return FB_OK;
}

int fb_fem_read_body_contact(fb_fem_t a, int direction, int* node, int* element, int* face, double* closest_xyz, double* bary3, double* depth) {
  CHECK_HANDLE(a);
  if (direction != FB_BODY_A_INTO_B && direction != FB_BODY_B_INTO_A) return fail(FB_EINVAL, "fb_fem_read_body_contact: direction %d", direction);
  const std::vector<BodyContactRec>& v = a->bodyc.host[direction == FB_BODY_A_INTO_B ? 0 : 1];
  for (size_t i = 0; i < v.size(); i++) {
    const BodyContactRec& r = v[i];
    if (node) node[i] = r.node;
    if (element) element[i] = r.elem;
    if (face) face[i] = r.face;
    if (closest_xyz) memcpy(closest_xyz + 3 * i, r.c, sizeof(double) * 3);
    if (bary3) memcpy(bary3 + 3 * i, r.b, sizeof(double) * 3);
    if (depth) depth[i] = r.d;
  }
  return FB_OK;
}

int fb_fem_time_body_contact(fb_fem_t a, fb_fem_t b, const fb_fem_body_contact_params* p, int reps, double seconds[5]) {
  CHECK_HANDLE(a);
  CHECK_HANDLE(b);
  FB_TRY(check_pair(a, b, p));
  if (reps < 1 || !seconds) return fail(FB_EINVAL, "fb_fem_time_body_contact: reps must be positive and seconds not null");
  FB_TRY(body_contact(a, b, *p, false, nullptr, nullptr));  // warm: the buffers exist
  double sum[5] = {0, 0, 0, 0, 0};
  for (int r = 0; r < reps; r++) FB_TRY(body_contact(a, b, *p, false, sum, nullptr));
  for (int k = 0; k < 5; k++) seconds[k] = sum[k] / reps;
  return FB_OK;
}
