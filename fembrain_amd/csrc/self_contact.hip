// Penalty contact of a handle with itself (self_contact.h), hand-written for gfx950.
//
// The rule is the header's (include/fembrain_hip.h, "Contact of a body with itself"): every surface vertex that lies inside an element
// it may meet is pushed to the closest point of the boundary it may meet, and the face there is pushed back.  What a point may not meet
// is its exclusion: under FB_SELF_CONTACT_ANY the elements and faces that have the point's node among their own, under
// FB_SELF_CONTACT_OTHER_PARTS those of the point's part.  A point's key is its internal node or its part, an element answers with its
// four nodes or element_part, a face with its three nodes or the part of its element (face_part, filled once per call).
//  - positions: a thread per node, x0 + q and the box; a position that is not finite opens the box to infinity and the call ends there;
//  - containment, the other way round than body_contact.hip: the body's box is its own, so every surface vertex is a candidate and every
//    element would be binned.  The surface vertices -- two orders of magnitude fewer -- are binned instead, one sort over the cells of a
//    grid over the box, positions and keys stored in sorted order; a thread per element walks the cells its padded current box overlaps
//    (the cell functions of embed_grid.hip.h) and, for each point there that its box holds, that it may meet and whose four weights
//    (embed's bary) are >= 0, takes the point's slot with an integer atomicMin of its own id.  The lowest element wins whatever the
//    order: no floating-point atomic, the same bits from call to call.  An element over more than kEmbedWideCells cells goes to an
//    overflow list that wavefronts walk afterwards, lanes striding over the sorted points.  One compaction of the taken slots, one host
//    wait for their number;
//  - closest face: k_sc_scan / k_sc_ring, body_contact.hip's two searches with the excluded faces skipped (below);
//  - forces: here a node can be pushed as a point and push back as a corner in one call, so all four contributions of a contact are
//    records (node, 4 contact + r), r = 0 the point's +F, r = 1..3 the corners' (-F) b_k; sorted stably by node, and the thread at the head
//    of a node's segment adds the whole segment, however long, in record order onto the value the vector had.
//
// The ring under an exclusion.  The coverage argument is body_contact.hip's, word for word: it shows that no face OUTSIDE the visited
// cells has a computed distance <= best_d.  Skipping faces inside visited cells removes candidates and touches none of its steps.  What
// changes is where best_d comes from:
//  - the shells look for their first candidate among the faces the point may take (a range "holds a face" only if it holds such a one):
//    a surface vertex's own cell is full of its own faces, and stopping at them would leave the second phase without a bound;
//  - the bound of the box, m, no longer implies that a face the point MAY TAKE lies within m -- the face where the point leaves the body
//    may be its own.  Nothing rested on that implication before and nothing does now: a search that ends without a face is flagged and
//    k_sc_scan decides, as for a point past its budget.  A contact for which the scan finds no face either has none left and is dropped.
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

// ---- the exclusion ----

// of an element: t its nodes, part its part
__device__ __forceinline__ bool element_excluded(int mode, int key, const int4& t, int part) {
  return mode == FB_SELF_CONTACT_OTHER_PARTS ? part == key : (t.x == key || t.y == key || t.z == key || t.w == key);
}

// of a face, as the searches ask
struct FaceExclusion {
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

// ---- positions ----

// A thread per node (internal order): x0 + q, and the workgroup's box of them; a value that is not finite makes the box infinite
__global__ __launch_bounds__(kB) void k_sc_positions(int n_nodes, const double* __restrict__ x0, const double* __restrict__ q, double* __restrict__ cur, double* __restrict__ part) {
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

// ---- the grid of surface vertices and containment ----

// A thread per surface vertex: its cell, its key, its empty slot.  A vertex without a node sorts behind every cell.
__global__ __launch_bounds__(kB) void k_sc_point_keys(int nv, const int* __restrict__ vnode, const int* __restrict__ vertex_ids, int n_nodes, const double* __restrict__ cur, GridDev g,
                                                      int mode, const int* __restrict__ node_part_out, int* __restrict__ p_key, uint32_t* __restrict__ cells,
                                                      uint32_t* __restrict__ vals, int* __restrict__ slot) {
  const int v = blockIdx.x * kB + threadIdx.x;
  if (v >= nv) return;
  const int nd = vnode[v];
  uint32_t cell = (uint32_t)(g.dim[0] * g.dim[1] * g.dim[2]);
  int key = -1;
  if ((unsigned)nd < (unsigned)n_nodes) {
    const double* p = cur + 3 * (size_t)nd;
    cell = (uint32_t)((cell_clamped(g, 2, p[2]) * g.dim[1] + cell_clamped(g, 1, p[1])) * g.dim[0] + cell_clamped(g, 0, p[0]));
    if (mode == FB_SELF_CONTACT_OTHER_PARTS) {
      const int c = vertex_ids[v];
      key = (unsigned)c < (unsigned)n_nodes ? node_part_out[c] : -1;
    } else {
      key = nd;
    }
  }
  cells[v] = cell;
  vals[v] = (uint32_t)v;
  p_key[v] = key;
  slot[v] = INT_MAX;
}

// A thread per sorted entry: the point's coordinates, a plane each, and its key (a vertex without a node: no position, nothing holds it)
__global__ __launch_bounds__(kB) void k_sc_point_store(int nv, const uint32_t* __restrict__ p_v_s, const int* __restrict__ vnode, int n_nodes, const double* __restrict__ cur,
                                                       const int* __restrict__ p_key, double* __restrict__ xyz, int* __restrict__ key_s) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= nv) return;
  const uint32_t v = p_v_s[j];
  const int nd = v < (uint32_t)nv ? vnode[v] : -1;
  const bool ok = (unsigned)nd < (unsigned)n_nodes;
#pragma unroll
  for (int k = 0; k < 3; k++) xyz[(size_t)k * nv + j] = ok ? cur[3 * (size_t)nd + k] : NAN;
  key_s[j] = ok ? p_key[v] : -1;
}

// what the containment kernels know of the sorted points
struct PointsDev {
  int nv, mode;
  const int *cell_lo, *cell_hi;
  const double* xyz;
  const int* key_s;
  const uint32_t* v_s;
  int* slot;
};

// the sorted point j against element e (vertices v, padded box [a, b], nodes t, part)
__device__ __forceinline__ void test_point(const PointsDev& P, int j, int e, const int4& t, int part, const double (*v)[3], const double* a, const double* b) {
  const double p[3] = {P.xyz[j], P.xyz[(size_t)P.nv + j], P.xyz[2 * (size_t)P.nv + j]};
  if (!in_box(p, a, b)) return;  // (also a position that is not a number)
  if (element_excluded(P.mode, P.key_s[j], t, part)) return;
  double w[4];
  if (!bary(v, p, w)) return;
  const uint32_t vr = P.v_s[j];
  if (vr < (uint32_t)P.nv) atomicMin(P.slot + vr, e);
}

__device__ __forceinline__ void padded_box(const double (*v)[3], double pad, double* a, double* b) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    a[k] = fmin(fmin(v[0][k], v[1][k]), fmin(v[2][k], v[3][k])) - pad;
    b[k] = fmax(fmax(v[0][k], v[1][k]), fmax(v[2][k], v[3][k])) + pad;
  }
}

// A thread per element: the points of the cells its padded box overlaps; an element over more than kEmbedWideCells cells is flagged
__global__ __launch_bounds__(kB) void k_sc_contain(int n_tets, const int4* __restrict__ tets, const double* __restrict__ cur, const int* __restrict__ element_part, GridDev g, PointsDev P,
                                                   unsigned char* __restrict__ wide_flag) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  double v[4][3], a[3], b[3];
  load_tet(tets, cur, e, v);
  padded_box(v, g.pad, a, b);
  int c0[3], c1[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c0[k] = cell_clamped(g, k, a[k]);
    c1[k] = cell_clamped(g, k, b[k]);
    if (c1[k] < c0[k]) c1[k] = c0[k];
  }
  const long long n = (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  const bool wide = n > kEmbedWideCells;
  wide_flag[e] = wide ? 1 : 0;
  if (wide) return;
  const int4 t = tets[e];
  const int part = P.mode == FB_SELF_CONTACT_OTHER_PARTS ? element_part[e] : 0;
  for (int z = c0[2]; z <= c1[2]; z++)
    for (int y = c0[1]; y <= c1[1]; y++)
      for (int x = c0[0]; x <= c1[0]; x++) {
        const int c = (z * g.dim[1] + y) * g.dim[0] + x;
        const int j1 = min(P.cell_hi[c], P.nv);
        for (int j = max(P.cell_lo[c], 0); j < j1; j++) test_point(P, j, e, t, part, v, a, b);
      }
}

// Wavefronts over the overflow list (its length on the device: nobody waits for it), lanes striding over every sorted point
__global__ __launch_bounds__(kB) void k_sc_contain_wide(const int* __restrict__ n_wide, const int* __restrict__ wide, int n_tets, const int4* __restrict__ tets,
                                                        const double* __restrict__ cur, const int* __restrict__ element_part, double pad, PointsDev P) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = min(max(*n_wide, 0), n_tets), n_waves = gridDim.x * kWaves;
  for (int i = blockIdx.x * kWaves + wave; i < n; i += n_waves) {
    const int e = wide[i];
    if ((unsigned)e >= (unsigned)n_tets) continue;
    double v[4][3], a[3], b[3];
    load_tet(tets, cur, e, v);
    padded_box(v, pad, a, b);
    const int4 t = tets[e];
    const int part = P.mode == FB_SELF_CONTACT_OTHER_PARTS ? element_part[e] : 0;
    for (int j = lane; j < P.nv; j += 64) test_point(P, j, e, t, part, v, a, b);
  }
}

// A thread per surface vertex: its slot was taken
__global__ __launch_bounds__(kB) void k_sc_taken(int nv, const int* __restrict__ slot, unsigned char* __restrict__ flag) {
  const int v = blockIdx.x * kB + threadIdx.x;
  if (v < nv) flag[v] = slot[v] != INT_MAX ? 1 : 0;
}

__global__ __launch_bounds__(kB) void k_sc_iota(int n, int* __restrict__ out) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i < n) out[i] = i;
}

// A thread per boundary face: the part of its element
__global__ __launch_bounds__(kB) void k_sc_face_part(int nf, const int* __restrict__ face_tets, int n_tets, const int* __restrict__ element_part, int* __restrict__ face_part) {
  const int f = blockIdx.x * kB + threadIdx.x;
  if (f >= nf) return;
  const int e = face_tets[f];
  face_part[f] = (unsigned)e < (unsigned)n_tets ? element_part[e] : -1;
}

// ---- the closest face: body_contact.hip's k_bc_scan and k_bc_ring with the excluded faces skipped ----

// One wavefront per contact, every face in its own order, lanes striding.  only_far: the points the ring search flagged, the others
// keep their records.
__global__ __launch_bounds__(kB) void k_sc_scan(SearchDev S, FaceExclusion ex, int only_far, BodyContactRec* __restrict__ rec) {
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
// may take is a vote of the lanes.
__global__ __launch_bounds__(kB) void k_sc_ring(SearchDev S, FaceExclusion ex, GridDev g, FaceDev fg, long long budget, BodyContactRec* __restrict__ rec) {
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
      return __any(seen) != 0;
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
        // only have shortened it), and the wavefront walks the rows that hold a face
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
    if (bf == INT_MAX) far = true;  // (no face the point may take within the bound: the scan decides)
  }
  if (lane == 0) {
    bc_finish(S, t, vr, p, far ? INT_MAX : bf, tested, false, rec);
    if (far) rec[t].far = 1;
  }
}

// ---- forces ----

// A thread per contact: F, and the four records -- the point's node, then the three corners of the face
__global__ __launch_bounds__(kB) void k_sc_force(SearchDev S, double stiffness, double depth_cap, BodyContactRec* __restrict__ rec, uint32_t* __restrict__ keys,
                                                 uint32_t* __restrict__ vals) {
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= S.n_contacts) return;
  double p[3] = {0.0, 0.0, 0.0};
  const int vr = contact_point(S, t, p);
  BodyContactRec r = rec[t];
  const bool push = vr >= 0 && (unsigned)r.face < (unsigned)S.nf && r.d > 0.0;
  if (push) {
    const double depth = depth_cap > 0.0 ? fmin(r.d, depth_cap) : r.d;
    const double sd = stiffness * depth;
#pragma unroll
    for (int k = 0; k < 3; k++) rec[t].f[k] = sd * ((r.c[k] - p[k]) / r.d);
  } else {
    rec[t].d = 0.0;  // (nothing is pushed: degenerate, or no face left)
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int nd = !push ? S.n_nodes_t : k == 0 ? S.vnode[vr] : S.faces_int[3 * (size_t)r.face + (k - 1)];
    if ((unsigned)nd >= (unsigned)S.n_nodes_t) nd = S.n_nodes_t;  // (no node: sorted behind every node, and skipped)
    keys[4 * (size_t)t + k] = (uint32_t)nd;
    vals[4 * (size_t)t + k] = (uint32_t)(4 * t + k);
  }
}

// k_sc_force under the friction law (contact_friction.hip.h): the same push test and records, F the law's total from the velocities of
// the point's node and of the face's corners -- one body, one qvel array, internal order.  side[t]: N, |t|, t, -f; zero for a contact
// that pushes nothing.
__global__ __launch_bounds__(kB) void k_sc_force_friction(SearchDev S, double stiffness, double depth_cap, FrictionLaw law, const double* __restrict__ qvel,
                                                          BodyContactRec* __restrict__ rec, ContactFrictionRec* __restrict__ side, uint32_t* __restrict__ keys,
                                                          uint32_t* __restrict__ vals) {
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= S.n_contacts) return;
  double p[3] = {0.0, 0.0, 0.0};
  const int vr = contact_point(S, t, p);
  const BodyContactRec r = rec[t];
  const bool push = vr >= 0 && (unsigned)r.face < (unsigned)S.nf && r.d > 0.0;
  ContactFrictionRec o = {0.0, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (push) {
    double vp[3], vt[3][3], F[3];
    node_velocity(qvel, S.n_nodes_p, S.vnode[vr], vp);
#pragma unroll
    for (int k = 0; k < 3; k++) node_velocity(qvel, S.n_nodes_t, S.faces_int[3 * (size_t)r.face + k], vt[k]);
    contact_friction_law(p, r.c, r.b, r.d, stiffness, depth_cap, law, vp, vt, F, o);
#pragma unroll
    for (int k = 0; k < 3; k++) rec[t].f[k] = F[k];
  } else {
    rec[t].d = 0.0;  // (nothing is pushed: degenerate, or no face left)
  }
  side[t] = o;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int nd = !push ? S.n_nodes_t : k == 0 ? S.vnode[vr] : S.faces_int[3 * (size_t)r.face + (k - 1)];
    if ((unsigned)nd >= (unsigned)S.n_nodes_t) nd = S.n_nodes_t;  // (no node: sorted behind every node, and skipped)
    keys[4 * (size_t)t + k] = (uint32_t)nd;
    vals[4 * (size_t)t + k] = (uint32_t)(4 * t + k);
  }
}

// A thread per sorted record: the first of a node's segment does that node's additions in record order, however many they are
__global__ __launch_bounds__(kB) void k_sc_segments(int n_rec, const uint32_t* __restrict__ keys_s, const uint32_t* __restrict__ vals_s, int n_contacts, int n_nodes,
                                                    const BodyContactRec* __restrict__ rec, double* __restrict__ fext) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_rec) return;
  const uint32_t node = keys_s[i];
  if (node >= (uint32_t)n_nodes || (i > 0 && keys_s[i - 1] == node)) return;
  double a[3] = {fext[3 * (size_t)node], fext[3 * (size_t)node + 1], fext[3 * (size_t)node + 2]};
  for (int k = i; k < n_rec && keys_s[k] == node; k++) {
    const uint32_t v = vals_s[k];
    const uint32_t t = v / 4u, which = v % 4u;
    if (t >= (uint32_t)n_contacts) continue;
    const BodyContactRec& r = rec[t];
    if (!(r.d > 0.0)) continue;
    if (which == 0) {
      a[0] += r.f[0]; a[1] += r.f[1]; a[2] += r.f[2];
    } else {
      const double w = r.b[which - 1];
      a[0] += (-r.f[0]) * w; a[1] += (-r.f[1]) * w; a[2] += (-r.f[2]) * w;
    }
  }
  fext[3 * (size_t)node] = a[0]; fext[3 * (size_t)node + 1] = a[1]; fext[3 * (size_t)node + 2] = a[2];
}

// ---- host ----

// the stages of fb_fem_time_self_contact: events around each, on the handle's stream
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

// FEMBRAIN_SELF_CONTACT, read at every call: FB_BODY_CONTACT_SCAN / _RING, 0 where it is not set
int path_knob() {
  const char* env = getenv("FEMBRAIN_SELF_CONTACT");
  if (!env || !*env) return FB_BODY_CONTACT_NONE;
  if (!strcmp(env, "scan")) return FB_BODY_CONTACT_SCAN;
  if (!strcmp(env, "ring")) return FB_BODY_CONTACT_RING;
  return FB_BODY_CONTACT_NONE;
}

int check_self(fb_fem_s* h, const fb_fem_self_contact_params* p) {
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_self_contact is for unsharded handles");
  if (!p) return fail(FB_EINVAL, "null self contact parameters");
  if (!std::isfinite(p->stiffness) || p->stiffness < 0.0) return fail(FB_EINVAL, "self contact stiffness %g", p->stiffness);
  if (!std::isfinite(p->depth_cap) || p->depth_cap < 0.0) return fail(FB_EINVAL, "self contact depth cap %g", p->depth_cap);
  if (p->mode != FB_SELF_CONTACT_ANY && p->mode != FB_SELF_CONTACT_OTHER_PARTS) return fail(FB_EINVAL, "self contact mode %d", p->mode);
  if (h->plan.n_global <= 0 || h->plan.n_global >= (1 << 28)) return fail(FB_EINVAL, "fb_fem_self_contact: %d nodes", h->plan.n_global);
  return FB_OK;
}

constexpr int kWideWorkgroups = 64;  // of k_sc_contain_wide: 256 wavefronts share the overflow list

// add: into the external force vector, the result kept for fb_fem_read_self_contact; else into scratch, nothing kept (seconds: the stages).
// fr: null for the frictionless call; else the friction call's parameters, fout its info.
int self_contact(fb_fem_s* h, const fb_fem_self_contact_params& prm, bool add, double* seconds, fb_fem_self_contact_info* out,
                 const fb_fem_contact_friction_params* fr = nullptr, fb_fem_contact_friction_info* fout = nullptr) {
  SelfContactWork& W = h->selfc;
  PlanWorkspace& ws = h->plan_ws;
  hipStream_t s = h->stream;
  const bool by_part = prm.mode == FB_SELF_CONTACT_OTHER_PARTS;
  fb_fem_self_contact_info I;
  memset(&I, 0, sizeof(I));
  // the surface and, where the mode asks for them, the labels belong to the current mesh
  FB_TRY(surface_current(h));
  if (by_part) {
    const int before = h->parts.n_builds;
    FB_TRY(parts_current(h));
    I.n_parts_builds = h->parts.n_builds - before;
  }
  for (auto& e : W.ev_t)
    if (!e) FB_HIP(hipEventCreate(&e));
  const SurfaceWork& SF = h->surf;
  const int n_nodes = h->plan.n_global, n_tets = h->plan.n_tets, nv = SF.n_vertices, nf = SF.n_faces;
  I.n_points = nv;
  Stages tm;
  tm.ev = W.ev_t; tm.s = s; tm.seconds = seconds;

  // ---- positions and box ----
  FB_TRY(tm.begin());
  const int nb = blocks_for(n_nodes);
  const size_t n_box = fr ? 7 : 6;  // (the friction call: behind the box the flag of a velocity that is not finite, read in the same wait)
  FB_TRY(W.cur.reserve((size_t)3 * n_nodes)); FB_TRY(W.box_part.reserve((size_t)6 * nb)); FB_TRY(W.boxes.reserve(n_box));
  FB_TRY(launch_1d(k_sc_positions, n_nodes, s, n_nodes, h->x0.p, h->q.p, W.cur.p, W.box_part.p));
  FB_TRY(launch_grid(k_box_final<double>, dim3(1), s, nb, W.box_part.p, W.boxes.p));
  if (fr) {
    FB_HIP(hipMemsetAsync(W.boxes.p + 6, 0, sizeof(double), s));
    FB_TRY(launch_1d(k_cf_finite, 3LL * n_nodes, s, 3LL * n_nodes, h->qvel.p, W.boxes.p + 6));
  }
  double box[7];
  box[6] = 0.0;
  FB_TRY(W.boxes.download(box, n_box, s));  // a host wait
  FB_TRY(tm.end(0));
  for (int k = 0; k < 6; k++)
    if (!std::isfinite(box[k])) return fail(FB_EINVAL, "fb_fem_self_contact: a position of the body is not finite");
  if (box[6] != 0.0) return fail(FB_EINVAL, "fb_fem_self_contact_friction: a velocity of the body is not finite");
  const bool nothing = nv <= 0 || nf <= 0 || n_tets <= 0 || (by_part && h->parts.n_parts < 2);  // (one part has nothing to meet: no grid, no write)
  std::vector<BodyContactRec> recs;
  std::vector<ContactFrictionRec> side;
  int n_found = 0;
  double* fext = h->fext.p;
  if (!add) {
    FB_TRY(W.scratch.reserve((size_t)3 * n_nodes));
    FB_TRY(W.scratch.zero(s));
    fext = W.scratch.p;
  }
  double ext_max = 0.0;
  for (int k = 0; k < 3; k++) ext_max = std::max(ext_max, box[3 + k] - box[k]);
  if (!(ext_max > 0.0)) ext_max = 1.0;
  const double pad = std::ldexp(ext_max, -30);  // (embed_grid_build's padding: far above the rounding of a determinant test)

  if (!nothing) {
    // ---- the grid of surface vertices, containment ----
    FB_TRY(tm.begin());
    GridDev pg = make_grid(box, box + 3, pad, nv);
    const int n_cells = pg.dim[0] * pg.dim[1] * pg.dim[2];
    FB_TRY(W.p_key.reserve((size_t)nv)); FB_TRY(W.p_key_s.reserve((size_t)nv)); FB_TRY(W.slot.reserve((size_t)nv)); FB_TRY(W.hit.reserve((size_t)nv));
    FB_TRY(W.p_cell.reserve((size_t)nv)); FB_TRY(W.p_cell_s.reserve((size_t)nv)); FB_TRY(W.p_v.reserve((size_t)nv)); FB_TRY(W.p_v_s.reserve((size_t)nv));
    FB_TRY(W.p_xyz.reserve((size_t)3 * nv));
    FB_TRY(W.cell_lo.reserve((size_t)n_cells)); FB_TRY(W.cell_hi.reserve((size_t)n_cells));
    FB_TRY(W.flag.reserve((size_t)std::max(nv, n_tets))); FB_TRY(W.wide.reserve((size_t)n_tets)); FB_TRY(W.counts.reserve(2));
    if (W.ident_n < (size_t)nv) {  // (growth may move the buffer: filled from the start)
      FB_TRY(W.ident.reserve((size_t)nv));
      FB_TRY(launch_1d(k_sc_iota, nv, s, nv, W.ident.p));
      W.ident_n = (size_t)nv;
    }
    const int* part_of_element = by_part ? h->parts.element_part.p : nullptr;
    FB_TRY(launch_1d(k_sc_point_keys, nv, s, nv, SF.vnode.p, SF.vertex_ids.p, n_nodes, W.cur.p, pg, prm.mode, by_part ? h->parts.node_part_out.p : nullptr, W.p_key.p,
                     W.p_cell.p, W.p_v.p, W.slot.p));
    FB_TRY(sort_pairs(ws.temp, s, W.p_cell.p, W.p_cell_s.p, W.p_v.p, W.p_v_s.p, (size_t)nv, (unsigned)bits_of((long long)n_cells + 1)));
    FB_HIP(hipMemsetAsync(W.cell_lo.p, 0, sizeof(int) * (size_t)n_cells, s));
    FB_HIP(hipMemsetAsync(W.cell_hi.p, 0, sizeof(int) * (size_t)n_cells, s));
    FB_TRY(launch_1d(k_run_bounds<>, (long long)nv, s, nv, W.p_cell_s.p, (uint32_t)n_cells, W.cell_lo.p, W.cell_hi.p));
    FB_TRY(launch_1d(k_sc_point_store, nv, s, nv, W.p_v_s.p, SF.vnode.p, n_nodes, W.cur.p, W.p_key.p, W.p_xyz.p, W.p_key_s.p));
    I.n_point_grid_builds = 1;
    const PointsDev PD = {nv, prm.mode, W.cell_lo.p, W.cell_hi.p, W.p_xyz.p, W.p_key_s.p, W.p_v_s.p, W.slot.p};
    FB_TRY(launch_1d(k_sc_contain, n_tets, s, n_tets, h->tets.p, W.cur.p, part_of_element, pg, PD, W.flag.p));
    FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.wide.p, W.counts.p, (size_t)n_tets));
    FB_TRY(launch_grid(k_sc_contain_wide, dim3(kWideWorkgroups), s, W.counts.p, W.wide.p, n_tets, h->tets.p, W.cur.p, part_of_element, pad, PD));
    FB_TRY(launch_1d(k_sc_taken, nv, s, nv, W.slot.p, W.flag.p));
    FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.hit.p, W.counts.p + 1, (size_t)nv));
    FB_TRY(W.counts.download(&n_found, 1, s, 1));  // a host wait
    if (n_found < 0 || n_found > nv) return fail(FB_EDEVICE, "self contact: %d contacts of %d surface vertices", n_found, nv);
    FB_TRY(tm.end(1));
  }

  if (n_found > 0) {
    // ---- the path, and the face grid where it is the ring's ----
    GridDev fgrid = make_grid(box, box + 3, pad, nf);
    const int knob = path_knob();
    const bool ring = knob != FB_BODY_CONTACT_SCAN && grid_covered(fgrid);  // (default: the ring wherever its proof holds)
    I.path = ring ? FB_BODY_CONTACT_RING : FB_BODY_CONTACT_SCAN;
    long long budget = nf;  // (a point that has tested as many faces as a scan tests gains nothing from going on)
    if (const char* env = getenv("FEMBRAIN_SELF_CONTACT_BUDGET"))
      if (*env) budget = std::max(0LL, atoll(env));
    FB_TRY(tm.begin());
    if (by_part) {
      FB_TRY(W.face_part.reserve((size_t)nf));
      FB_TRY(launch_1d(k_sc_face_part, nf, s, nf, SF.face_tets.p, n_tets, h->parts.element_part.p, W.face_part.p));
    }
    if (ring) {
      const int n_cells = fgrid.dim[0] * fgrid.dim[1] * fgrid.dim[2], nbf = blocks_for(nf);
      FB_TRY(W.f_cnt.reserve((size_t)n_cells + 1)); FB_TRY(W.f_start.reserve((size_t)n_cells + 1)); FB_TRY(W.f_face.reserve((size_t)nf));
      FB_TRY(W.f_tri.reserve((size_t)9 * nf)); FB_TRY(W.f_R.reserve((size_t)nbf + 1));
      FB_HIP(hipMemsetAsync(W.f_cnt.p, 0, sizeof(int) * ((size_t)n_cells + 1), s));
      FB_TRY(ws.keys.reserve(((size_t)nf + 1) / 2)); FB_TRY(ws.keys_s.reserve(((size_t)nf + 1) / 2)); FB_TRY(ws.vals.reserve((size_t)nf));
      uint32_t* ck = reinterpret_cast<uint32_t*>(ws.keys.p);
      uint32_t* ck_s = reinterpret_cast<uint32_t*>(ws.keys_s.p);
      FB_TRY(launch_1d(k_bc_face_keys, nf, s, nf, SF.faces_int.p, n_nodes, W.cur.p, fgrid, ck, ws.vals.p, W.f_cnt.p, W.f_R.p));
      FB_TRY(launch_grid(k_bc_R_final, dim3(1), s, nbf, W.f_R.p, W.f_R.p + nbf));
      FB_TRY(sort_pairs(ws.temp, s, ck, ck_s, ws.vals.p, reinterpret_cast<uint32_t*>(W.f_face.p), (size_t)nf, (unsigned)bits_of(n_cells)));
      FB_TRY(exclusive_scan(ws.temp, s, W.f_cnt.p, W.f_start.p, 0, (size_t)n_cells + 1));
      FB_TRY(launch_1d(k_bc_face_store, nf, s, nf, W.f_face.p, SF.faces_int.p, n_nodes, W.cur.p, W.f_tri.p));
      I.n_face_grid_builds = 1;
    }
    FB_TRY(tm.end(2));

    // ---- the closest faces ----
    FB_TRY(tm.begin());
    FB_TRY(W.rec.reserve((size_t)n_found));
    SearchDev S;
    S.n_contacts = n_found; S.hit = W.hit.p; S.cand = W.ident.p; S.vnode = SF.vnode.p; S.vertex_ids = SF.vertex_ids.p; S.c_elem = W.slot.p;
    S.n_cand = nv; S.nv = nv; S.n_nodes_p = n_nodes; S.cur_p = W.cur.p;
    S.nf = nf; S.n_nodes_t = n_nodes; S.faces_int = SF.faces_int.p; S.cur_t = W.cur.p;
    const FaceExclusion ex = {prm.mode, nf, SF.faces_int.p, by_part ? W.face_part.p : nullptr, W.p_key.p};
    if (ring) {
      const FaceDev fg = {W.f_start.p, W.f_face.p, W.f_tri.p, W.f_R.p + blocks_for(nf)};
      FB_TRY(launch_waves(k_sc_ring, n_found, s, S, ex, fgrid, fg, budget, W.rec.p));
      FB_TRY(launch_waves(k_sc_scan, n_found, s, S, ex, 1, W.rec.p));  // (the points past their budget or without a face; a wavefront of any other returns at once)
    } else {
      FB_TRY(launch_waves(k_sc_scan, n_found, s, S, ex, 0, W.rec.p));
    }
    FB_TRY(tm.end(3));

    // ---- forces ----
    FB_TRY(tm.begin());
    const size_t n_rec = (size_t)4 * n_found;
    FB_TRY(W.r_key.reserve(n_rec)); FB_TRY(W.r_key_s.reserve(n_rec)); FB_TRY(W.r_val.reserve(n_rec)); FB_TRY(W.r_val_s.reserve(n_rec));
    if (fr) {
      const FrictionLaw law = {fr->mu, fr->slip_speed, fr->damping};
      FB_TRY(W.fric.reserve((size_t)n_found));
      FB_TRY(launch_1d(k_sc_force_friction, n_found, s, S, prm.stiffness, prm.depth_cap, law, h->qvel.p, W.rec.p, W.fric.p, W.r_key.p, W.r_val.p));
    } else {
      FB_TRY(launch_1d(k_sc_force, n_found, s, S, prm.stiffness, prm.depth_cap, W.rec.p, W.r_key.p, W.r_val.p));
    }
    FB_TRY(sort_pairs(ws.temp, s, W.r_key.p, W.r_key_s.p, W.r_val.p, W.r_val_s.p, n_rec, (unsigned)bits_of((long long)n_nodes + 1)));
    FB_TRY(launch_1d(k_sc_segments, (long long)n_rec, s, (int)n_rec, W.r_key_s.p, W.r_val_s.p, n_found, n_nodes, W.rec.p, fext));
    recs.resize((size_t)n_found);
    if (fr) {
      side.resize((size_t)n_found);
      FB_HIP(hipMemcpyAsync(side.data(), W.fric.p, sizeof(ContactFrictionRec) * (size_t)n_found, hipMemcpyDeviceToHost, s));  // (the wait below covers it)
    }
    FB_TRY(W.rec.download(recs.data(), (size_t)n_found, s));  // a host wait
    FB_TRY(tm.end(4));
  }

  // the sums, in record order; a contact without a face is dropped here (it made no record that counts)
  std::vector<BodyContactRec> kept;
  std::vector<ContactFrictionRec> kept_side;
  kept.reserve(recs.size());
  for (size_t i = 0; i < recs.size(); i++) {
    const BodyContactRec& r = recs[i];
    I.faces_tested += r.tested;
    if (r.face < 0) continue;
    kept.push_back(r);
    if (fr) kept_side.push_back(side[i]);
    if (!(r.d > 0.0)) { I.n_degenerate++; continue; }
    const double depth = prm.depth_cap > 0.0 ? std::min(r.d, prm.depth_cap) : r.d;
    I.max_depth = std::max(I.max_depth, depth);
    for (int k = 0; k < 3; k++) I.force_on_points[k] += r.f[k];
    for (int c = 0; c < 3; c++)
      for (int k = 0; k < 3; k++) I.force_on_faces[k] += (-r.f[k]) * r.b[c];
  }
  I.n_contacts = (int)kept.size();
  if (fr) {
    fb_fem_contact_friction_info FI;
    memset(&FI, 0, sizeof(FI));
    friction_sums(kept, kept_side, *fr, 0, FI);
    if (fout) *fout = FI;
  }
  if (add) {
    W.host.swap(kept);
    W.info = I;
    if (fr) W.fric_host.swap(kept_side);
  }
  if (out) *out = I;
  return FB_OK;
}

}  // namespace
}  // namespace fb

// ---- the C ABI ----

int fb_fem_self_contact(fb_fem_t h, const fb_fem_self_contact_params* p, fb_fem_self_contact_info* out) {
  CHECK_HANDLE(h);
  FB_TRY(check_self(h, p));
  return self_contact(h, *p, true, nullptr, out);
}

int fb_fem_self_contact_friction(fb_fem_t h, const fb_fem_self_contact_params* p, const fb_fem_contact_friction_params* fr, fb_fem_self_contact_info* out,
                                 fb_fem_contact_friction_info* fout) {
  CHECK_HANDLE(h);
  FB_TRY(check_self(h, p));
  FB_TRY(check_friction(fr, "fb_fem_self_contact_friction"));
  return self_contact(h, *p, true, nullptr, out, fr, fout);
}

int fb_fem_read_self_contact_friction(fb_fem_t h, double* normal_force, double* slip3, double* friction3) {
  CHECK_HANDLE(h);
  read_friction(h->selfc.fric_host, normal_force, slip3, friction3);
  return FB_OK;
}

int fb_fem_read_self_contact(fb_fem_t h, int* node, int* element, int* face, double* closest_xyz, double* bary3, double* depth) {
  CHECK_HANDLE(h);
  const std::vector<BodyContactRec>& v = h->selfc.host;
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

int fb_fem_time_self_contact(fb_fem_t h, const fb_fem_self_contact_params* p, int reps, double seconds[5]) {
  CHECK_HANDLE(h);
  FB_TRY(check_self(h, p));
  if (reps < 1 || !seconds) return fail(FB_EINVAL, "fb_fem_time_self_contact: reps must be positive and seconds not null");
  FB_TRY(self_contact(h, *p, false, nullptr, nullptr));  // warm: the buffers exist, the labels are current
  double sum[5] = {0, 0, 0, 0, 0};
  for (int r = 0; r < reps; r++) FB_TRY(self_contact(h, *p, false, sum, nullptr));
  for (int k = 0; k < 5; k++) seconds[k] = sum[k] / reps;
  return FB_OK;
}
