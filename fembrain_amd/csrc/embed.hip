// Point sets bound to the handle's tet mesh (embed.h), hand-written for gfx950.
//
// Binding (the reference's rule, fp64 on the rest positions): w_i = D_i / D_0 with D_0 the element's determinant and D_i the same with vertex
// i replaced by the point (TetMesh::computeBarycentricWeights; the determinants in TetMesh::getTetDeterminant's operation order); the
// lowest-numbered element with four weights >= 0 contains the point; a point no element contains goes to the element with the closest
// centre (strict <, ascending ids) and counts as external.
//
// The reference scans every element for every point.  Here a uniform grid over the rest box holds, per cell, the elements whose (padded)
// box overlaps it: (cell, element) pairs are emitted in element order and sorted by a STABLE radix sort, so a cell's elements ascend and a
// point's loop stops at the first that contains it.  An element over more than kEmbedWideCells cells (the hull slivers of a Delaunay mesh)
// goes to an overflow list every point tests from LDS.  Points without a containing element are compacted and scan all centres, tiled
// through LDS, once.  No float atomics, no spinning; every loop is bounded by a count the host knows.
//
// Update: a thread per point gathers its four nodes through the internal ids and forms ((w0 p0 + w1 p1) + w2 p2) + w3 p3 in fp64, p = x0 + q;
// a second pass walks the point's triangles in ascending order (the incidence list is the 3 n_triangles corners sorted stably by point)
// and sums unit normals as fb_fem_surface_update does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_prims.hip.h"
#include "embed.h"
#include "embed_grid.hip.h"
#include "fem_handle.h"
#include "launch.hip.h"
#include "mesh_device.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

constexpr int kWideTile = 64;  // overflow elements per LDS tile

// (det3, tet_det and bary, the weights of a point in an element: embed_grid.hip.h)

// ---- the mesh box (fp64; the partials are folded by k_box_final<double>) ----
__global__ __launch_bounds__(kB) void k_node_box(int n_nodes, const double* __restrict__ x0, double* __restrict__ part) {
  const int i = blockIdx.x * kB + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n_nodes)
    for (int k = 0; k < 3; k++) lo[k] = hi[k] = x0[3 * (size_t)i + k];
  wg_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

// ---- the grid ----

// the cells the padded box of element e overlaps: lowest and highest cell per axis
__device__ __forceinline__ void tet_cells(const GridDev& g, const int4* __restrict__ tets, const double* __restrict__ x0, int e, int* c0, int* c1) {
  double v[4][3];
  load_tet(tets, x0, e, v);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double mn = fmin(fmin(v[0][k], v[1][k]), fmin(v[2][k], v[3][k])), mx = fmax(fmax(v[0][k], v[1][k]), fmax(v[2][k], v[3][k]));
    // (mn - pad is not below the grid's lower bound, the mesh box less the same padding: both roundings are monotone.  A coordinate that
    // is not a number would fail the comparison and give cell 0.)
    const double a = mn - g.pad, b = mx + g.pad;
    c0[k] = a >= g.lo[k] ? cell_of(g, k, a) : 0;
    c1[k] = b >= g.lo[k] ? cell_of(g, k, b) : 0;
    if (c1[k] < c0[k]) c1[k] = c0[k];
  }
}

// A thread per element: the cells its box overlaps, 0 for an element of the overflow list.  (One entry past the end: the scan leaves the total there.)
__global__ __launch_bounds__(kB) void k_grid_count(int n_tets, GridDev g, const int4* __restrict__ tets, const double* __restrict__ x0, int* __restrict__ cnt,
                                                   unsigned char* __restrict__ wide_flag) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e > n_tets) return;
  if (e == n_tets) { cnt[e] = 0; return; }
  int c0[3], c1[3];
  tet_cells(g, tets, x0, e, c0, c1);
  const long long n = (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  const bool wide = n > kEmbedWideCells;
  cnt[e] = wide ? 0 : (int)n;
  wide_flag[e] = wide ? 1 : 0;
}

// A thread per element: its (cell, element) pairs behind off[e]; at most kEmbedWideCells of them
__global__ __launch_bounds__(kB) void k_grid_emit(int n_tets, GridDev g, const int4* __restrict__ tets, const double* __restrict__ x0, const int* __restrict__ cnt,
                                                  const int* __restrict__ off, long long n_pairs, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets || cnt[e] == 0) return;
  int c0[3], c1[3];
  tet_cells(g, tets, x0, e, c0, c1);
  long long o = off[e];
  const long long end = o + cnt[e];  // (the count pass's own number: the two passes cannot disagree about the room)
  for (int z = c0[2]; z <= c1[2]; z++)
    for (int y = c0[1]; y <= c1[1]; y++)
      for (int x = c0[0]; x <= c1[0]; x++) {
        if (o >= end || o >= n_pairs) return;
        keys[o] = (uint32_t)((z * g.dim[1] + y) * g.dim[0] + x);
        vals[o] = (uint32_t)e;
        o++;
      }
}

// (the cells' runs in the sorted pairs: k_run_bounds, mesh_device.hip.h)

// ---- the search ----

// A thread per point.  In the point's cell the first element that contains it is the lowest; of the overflow list, staged in LDS tile by
// tile by the whole workgroup, only elements below that one are tested.  elem = -1 and need = 1 where nothing contains the point.
__global__ __launch_bounds__(kB) void k_locate(int n, const unsigned char* __restrict__ only, const double* __restrict__ loc, GridDev g, int n_tets, const int4* __restrict__ tets, const double* __restrict__ x0,
                                               int* __restrict__ elem, unsigned char* __restrict__ need) {
  const int i = blockIdx.x * kB + threadIdx.x;
  const bool active = i < n && (!only || only[i]);  // (only: the orphans of a change in place; the others keep their binding)
  double p[3] = {0, 0, 0};
  int best = INT_MAX;
  if (active) {
    p[0] = loc[3 * (size_t)i]; p[1] = loc[3 * (size_t)i + 1]; p[2] = loc[3 * (size_t)i + 2];
    // outside the grid's box there is no cell: decided on the coordinates, before any index is formed
    if (in_box(p, g.lo, g.hi)) {
      const int c = (cell_of(g, 2, p[2]) * g.dim[1] + cell_of(g, 1, p[1])) * g.dim[0] + cell_of(g, 0, p[0]);
      const int j1 = g.cell_hi[c];
      for (int j = g.cell_lo[c]; j < j1; j++) {
        const int e = g.cell_elem[j];
        if (e < 0 || e >= n_tets) continue;
        double v[4][3], w[4];
        load_tet(tets, x0, e, v);
        if (bary(v, p, w)) { best = e; break; }
      }
    }
  }
  __shared__ double tv[kWideTile][12];
  __shared__ int tid[kWideTile];
  for (int base = 0; base < g.n_wide; base += kWideTile) {
    const int m = min(kWideTile, g.n_wide - base);
    __syncthreads();  // (the tile before has been read)
    {
      const int j = threadIdx.x >> 2, k = threadIdx.x & 3;  // kB == 4 kWideTile: a thread per vertex
      if (j < m) {
        const int e = g.wide[base + j];
        const bool ok = e >= 0 && e < n_tets;
        if (k == 0) tid[j] = ok ? e : INT_MAX;
        const double* q = x0 + 3 * (size_t)tet_node(tets[ok ? e : 0], k);
        tv[j][3 * k] = q[0]; tv[j][3 * k + 1] = q[1]; tv[j][3 * k + 2] = q[2];
      }
    }
    __syncthreads();
    if (active)
      for (int j = 0; j < m; j++) {
        if (tid[j] >= best) break;  // (the list ascends)
        double w[4];
        if (bary(reinterpret_cast<const double(*)[3]>(tv[j]), p, w)) { best = tid[j]; break; }
      }
  }
  if (active) {
    elem[i] = best == INT_MAX ? -1 : best;
    need[i] = best == INT_MAX ? 1 : 0;
  } else if (i < n) {
    need[i] = 0;
  }
}
static_assert(kB == 4 * kWideTile, "k_locate stages a vertex per thread");

// A thread per point without a containing element and, along blockIdx.y, a chunk of the element list (chunk_len elements, a multiple of the
// tile): the chunk's centres, tile by tile from LDS (a thread per element computes it: the mean of the four vertices, summed in order and
// scaled by 1.0 / 4), distance sqrt(dx dx + dy dy + dz dz), strict < in ascending order.  The chunk's (distance, element) goes to
// part[chunk][t]; k_closest_final folds the chunks in ascending order under the same strict <, which is the element one pass over the
// whole list finds.  (A few outside points would otherwise make one workgroup walk every centre of the mesh alone.)
__global__ __launch_bounds__(kB) void k_closest(int n_ext, const int* __restrict__ ext_ids, int n, const double* __restrict__ loc, int n_tets, int chunk_len,
                                                const int4* __restrict__ tets, const double* __restrict__ x0, double* __restrict__ part_d, int* __restrict__ part_e) {
  const int t = blockIdx.x * kB + threadIdx.x;
  int i = t < n_ext ? ext_ids[t] : -1;
  if (i >= n) i = -1;
  double p[3] = {0, 0, 0};
  if (i >= 0) { p[0] = loc[3 * (size_t)i]; p[1] = loc[3 * (size_t)i + 1]; p[2] = loc[3 * (size_t)i + 2]; }
  double best = DBL_MAX;
  int be = 0;
  const long long first = (long long)blockIdx.y * chunk_len;
  const int end = (int)min((long long)n_tets, first + chunk_len);
  __shared__ double sc[kB][3];
  for (long long base = first; base < end; base += kB) {
    const int m = min(kB, end - (int)base);
    __syncthreads();
    if ((int)threadIdx.x < m) {
      double v[4][3];
      load_tet(tets, x0, (int)base + threadIdx.x, v);
      tet_centre(v, sc[threadIdx.x]);
    }
    __syncthreads();
    if (i >= 0)
      for (int j = 0; j < m; j++) {
        const double d = centre_distance(p, sc[j]);
        if (d < best) { best = d; be = (int)base + j; }
      }
  }
  if (t < n_ext) {
    part_d[(size_t)blockIdx.y * n_ext + t] = best;
    part_e[(size_t)blockIdx.y * n_ext + t] = be;
  }
}

__global__ __launch_bounds__(kB) void k_closest_final(int n_ext, int n_chunks, const double* __restrict__ part_d, const int* __restrict__ part_e, const int* __restrict__ ext_ids,
                                                      int n, int* __restrict__ elem) {
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= n_ext) return;
  const int i = ext_ids[t];
  if (i < 0 || i >= n) return;
  double best = DBL_MAX;
  int be = 0;
  for (int c = 0; c < n_chunks; c++) {
    const double d = part_d[(size_t)c * n_ext + t];
    if (d < best) { best = d; be = part_e[(size_t)c * n_ext + t]; }
  }
  elem[i] = be;
}

// A thread per point: weights and vertices of its element; zero_threshold > 0: four zero weights for a point farther than that from every
// vertex of its element.  changed: the element differs from the binding before (null: not asked).
__global__ __launch_bounds__(kB) void k_bind(int n, const unsigned char* __restrict__ only, const double* __restrict__ loc, const int* __restrict__ elem, const unsigned char* __restrict__ need, int n_tets,
                                             const int4* __restrict__ tets, const double* __restrict__ x0, const int* __restrict__ caller_of, double zero_threshold,
                                             const int* __restrict__ elem_old, double* __restrict__ w4, int* __restrict__ vert, int* __restrict__ vert_int,
                                             unsigned char* __restrict__ ext, unsigned char* __restrict__ zeroed, unsigned char* __restrict__ changed) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  if (only && !only[i]) {
    if (changed) changed[i] = 0;
    return;
  }
  int e = elem[i];
  if (e < 0 || e >= n_tets) e = 0;  // (k_closest has given every such point an element; a mesh without elements does not get here)
  const double p[3] = {loc[3 * (size_t)i], loc[3 * (size_t)i + 1], loc[3 * (size_t)i + 2]};
  const int4 t = tets[e];
  double v[4][3], w[4];
  load_tet(tets, x0, e, v);
  bary(v, p, w);
  unsigned char z = 0;
  if (zero_threshold > 0) {
    double dmin = DBL_MAX;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double dx = v[k][0] - p[0], dy = v[k][1] - p[1], dz = v[k][2] - p[2];
      const double d = sqrt(dx * dx + dy * dy + dz * dz);
      if (d < dmin) dmin = d;
    }
    if (dmin > zero_threshold) { z = 1; w[0] = w[1] = w[2] = w[3] = 0.0; }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int nd = tet_node(t, k);
    w4[4 * (size_t)i + k] = w[k];
    vert_int[4 * (size_t)i + k] = nd;
    vert[4 * (size_t)i + k] = caller_of ? caller_of[nd] : nd;
  }
  ext[i] = need[i];
  zeroed[i] = z;
  if (changed) changed[i] = only || elem_old[i] != e ? 1 : 0;  // (an orphan had no element in this mesh)
}

// A thread per point: the binding carried across a change of the mesh in place (embed.h, embed_follow)
__global__ __launch_bounds__(kB) void k_follow(int n, int n_tets_old, const unsigned char* __restrict__ estate, const int* __restrict__ pos, int n_kept, int n_cut,
                                               const int* __restrict__ cut_tets, const int* __restrict__ piece_off, const int* __restrict__ pcount, int n_tets, int n_nodes,
                                               const int4* __restrict__ tets, const double* __restrict__ x0, const int* __restrict__ caller_of,
                                               const int* __restrict__ internal_of, int bake, int* __restrict__ elem, double* __restrict__ w4, int* __restrict__ vert,
                                               int* __restrict__ vert_int, double* __restrict__ loc, const unsigned char* __restrict__ zeroed,
                                               unsigned char* __restrict__ orphan, unsigned char* __restrict__ changed) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  changed[i] = 0;
  if (orphan[i]) return;  // (it waits for a search already: its element went with an earlier change)
  const int e = elem[i];
  int vi[4];
  bool ok = e >= 0 && e < n_tets_old;
#pragma unroll
  for (int k = 0; k < 4; k++) {  // the parent's nodes in the new internal order: the caller's ids of old nodes never change
    const int c = vert[4 * (size_t)i + k];
    vi[k] = c >= 0 && c < n_nodes ? (internal_of ? internal_of[c] : c) : -1;
    if (vi[k] < 0 || vi[k] >= n_nodes) ok = false;
  }
  const unsigned char st = ok ? estate[e] : 2;
  const bool z = zeroed[i] != 0;  // (four zero weights say nothing about where the point is: its loc stands)
  double p[3] = {loc[3 * (size_t)i], loc[3 * (size_t)i + 1], loc[3 * (size_t)i + 2]};
  if (ok && !z && (bake || st == 1)) {
    const double w[4] = {w4[4 * (size_t)i], w4[4 * (size_t)i + 1], w4[4 * (size_t)i + 2], w4[4 * (size_t)i + 3]};
#pragma unroll
    for (int c = 0; c < 3; c++)
      p[c] = ((w[0] * x0[3 * (size_t)vi[0] + c] + w[1] * x0[3 * (size_t)vi[1] + c]) + w[2] * x0[3 * (size_t)vi[2] + c]) + w[3] * x0[3 * (size_t)vi[3] + c];
  }
  if (st == 0) {  // kept: the new id, the weights as they are
    elem[i] = pos[e];
#pragma unroll
    for (int k = 0; k < 4; k++) vert_int[4 * (size_t)i + k] = vi[k];
    if (bake && !z)
      for (int c = 0; c < 3; c++) loc[3 * (size_t)i + c] = p[c];
    return;
  }
  if (st == 1 && n_cut > 0) {  // removed: one of the cut's parents?
    int lo = 0, hi = n_cut - 1, j = -1;
    while (lo <= hi) {
      const int mid = (lo + hi) >> 1;
      const int c = cut_tets[mid];
      if (c == e) { j = mid; break; }
      if (c < e) lo = mid + 1; else hi = mid - 1;
    }
    if (j >= 0) {
      const int first = n_kept + piece_off[j];
      const int cnt = min(pcount[j], 8);  // (4 or 6)
      if (first >= 0 && cnt > 0 && first + cnt <= n_tets) {
        int best = -1, bc = first;
        double bd = DBL_MAX, v[4][3], w[4];
        for (int m = 0; m < cnt; m++) {
          load_tet(tets, x0, first + m, v);
          if (bary(v, p, w)) { best = first + m; break; }
          const double dx = p[0] - (((v[0][0] + v[1][0]) + v[2][0]) + v[3][0]) * (1.0 / 4), dy = p[1] - (((v[0][1] + v[1][1]) + v[2][1]) + v[3][1]) * (1.0 / 4),
                       dz = p[2] - (((v[0][2] + v[1][2]) + v[2][2]) + v[3][2]) * (1.0 / 4);
          const double d = sqrt(dx * dx + dy * dy + dz * dz);
          if (d < bd) { bd = d; bc = first + m; }
        }
        if (best < 0) {
          best = bc;
          load_tet(tets, x0, best, v);
          bary(v, p, w);
        }
        const int4 t = tets[best];
        elem[i] = best;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int nd = tet_node(t, k);
          w4[4 * (size_t)i + k] = z ? 0.0 : w[k];
          vert_int[4 * (size_t)i + k] = nd;
          vert[4 * (size_t)i + k] = caller_of ? caller_of[nd] : nd;
        }
        if (!z)
          for (int c = 0; c < 3; c++) loc[3 * (size_t)i + c] = p[c];
        changed[i] = 1;
        return;
      }
    }
  }
  // removed without pieces, or changed in place: an orphan.  Nothing reads its binding before the search; node 0 with weight 0 is safe anyway
  orphan[i] = 1;
#pragma unroll
  for (int k = 0; k < 4; k++) { w4[4 * (size_t)i + k] = 0.0; vert_int[4 * (size_t)i + k] = 0; }
}

// one workgroup: the sums of up to three byte arrays (integer sums: any order)
__global__ __launch_bounds__(kB) void k_flag_sums(int n, const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, const unsigned char* __restrict__ c,
                                                  int* __restrict__ out3) {
  int s[3] = {0, 0, 0};
  for (int i = threadIdx.x; i < n; i += kB) { s[0] += a ? a[i] : 0; s[1] += b ? b[i] : 0; s[2] += c ? c[i] : 0; }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int r = wg_sum(s[k]);
    if (threadIdx.x == 0) out3[k] = r;
  }
}

// ---- the incidence list ----
// (an index outside [0, n) -- a list handed over on the device is not checked on the host -- gets the key n: behind every point's run, where
// k_run_bounds drops it; the sort looks at bits_of(n + 1) bits)
__global__ __launch_bounds__(kB) void k_tri_corner_keys(int n_corners, int n, const int* __restrict__ tris, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_corners) return;
  const int v = tris[j];
  keys[j] = (unsigned)v < (unsigned)n ? (uint32_t)v : (uint32_t)n;
  vals[j] = (uint32_t)j;
}

// ---- the update ----

// A thread per point: its fp64 position (kept for the normals), the float of it, the workgroup's box
__global__ __launch_bounds__(kB) void k_embed_pos(int n, int n_nodes, const int* __restrict__ vert_int, const double* __restrict__ w4, const double* __restrict__ x0,
                                                  const double* __restrict__ q, double* __restrict__ cur, float* __restrict__ xyz, float* __restrict__ part) {
  const int i = blockIdx.x * kB + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n) {
    double s[3];
    embed_point(i, n_nodes, vert_int, w4, x0, q, s);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      cur[3 * (size_t)i + c] = s[c];
      const float f = (float)s[c];
      xyz[3 * (size_t)i + c] = f;
      lo[c] = hi[c] = f;
    }
  }
  wg_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

// A thread per point: the normalised fp64 sum of the unit normals of its triangles, ascending; zero where there is none
__global__ __launch_bounds__(kB) void k_embed_normals(int n, int n_triangles, const int* __restrict__ inc_lo, const int* __restrict__ inc_hi, const uint32_t* __restrict__ inc,
                                                      const int* __restrict__ tris, const double* __restrict__ cur, float* __restrict__ normals) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  double sum[3] = {0.0, 0.0, 0.0};
  const int j1 = n_triangles ? inc_hi[i] : 0;
  for (int j = n_triangles ? inc_lo[i] : 0; j < j1; j++) {
    const uint32_t tr = inc[j] / 3u;
    if (tr >= (uint32_t)n_triangles) continue;
    const int* f = tris + 3 * (size_t)tr;
    if ((unsigned)f[0] >= (unsigned)n || (unsigned)f[1] >= (unsigned)n || (unsigned)f[2] >= (unsigned)n) continue;  // (a list handed over on the device)
    double p[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const size_t b = 3 * (size_t)f[c];
#pragma unroll
      for (int k = 0; k < 3; k++) p[c][k] = cur[b + k];
    }
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double nn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double len = sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
    if (len > 0.0) { sum[0] += nn[0] / len; sum[1] += nn[1] / len; sum[2] += nn[2] / len; }  // (a triangle without area has no normal)
  }
  const double len = sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
#pragma unroll
  for (int k = 0; k < 3; k++) normals[3 * (size_t)i + k] = len > 0.0 ? (float)(sum[k] / len) : 0.0f;
}

}  // namespace

void Embedding::release_all() {
  loc.release(); w.release(); elem.release(); elem_old.release(); vert.release(); vert_int.release(); ext.release(); zeroed.release(); need.release(); changed.release(); orphan.release();
  tris.release(); inc.release(); inc_lo.release(); inc_hi.release(); cur.release(); out.release(); part.release();
  tr_corner.release(); tr_lo.release(); tr_hi.release(); tr_nodes.release(); tr_flag.release(); f_stage.release(); f_mask.release();
  host.clear(); host.shrink_to_fit();
  live = orphan_all = lost = tr_valid = false;
  tr_builds = tr_longest = tr_touched = 0;
  n_points = n_triangles = n_external = n_zeroed = n_locates = n_rebound = n_orphans = 0;
  search = EmbedSearchStats();
}

int embed_grid_build(hipStream_t s, EmbedGrid& G, const EmbedMesh& M, PlanWorkspace& W) {
  G.valid = false;
  if (M.n_tets <= 0 || M.n_nodes <= 0) return fail(FB_EINVAL, "embedding: the mesh has no elements");
  // the box of the rest positions
  const int nblk = blocks_for(M.n_nodes);
  FB_TRY(G.box_part.alloc((size_t)6 * nblk + 6));
  FB_TRY(launch_1d(k_node_box, M.n_nodes, s, M.n_nodes, M.x0, G.box_part.p));
  FB_TRY(launch_grid(k_box_final<double>, dim3(1), s, nblk, G.box_part.p, G.box_part.p + 6 * (size_t)nblk));
  double box[6];
  FB_TRY(G.box_part.download(box, 6, s, (size_t)6 * nblk));  // the first host wait
  double ext_max = 0.0;
  for (int k = 0; k < 3; k++) {
    if (!std::isfinite(box[k]) || !std::isfinite(box[3 + k])) return fail(FB_EINVAL, "embedding: a rest position of the mesh is not finite");
    ext_max = std::max(ext_max, box[3 + k] - box[k]);
  }
  if (!(ext_max > 0.0)) ext_max = 1.0;
  // Padding far above the rounding of a determinant test (2^-30 of the extent against 2^-52): a point an element contains up to rounding
  // lies inside that element's padded box, so its cell is one of the element's.
  G.pad = std::ldexp(ext_max, -30);
  double ext[3], vol = 1.0;
  for (int k = 0; k < 3; k++) {
    G.lo[k] = box[k] - G.pad; G.hi[k] = box[3 + k] + G.pad;
    ext[k] = G.hi[k] - G.lo[k];
    vol *= ext[k];
  }
  // of the order of one cell per element
  const double hcell = std::cbrt(vol / M.n_tets);
  long long cells = 1;
  for (int k = 0; k < 3; k++) {
    const double d = hcell > 0.0 ? std::ceil(ext[k] / hcell) : 1.0;
    G.dim[k] = d >= 1024.0 ? 1024 : d >= 1.0 ? (int)d : 1;
    cells *= G.dim[k];
  }
  const long long cell_cap = std::max<long long>(64, 8LL * M.n_tets);  // (a flat box: the cube-root rule alone would over-resolve its long sides)
  while (cells > cell_cap) {
    const int k = G.dim[0] >= G.dim[1] && G.dim[0] >= G.dim[2] ? 0 : G.dim[1] >= G.dim[2] ? 1 : 2;
    G.dim[k] = (G.dim[k] + 1) / 2;
    cells = (long long)G.dim[0] * G.dim[1] * G.dim[2];
  }
  for (int k = 0; k < 3; k++) G.inv[k] = G.dim[k] / ext[k];
  const int n_cells = (int)cells;

  FB_TRY(G.cnt.alloc((size_t)M.n_tets + 1)); FB_TRY(G.off.alloc((size_t)M.n_tets + 1)); FB_TRY(G.wide_flag.alloc((size_t)M.n_tets));
  FB_TRY(G.wide.alloc((size_t)M.n_tets)); FB_TRY(G.wide_count.alloc(1));
  FB_TRY(G.cell_lo.alloc((size_t)n_cells)); FB_TRY(G.cell_hi.alloc((size_t)n_cells));
  GridDev g = grid_dev(G);
  FB_TRY(launch_1d(k_grid_count, M.n_tets + 1, s, M.n_tets, g, M.tets, M.x0, G.cnt.p, G.wide_flag.p));
  FB_TRY(exclusive_scan(W.temp, s, G.cnt.p, G.off.p, 0, (size_t)M.n_tets + 1));
  FB_TRY(select_flagged(W.temp, s, rocprim::counting_iterator<int>(0), G.wide_flag.p, G.wide.p, G.wide_count.p, (size_t)M.n_tets));
  int total = 0, n_wide = 0;
  FB_HIP(hipMemcpyAsync(&total, G.off.p + M.n_tets, sizeof(int), hipMemcpyDeviceToHost, s));
  FB_HIP(hipMemcpyAsync(&n_wide, G.wide_count.p, sizeof(int), hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));  // the second host wait
  if (total < 0 || (long long)total > (long long)kEmbedWideCells * M.n_tets || n_wide < 0 || n_wide > M.n_tets)
    return fail(FB_EDEVICE, "embedding grid: %d pairs, %d wide elements out of range", total, n_wide);
  G.n_pairs = total;
  G.n_wide = n_wide;
  FB_TRY(G.cell_lo.zero(s)); FB_TRY(G.cell_hi.zero(s));
  FB_TRY(G.cell_elem.alloc((size_t)std::max(total, 1)));
  if (total) {
    // (the sort's arrays are the plan builder's: it is not running, every build is an entry point of its own on the handle's stream)
    FB_TRY(W.keys.reserve(((size_t)total + 1) / 2)); FB_TRY(W.keys_s.reserve(((size_t)total + 1) / 2)); FB_TRY(W.vals.reserve((size_t)total));
    uint32_t* ck = reinterpret_cast<uint32_t*>(W.keys.p);
    uint32_t* ck_s = reinterpret_cast<uint32_t*>(W.keys_s.p);
    FB_TRY(launch_1d(k_grid_emit, M.n_tets, s, M.n_tets, g, M.tets, M.x0, G.cnt.p, G.off.p, (long long)total, ck, W.vals.p));
    FB_TRY(sort_pairs(W.temp, s, ck, ck_s, W.vals.p, reinterpret_cast<uint32_t*>(G.cell_elem.p), (size_t)total, (unsigned)bits_of(n_cells)));
    FB_TRY(launch_1d(k_run_bounds<>, (long long)total, s, total, ck_s, (uint32_t)n_cells, G.cell_lo.p, G.cell_hi.p));
  }
  G.valid = true;
  G.n_builds++;
  return FB_OK;
}

int embed_locate(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, bool count_rebound, PlanWorkspace& W) {
  int n_ext = 0;
  FB_TRY(embed_locate_search(s, EW, E, M, count_rebound, W, &n_ext));
  return embed_locate_finish(s, EW, E, M, count_rebound, W, n_ext);
}

int embed_locate_search(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, bool count_rebound, PlanWorkspace& W, int* n_ext_out) {
  const int n = E.n_points;
  const EmbedGrid& G = EW.grid;
  if (!G.valid) return fail(FB_EDEVICE, "embedding: no search grid");
  FB_TRY(E.elem.alloc((size_t)n)); FB_TRY(E.w.alloc((size_t)4 * n)); FB_TRY(E.vert.alloc((size_t)4 * n)); FB_TRY(E.vert_int.alloc((size_t)4 * n));
  FB_TRY(E.ext.alloc((size_t)n)); FB_TRY(E.zeroed.alloc((size_t)n)); FB_TRY(E.need.alloc((size_t)n));
  FB_TRY(EW.ext_ids.reserve((size_t)n)); FB_TRY(EW.counts.reserve(4));
  if (count_rebound) {
    FB_TRY(E.elem_old.alloc((size_t)n)); FB_TRY(E.changed.alloc((size_t)n));
    FB_HIP(hipMemcpyAsync(E.elem_old.p, E.elem.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, s));
  }
  const unsigned char* only = E.orphan_all || !E.n_orphans ? nullptr : E.orphan.p;
  FB_TRY(launch_1d(k_locate, n, s, n, only, E.loc.p, grid_dev(G), M.n_tets, M.tets, M.x0, E.elem.p, E.need.p));
  FB_TRY(select_flagged(W.temp, s, rocprim::counting_iterator<int>(0), E.need.p, EW.ext_ids.p, EW.counts.p, (size_t)n));
  int n_ext = 0;
  FB_TRY(EW.counts.download(&n_ext, 1, s));  // the host wait
  if (n_ext < 0 || n_ext > n) return fail(FB_EDEVICE, "embedding: %d points without an element out of range", n_ext);
  *n_ext_out = n_ext;
  return FB_OK;
}

namespace {
// the full scan for the n_list points of `ids`: every centre of the mesh for each
int closest_scan(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, int n_list, const int* ids) {
  // about 2048 workgroups in all: few outside points get many short chunks, many points few long ones (at most 2048 x 256 partial minima)
  const int bx = ceil_div(n_list, kB), tiles = ceil_div(M.n_tets, kB);
  const int n_chunks = std::max(1, std::min(tiles, 2048 / bx));
  const int chunk_len = ceil_div(tiles, n_chunks) * kB;
  const int used = ceil_div(M.n_tets, chunk_len);  // (chunks that hold an element)
  FB_TRY(EW.close_d.reserve((size_t)used * n_list)); FB_TRY(EW.close_e.reserve((size_t)used * n_list));
  FB_TRY(launch_grid(k_closest, dim3((unsigned)bx, (unsigned)used), s, n_list, ids, E.n_points, E.loc.p, M.n_tets, chunk_len, M.tets, M.x0, EW.close_d.p, EW.close_e.p));
  return launch_1d(k_closest_final, n_list, s, n_list, used, EW.close_d.p, EW.close_e.p, ids, E.n_points, E.elem.p);
}

// The automatic rule of the external pass, measured on the MI355X with tools/probe_embed.py --outside (profiles/embed_probe_outside.json;
// medians of HIP-event timings, the ring's figure with its host wait, the centre grid built beforehand):
// the sphere surface scaled to enclose the cantilever, every vertex outside, the first n_ext of a shuffle of its 38,958 vertices):
//
//            |        998,250 tets (grid 100^3)       |        105,456 tets (grid 48^3)
//    n_ext   |  scan      ring     (ring + build)/scan |  scan      ring     (ring + build)/scan
//        12  |  0.53 ms   4.00 ms   8.0                |  0.15 ms   1.02 ms   7.5
//       256  |  0.86 ms   5.60 ms   6.8                |  0.16 ms   1.32 ms   8.7
//     1,024  |  1.28 ms   4.62 ms   3.8                |  0.24 ms   1.15 ms   5.2
//     4,096  |  4.14 ms   4.89 ms   1.24               |  0.53 ms   1.21 ms   2.4
//    16,384  | 15.5  ms   9.11 ms   0.60               |  1.85 ms   2.09 ms   1.17
//    38,958  | 36.9  ms   8.15 ms   0.23               |  4.07 ms   2.13 ms   0.54
//    centre grid build: 0.24 ms | 0.076 ms
//
// The ring has a floor of a few milliseconds here whatever the count: this surface is up to 40 cells away from the body, the cap of the
// ball that reaches into the grid covers hundreds of rows, and one wavefront walks them one after another, a few dependent loads each.
// The two passes cost the same at about 7,000 outside points at 1M tets and about 20,000 at 105k tets.  kRingMinOutside = 8,192: below
// it a search on a mesh generation without a centre grid scans; between 8,192 and 20,000 points at 105k tets that costs under a
// millisecond.  With a grid in place the ring is taken at any count.
// The budget: the ring pass tested 96 M centres in 8.15 ms (85 ps each, 2,473 per point), the scan 38.9 G pairs in 36.9 ms (0.95 ps each),
// so a wavefront that has tested n_tets / 89 centres has cost what the scan costs for its point.  max(64, n_tets / 32): a point is given up
// at three times that, and costs under four scans in all.  No point of the probe came near it (the most one tested: 10,200, against 31,195).
constexpr int kRingMinOutside = 8192;
constexpr long long kRingBudgetFloor = 64, kRingBudgetDivisor = 32;
}  // namespace

int embed_closest_choice(const EmbedWork& EW, const EmbedMesh& M, int n_ext, long long* budget) {
  // (read at every search, like FEMBRAIN_PARTS_WIDE_KEYS: a process may switch between two searches)
  const char* b = getenv("FEMBRAIN_EMBED_RING_BUDGET");
  const long long asked = b ? atoll(b) : 0;
  *budget = asked > 0 ? asked : std::max(kRingBudgetFloor, (long long)M.n_tets / kRingBudgetDivisor);
  if (!embed_ring_covers(EW.grid)) return FB_EMBED_CLOSEST_SCAN;
  const char* c = getenv("FEMBRAIN_EMBED_CLOSEST");
  if (c && !strcmp(c, "scan")) return FB_EMBED_CLOSEST_SCAN;
  if (c && !strcmp(c, "ring")) return FB_EMBED_CLOSEST_RING;
  return EW.cgrid.valid || n_ext >= kRingMinOutside ? FB_EMBED_CLOSEST_RING : FB_EMBED_CLOSEST_SCAN;
}

int embed_closest(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, PlanWorkspace& W, int n_ext, int path, long long budget) {
  E.search = EmbedSearchStats();
  if (!n_ext) return FB_OK;
  if (path == FB_EMBED_CLOSEST_RING) {
    int n_far = 0;
    FB_TRY(embed_closest_ring(s, EW, E, M, W, n_ext, budget, &n_far));
    if (n_far) FB_TRY(closest_scan(s, EW, E, M, n_far, EW.far_ids.p));
    E.search.tested += (long long)n_far * M.n_tets;
    return FB_OK;
  }
  FB_TRY(closest_scan(s, EW, E, M, n_ext, EW.ext_ids.p));
  E.search.path = FB_EMBED_CLOSEST_SCAN;
  E.search.n_outside = E.search.n_far = n_ext;
  E.search.max_one = M.n_tets;
  E.search.tested = (long long)n_ext * M.n_tets;
  return FB_OK;
}

int embed_locate_finish(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, bool count_rebound, PlanWorkspace& W, int n_ext) {
  const int n = E.n_points;
  const unsigned char* only = E.orphan_all || !E.n_orphans ? nullptr : E.orphan.p;
  long long budget = 0;
  const int path = embed_closest_choice(EW, M, n_ext, &budget);
  FB_TRY(embed_closest(s, EW, E, M, W, n_ext, path, budget));
  FB_TRY(launch_1d(k_bind, n, s, n, only, E.loc.p, E.elem.p, E.need.p, M.n_tets, M.tets, M.x0, M.caller_of, E.zero_threshold, count_rebound ? E.elem_old.p : nullptr, E.w.p, E.vert.p,
                   E.vert_int.p, E.ext.p, E.zeroed.p, count_rebound ? E.changed.p : nullptr));
  FB_TRY(launch_grid(k_flag_sums, dim3(1), s, n, E.ext.p, E.zeroed.p, count_rebound ? E.changed.p : nullptr, EW.counts.p + 1));
  int c[3] = {0, 0, 0};
  FB_TRY(EW.counts.download(c, 3, s, 1));
  E.n_external = c[0];
  E.n_zeroed = c[1];
  if (count_rebound) E.n_rebound += c[2];
  E.n_locates++;
  E.orphan_all = false;
  E.n_orphans = 0;
  E.tr_valid = false;  // (the transposed table is of the binding before)
  return FB_OK;
}

int embed_incidence(hipStream_t s, Embedding& E, PlanWorkspace& W) {
  const int n = E.n_points, nc = 3 * E.n_triangles;
  if (!nc) return FB_OK;
  FB_TRY(E.inc.alloc((size_t)nc)); FB_TRY(E.inc_lo.alloc((size_t)n)); FB_TRY(E.inc_hi.alloc((size_t)n));
  FB_TRY(E.inc_lo.zero(s)); FB_TRY(E.inc_hi.zero(s));
  FB_TRY(W.keys.reserve(((size_t)nc + 1) / 2)); FB_TRY(W.keys_s.reserve(((size_t)nc + 1) / 2)); FB_TRY(W.vals.reserve((size_t)nc));
  uint32_t* ck = reinterpret_cast<uint32_t*>(W.keys.p);
  uint32_t* ck_s = reinterpret_cast<uint32_t*>(W.keys_s.p);
  FB_TRY(launch_1d(k_tri_corner_keys, nc, s, nc, n, E.tris.p, ck, W.vals.p));
  // the corners sorted stably by point keep their ascending triangle order
  FB_TRY(sort_pairs(W.temp, s, ck, ck_s, W.vals.p, E.inc.p, (size_t)nc, (unsigned)bits_of((long long)n + 1)));
  return launch_1d(k_run_bounds<>, (long long)nc, s, nc, ck_s, (uint32_t)n, E.inc_lo.p, E.inc_hi.p);
}

int embed_update(hipStream_t s, Embedding& E, int n_nodes, const double* x0, const double* q, bool copy_out) {
  const int n = E.n_points;
  const int nblk = ceil_div(n, kB);
  FB_TRY(E.cur.alloc((size_t)3 * n)); FB_TRY(E.out.alloc((size_t)6 * n + 6)); FB_TRY(E.part.alloc((size_t)6 * nblk));
  float* xyz = E.out.p;
  float* nrm = E.out.p + 3 * (size_t)n;
  float* box = E.out.p + 6 * (size_t)n;
  FB_TRY(launch_1d(k_embed_pos, n, s, n, n_nodes, E.vert_int.p, E.w.p, x0, q, E.cur.p, xyz, E.part.p));
  FB_TRY(launch_1d(k_embed_normals, n, s, n, E.n_triangles, E.inc_lo.p, E.inc_hi.p, E.inc.p, E.tris.p, E.cur.p, nrm));
  FB_TRY(launch_grid(k_box_final<float>, dim3(1), s, nblk, E.part.p, box));
  if (copy_out) {
    E.host.resize((size_t)6 * n + 6);
    FB_HIP(hipMemcpyAsync(E.host.data(), E.out.p, sizeof(float) * E.host.size(), hipMemcpyDeviceToHost, s));  // 24 n + 24 bytes
    FB_HIP(hipStreamSynchronize(s));
  }
  return FB_OK;
}

void embed_mesh_changed(EmbedWork& EW, bool in_place) {
  EW.grid.valid = false;
  EW.cgrid.valid = false;
  for (Embedding& E : EW.slot)
    if (E.live) {
      if (in_place) E.lost = true;
      else E.orphan_all = true;
    }
}

int embed_follow(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, const MeshDelta& D, const CutWork* C, bool bake) {
  const int n = E.n_points;
  E.tr_valid = false;  // (internal ids and elements change under the transposed table)
  if (E.orphan_all) { E.lost = false; return FB_OK; }  // (no binding to carry: every point is searched in whatever mesh is there when it is read)
  if (!E.orphan.p) {
    FB_TRY(E.orphan.alloc((size_t)n));
    FB_TRY(E.orphan.zero(s));
  }
  FB_TRY(E.changed.alloc((size_t)n)); FB_TRY(EW.counts.reserve(4));
  const bool pieces = C && C->n_cut > 0 && C->n_added > 0;
  FB_TRY(launch_1d(k_follow, n, s, n, D.n_tets_old, D.estate.p, D.pos.p, D.n_kept, pieces ? C->n_cut : 0, pieces ? C->cut_tets.p : nullptr, pieces ? C->piece_off.p : nullptr,
                   pieces ? C->pcount.p : nullptr, M.n_tets, M.n_nodes, M.tets, M.x0, M.caller_of, M.internal_of, bake ? 1 : 0, E.elem.p, E.w.p, E.vert.p, E.vert_int.p,
                   E.loc.p, E.zeroed.p, E.orphan.p, E.changed.p));
  FB_TRY(launch_grid(k_flag_sums, dim3(1), s, n, E.changed.p, E.orphan.p, nullptr, EW.counts.p + 1));
  int c[2] = {0, 0};
  FB_TRY(EW.counts.download(c, 2, s, 1));
  if (c[0] < 0 || c[0] > n || c[1] < 0 || c[1] > n) return fail(FB_EDEVICE, "embedding: %d re-bound points, %d orphans out of range", c[0], c[1]);
  E.n_rebound += c[0];
  E.n_orphans = c[1];
  E.lost = false;
  return FB_OK;
}

}  // namespace fb

// ---- the C ABI ----

namespace {

EmbedMesh mesh_of(const fb_fem_s* h) {
  EmbedMesh M;
  M.n_nodes = h->plan.n_global; M.n_tets = h->plan.n_tets;
  M.tets = h->tets.p; M.x0 = h->x0.p;
  M.caller_of = h->ren.active ? h->ren.d_old_of_new.p : nullptr;
  M.internal_of = h->ren.active ? h->ren.d_new_of_old.p : nullptr;
  return M;
}

}  // namespace

// the embedding of a slot, searched again where the mesh under it was replaced
int fb::embedding_current(fb_fem_s* h, int id, Embedding** out) {
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_embed is for unsharded handles");
  if (id < 0 || id >= kEmbedSlots || !h->embed.slot[id].live) return fail(FB_EINVAL, "no embedding %d", id);
  Embedding& E = h->embed.slot[id];
  if (E.lost) return fail(FB_EINVAL, "embedding %d was not carried across a change of the mesh (the change failed): release it and embed again", id);
  if (E.orphan_all || E.n_orphans) {
    SlackScope slack(handle_slack_now(h));
    const EmbedMesh M = mesh_of(h);
    if (!h->embed.grid.valid) FB_TRY(embed_grid_build(h->stream, h->embed.grid, M, h->plan_ws));
    FB_TRY(embed_locate(h->stream, h->embed, E, M, true, h->plan_ws));
    if (E.orphan.p) FB_TRY(E.orphan.zero(h->stream));
  }
  *out = &E;
  return FB_OK;
}

namespace {

int free_slot(fb_fem_s* h, int* slot) {
  for (int k = 0; k < kEmbedSlots; k++)
    if (!h->embed.slot[k].live) { *slot = k; return FB_OK; }
  return fail(FB_EINVAL, "the handle has %d live embeddings already", kEmbedSlots);
}
int embed_finish(fb_fem_s* h, int slot, int rc, const fb_fem_embed_params* p, int* id, fb_fem_embed_info* out);

void embed_fill(const fb_fem_s* h, int id, const Embedding& E, const float* box, fb_fem_embed_info* out) {
  if (!out) return;
  const EmbedGrid& G = h->embed.grid;
  out->id = id; out->n_points = E.n_points; out->n_triangles = E.n_triangles;
  out->n_external = E.n_external; out->n_zeroed = E.n_zeroed; out->n_locates = E.n_locates; out->n_rebound = E.n_rebound;
  for (int k = 0; k < 3; k++) { out->grid[k] = G.dim[k]; out->aabb_lo[k] = box[k]; out->aabb_hi[k] = box[3 + k]; }
  out->n_wide = G.n_wide;
}

}  // namespace

int fb_fem_embed(fb_fem_t h, int n_points, const double* xyz, int n_triangles, const int* triangles, const fb_fem_embed_params* p, int* id, fb_fem_embed_info* out) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_embed is for unsharded handles");
  if (n_points <= 0 || !xyz) return fail(FB_EINVAL, "an embedding needs at least one point");
  if (n_triangles < 0 || (n_triangles > 0 && !triangles)) return fail(FB_EINVAL, "bad triangle list");
  if ((long long)n_triangles * 3 > INT_MAX) return fail(FB_EINVAL, "%d triangles are too many", n_triangles);
  if (h->plan.n_tets <= 0) return fail(FB_EINVAL, "the handle's mesh has no elements");
  for (size_t i = 0; i < (size_t)3 * n_points; i++)
    if (!std::isfinite(xyz[i])) return fail(FB_EINVAL, "coordinate %zu of point %zu is not finite", i % 3, i / 3);
  for (size_t i = 0; i < (size_t)3 * n_triangles; i++)
    if (triangles[i] < 0 || triangles[i] >= n_points) return fail(FB_EINVAL, "triangle %zu: index %d outside [0, %d)", i / 3, triangles[i], n_points);
  int slot = -1;
  FB_TRY(free_slot(h, &slot));
  SlackScope slack(handle_slack_now(h));
  Embedding& E = h->embed.slot[slot];
  E.n_points = n_points; E.n_triangles = n_triangles;
  int rc = E.loc.upload(xyz, (size_t)3 * n_points, h->stream);
  if (rc == FB_OK && n_triangles) rc = E.tris.upload(triangles, (size_t)3 * n_triangles, h->stream);
  return embed_finish(h, slot, rc, p, id, out);
}

int fb_fem_embed_from_poly(fb_fem_t h, fb_poly_t poly, const fb_fem_embed_params* p, int* id, fb_fem_embed_info* out) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_embed is for unsharded handles");
  if (h->plan.n_tets <= 0) return fail(FB_EINVAL, "the handle's mesh has no elements");
  DeviceSurface ds;
  FB_TRY(poly_device_surface(poly, &ds));
  FB_HIP(hipSetDevice(h->prm.device));  // (the polygonizer's calls select its own)
  if (ds.device != h->prm.device) return fail(FB_EINVAL, "the polygonizer lives on device %d, the handle on device %d", ds.device, h->prm.device);
  if (ds.n_vertices <= 0) return fail(FB_EINVAL, "an embedding needs at least one point: the surface is empty");
  int slot = -1;
  FB_TRY(free_slot(h, &slot));
  SlackScope slack(handle_slack_now(h));
  Embedding& E = h->embed.slot[slot];
  hipStream_t s = h->stream;
  E.n_points = ds.n_vertices; E.n_triangles = ds.n_triangles;
  // (the polygonizer's stream has been waited for: its arrays are complete)
  int rc = E.loc.alloc((size_t)3 * ds.n_vertices);
  if (rc == FB_OK) rc = widen_positions(s, 3LL * ds.n_vertices, ds.xyz, E.loc.p);
  if (rc == FB_OK && ds.n_triangles) rc = E.tris.alloc((size_t)3 * ds.n_triangles);
  if (rc == FB_OK && ds.n_triangles && hipMemcpyAsync(E.tris.p, ds.indices, sizeof(int) * 3 * (size_t)ds.n_triangles, hipMemcpyDeviceToDevice, s) != hipSuccess)
    rc = fail(FB_EDEVICE, "copy of the surface's triangles failed");
  return embed_finish(h, slot, rc, p, id, out);
}

namespace {
// the rest of a creation, from E.loc and E.tris on the device (rc: what filling them returned)
int embed_finish(fb_fem_s* h, int slot, int rc, const fb_fem_embed_params* p, int* id, fb_fem_embed_info* out) {
  Embedding& E = h->embed.slot[slot];
  hipStream_t s = h->stream;
  const int n_points = E.n_points;
  E.zero_threshold = p ? p->zero_threshold : 0.0;
  const EmbedMesh M = mesh_of(h);
  if (rc == FB_OK && !h->embed.grid.valid) rc = embed_grid_build(s, h->embed.grid, M, h->plan_ws);
  if (rc == FB_OK) rc = embed_locate(s, h->embed, E, M, false, h->plan_ws);
  if (rc == FB_OK) rc = embed_incidence(s, E, h->plan_ws);
  if (rc == FB_OK) rc = embed_update(s, E, M.n_nodes, M.x0, nullptr, false);  // the rest box
  if (rc == FB_OK) rc = E.out.download(E.rest_box, 6, s, (size_t)6 * n_points);
  if (rc != FB_OK) { E.release_all(); return rc; }
  E.live = true;
  h->embed.n_live++;
  if (id) *id = slot;
  embed_fill(h, slot, E, E.rest_box, out);
  return FB_OK;
}
}  // namespace

int fb_fem_read_embedding(fb_fem_t h, int id, int* elements, int* vertices4, double* weights4, double* rest_xyz) {
  CHECK_HANDLE(h);
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  const size_t n = (size_t)E->n_points;
  if (elements) FB_TRY(E->elem.download(elements, n, h->stream));
  if (vertices4) FB_TRY(E->vert.download(vertices4, 4 * n, h->stream));
  if (weights4) FB_TRY(E->w.download(weights4, 4 * n, h->stream));
  if (rest_xyz) FB_TRY(E->loc.download(rest_xyz, 3 * n, h->stream));
  return FB_OK;
}

int fb_fem_embed_update(fb_fem_t h, int id, float* xyz, float* normals, fb_fem_embed_info* out) {
  CHECK_HANDLE(h);
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  const size_t n = (size_t)E->n_points;
  FB_TRY(embed_update(h->stream, *E, h->plan.n_global, h->x0.p, h->q.p, true));
  if (xyz) memcpy(xyz, E->host.data(), sizeof(float) * 3 * n);
  if (normals) memcpy(normals, E->host.data() + 3 * n, sizeof(float) * 3 * n);
  embed_fill(h, id, *E, E->host.data() + 6 * n, out);
  return FB_OK;
}

int fb_fem_embed_release(fb_fem_t h, int id) {
  CHECK_HANDLE(h);
  if (id < 0 || id >= kEmbedSlots || !h->embed.slot[id].live) return fail(FB_EINVAL, "no embedding %d", id);
  FB_HIP(hipStreamSynchronize(h->stream));
  h->embed.slot[id].release_all();
  h->embed.n_live--;
  return FB_OK;
}

namespace {
// A full search as a new mesh would cost it -- grid, every point, the external pass -- on a SCRATCH copy of the embedding's locations: the
// live binding, its counts and its flags are not touched (the grid is built again over the same mesh and stays valid).  seconds3: grid
// build | search (k_locate, the compaction, its host wait) | external pass with the weights and the counts; each the median of reps.
int time_search(fb_fem_s* h, const Embedding& E, int reps, double* seconds3) {
  hipStream_t s = h->stream;
  const EmbedMesh M = mesh_of(h);
  Embedding T;
  T.n_points = E.n_points;
  T.zero_threshold = E.zero_threshold;
  T.orphan_all = true;
  FB_TRY(T.loc.alloc((size_t)3 * E.n_points));
  FB_HIP(hipMemcpyAsync(T.loc.p, E.loc.p, sizeof(double) * 3 * (size_t)E.n_points, hipMemcpyDeviceToDevice, s));
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (hipEvent_t& e : ev) FB_HIP(hipEventCreate(&e));
  std::vector<double> t[3];
  int rc = FB_OK;
  // (as a new mesh: no centre grid yet, so the rule decides on the count alone and a ring search pays for its grid in the third phase;
  // a grid that was there is this generation's and stands as it was -- a build in here writes the same arrays again)
  EmbedCentreGrid& CG = h->embed.cgrid;
  const bool had = CG.valid;
  const int builds = CG.n_builds;
  for (int r = 0; r < reps && rc == FB_OK; r++) {
    int n_ext = 0;
    T.orphan_all = true;
    CG.valid = false;
    rc = hipEventRecord(ev[0], s) == hipSuccess ? FB_OK : fail(FB_EDEVICE, "event record failed");
    if (rc == FB_OK) rc = embed_grid_build(s, h->embed.grid, M, h->plan_ws);
    if (rc == FB_OK) (void)hipEventRecord(ev[1], s);
    if (rc == FB_OK) rc = embed_locate_search(s, h->embed, T, M, false, h->plan_ws, &n_ext);
    if (rc == FB_OK) (void)hipEventRecord(ev[2], s);
    if (rc == FB_OK) rc = embed_locate_finish(s, h->embed, T, M, false, h->plan_ws, n_ext);
    if (rc == FB_OK) (void)hipEventRecord(ev[3], s);
    if (rc == FB_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(FB_EDEVICE, "stream wait failed");
    for (int k = 0; k < 3 && rc == FB_OK; k++) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) != hipSuccess) rc = fail(FB_EDEVICE, "event time failed");
      t[k].push_back(ms * 1e-3);
    }
  }
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  CG.valid = rc == FB_OK && had;
  CG.n_builds = builds;
  FB_TRY(rc);
  for (int k = 0; k < 3; k++) {
    std::sort(t[k].begin(), t[k].end());
    seconds3[k] = t[k][t[k].size() / 2];
  }
  return FB_OK;
}
}  // namespace

int fb_fem_time_embed(fb_fem_t h, int id, int reps, double* seconds_locate, double* seconds_update) {
  CHECK_HANDLE(h);
  if (reps < 1) return fail(FB_EINVAL, "reps must be positive");
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  SlackScope slack(handle_slack_now(h));
  if (seconds_locate) {
    double s3[3];
    FB_TRY(time_search(h, *E, reps, s3));
    *seconds_locate = s3[0] + s3[1] + s3[2];
  }
  if (seconds_update) FB_TRY(timed_median(h, reps, [&] { return embed_update(h->stream, *E, h->plan.n_global, h->x0.p, h->q.p, true); }, seconds_update));
  return FB_OK;
}

int fb_fem_time_embed_search(fb_fem_t h, int id, int reps, double seconds3[3]) {
  CHECK_HANDLE(h);
  if (reps < 1 || !seconds3) return fail(FB_EINVAL, "reps must be positive and seconds3 not null");
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  SlackScope slack(handle_slack_now(h));
  return time_search(h, *E, reps, seconds3);
}

namespace {
// The external pass alone, for the outside points of E, on a scratch copy: seconds2[0] the centre grid's build (ring; 0 for the scan),
// [1] the pass with the given path.  The handle is left as it was: binding, counts, and whether a centre grid exists.
int time_closest(fb_fem_s* h, const Embedding& E, int reps, int path, double* seconds2) {
  hipStream_t s = h->stream;
  const EmbedMesh M = mesh_of(h);
  if (!h->embed.grid.valid) FB_TRY(embed_grid_build(s, h->embed.grid, M, h->plan_ws));
  if (path == FB_EMBED_CLOSEST_RING && !embed_ring_covers(h->embed.grid)) return fail(FB_EINVAL, "the ring search does not cover a mesh this far from the origin");
  Embedding T;
  T.n_points = E.n_points;
  T.orphan_all = true;
  FB_TRY(T.loc.alloc((size_t)3 * E.n_points));
  FB_HIP(hipMemcpyAsync(T.loc.p, E.loc.p, sizeof(double) * 3 * (size_t)E.n_points, hipMemcpyDeviceToDevice, s));
  int n_ext = 0;
  FB_TRY(embed_locate_search(s, h->embed, T, M, false, h->plan_ws, &n_ext));  // (the list of the outside points stays in the handle's workspace)
  long long budget = 0;
  (void)embed_closest_choice(h->embed, M, n_ext, &budget);
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  for (hipEvent_t& e : ev) FB_HIP(hipEventCreate(&e));
  EmbedCentreGrid& CG = h->embed.cgrid;
  const bool had = CG.valid;
  const int builds = CG.n_builds;
  std::vector<double> t[2];
  int rc = FB_OK;
  for (int r = 0; r < reps && rc == FB_OK; r++) {
    rc = hipEventRecord(ev[0], s) == hipSuccess ? FB_OK : fail(FB_EDEVICE, "event record failed");
    if (rc == FB_OK && path == FB_EMBED_CLOSEST_RING) rc = embed_centre_grid_build(s, h->embed, M, h->plan_ws);
    if (rc == FB_OK) (void)hipEventRecord(ev[1], s);
    if (rc == FB_OK) rc = embed_closest(s, h->embed, T, M, h->plan_ws, n_ext, path, budget);
    if (rc == FB_OK) (void)hipEventRecord(ev[2], s);
    if (rc == FB_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(FB_EDEVICE, "stream wait failed");
    for (int k = 0; k < 2 && rc == FB_OK; k++) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) != hipSuccess) rc = fail(FB_EDEVICE, "event time failed");
      t[k].push_back(ms * 1e-3);
    }
  }
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  CG.valid = rc == FB_OK && had;  // (a grid that was there is this generation's: a build in here wrote the same arrays again)
  CG.n_builds = builds;
  FB_TRY(rc);
  for (int k = 0; k < 2; k++) {
    std::sort(t[k].begin(), t[k].end());
    seconds2[k] = t[k][t[k].size() / 2];
  }
  if (path != FB_EMBED_CLOSEST_RING) seconds2[0] = 0.0;
  return FB_OK;
}
}  // namespace

int fb_fem_embed_search_info_get(fb_fem_t h, int id, fb_fem_embed_search_info* out) {
  CHECK_HANDLE(h);
  if (!out) return fail(FB_EINVAL, "out must not be null");
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  out->path = E->search.path; out->n_outside = E->search.n_outside; out->n_far = E->search.n_far;
  out->centre_grid_builds = h->embed.cgrid.n_builds;
  out->max_centres_one_point = E->search.max_one;
  out->centres_tested = E->search.tested;
  return FB_OK;
}

int fb_fem_time_embed_closest(fb_fem_t h, int id, int reps, int path, double seconds2[2]) {
  CHECK_HANDLE(h);
  if (reps < 1 || !seconds2) return fail(FB_EINVAL, "reps must be positive and seconds2 not null");
  if (path != FB_EMBED_CLOSEST_SCAN && path != FB_EMBED_CLOSEST_RING) return fail(FB_EINVAL, "path must be FB_EMBED_CLOSEST_SCAN or FB_EMBED_CLOSEST_RING");
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  SlackScope slack(handle_slack_now(h));
  return time_closest(h, *E, reps, path, seconds2);
}
