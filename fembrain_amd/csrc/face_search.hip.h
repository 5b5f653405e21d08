// What the two contact units (body_contact.hip, self_contact.hip) share of the search for the closest boundary face, each written once:
// the closest point of a triangle, the grid rule, the grid of face centroids and its build, what a search knows of its points, and the
// record a search leaves (bc_finish).  The two searches themselves stay in their units: k_bc_scan / k_bc_ring in body_contact.hip, and
// in self_contact.hip their twins k_sc_scan / k_sc_ring, which skip the faces a point may not take.  (Written once over an exclusion
// functor that folds away for two bodies, the shared search compiled body_contact's kernels to other instructions than they had;
// the twins leave them as they were.)
// The units are built with -ffp-contract=off: one function is one sequence of roundings wherever it is called.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include "body_contact.h"
#include "embed_grid.hip.h"
#include "launch.hip.h"
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

// ---- host ----

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

}  // namespace
}  // namespace fb
