// The way back from an embedded point set to the tets (embed.h), hand-written for gfx950: forces on drawn points to the nodes, ray and
// point picks on the drawn mesh, element stress per drawn point.
//
// Forces: the transpose of the binding.  The 4 n corners (point p, vertex k) are sorted ONCE, stably, by internal node: a node's run holds
// its corners in ascending 4 p + k, which is the order in which the host loop
//   for p ascending, k = 0..3, c = 0..2:  fext[3 v + c] = fext[3 v + c] + w[4 p + k] * f[3 p + c]
// reaches that node.  The scatter gives a wavefront to every node that has a run.  Sixty-four corners at a time, each lane gathers one
// corner's weight and force and forms its three products; the selected lanes' products are then added in lane order -- every lane adds the
// same values in the same order, so no lane waits for another -- onto the node's value of fext, which is read first and written once.
// One fp64 multiply and one fp64 add per addition (-ffp-contract=off): the bits of the host loop, with no floating-point atomics and
// no second path for short lists.  A list of points is a byte mask over the points and a staging array of their forces; corners of
// points outside the list are skipped, not added as zeros (-0.0 + 0.0 is +0.0).
//
// Picks work on the fp64 positions of fb_fem_embed_update (k_embed_cur forms them again at the current state).  A thread per triangle
// (Moeller-Trumbore, two-sided) or per point; the (t, triangle) / (d, point) minimum leaves the workgroup as a partial and a second,
// single-workgroup launch folds the partials: of equal values the lowest id, the same from call to call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_prims.hip.h"
#include "embed.h"
#include "fem_handle.h"
#include "launch.hip.h"
#include "mesh_device.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

// ---- the transposed table ----

// A thread per corner: its internal node as the sort key (a node outside [0, n_nodes) gets the key n_nodes: behind every run, where
// k_run_bounds drops it), itself as the value
__global__ __launch_bounds__(kB) void k_table_keys(int n_corners, int n_nodes, const int* __restrict__ vert_int, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_corners) return;
  const int v = vert_int[j];
  keys[j] = (unsigned)v < (unsigned)n_nodes ? (uint32_t)v : (uint32_t)n_nodes;
  vals[j] = (uint32_t)j;
}

// (a node's run in the sorted corners: k_run_bounds, mesh_device.hip.h)

// A thread per node: has it a run?
__global__ __launch_bounds__(kB) void k_table_flags(int n_nodes, const int* __restrict__ lo, const int* __restrict__ hi, unsigned char* __restrict__ flag) {
  const int v = blockIdx.x * kB + threadIdx.x;
  if (v < n_nodes) flag[v] = hi[v] > lo[v] ? 1 : 0;
}

// one workgroup: the longest run (an integer maximum: any order)
__global__ __launch_bounds__(kB) void k_table_longest(int n_nodes, const int* __restrict__ lo, const int* __restrict__ hi, int* __restrict__ out) {
  int m = 0;
  for (int v = threadIdx.x; v < n_nodes; v += kB) m = max(m, hi[v] - lo[v]);
  m = wg_max(m);
  if (threadIdx.x == 0) *out = m;
}

// ---- the scatter ----

// A thread per entry of the list: the point's force into the staging array, its byte of the mask
__global__ __launch_bounds__(kB) void k_stage_list(int n, int n_points, const int* __restrict__ ids, const double* __restrict__ f3, double* __restrict__ stage,
                                                   unsigned char* __restrict__ mask, unsigned char on) {
  const int s = blockIdx.x * kB + threadIdx.x;
  if (s >= n) return;
  const int p = ids[s];
  if ((unsigned)p >= (unsigned)n_points) return;  // (validated on the host already)
  if (on) { stage[3 * (size_t)p] = f3[3 * (size_t)s]; stage[3 * (size_t)p + 1] = f3[3 * (size_t)s + 1]; stage[3 * (size_t)p + 2] = f3[3 * (size_t)s + 2]; }
  mask[p] = on;
}

// A wavefront per node with a run (header).  mask null: every point takes part.
__global__ __launch_bounds__(kB) void k_scatter(int n_touched, const int* __restrict__ nodes, int n_nodes, const int* __restrict__ lo, const int* __restrict__ hi,
                                                const uint32_t* __restrict__ corner, int n_corners, const double* __restrict__ w4, const double* __restrict__ stage,
                                                const unsigned char* __restrict__ mask, double* __restrict__ fext) {
  const int item = (blockIdx.x * kB + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (item >= n_touched) return;  // (the whole wavefront)
  const int node = nodes[item];
  if ((unsigned)node >= (unsigned)n_nodes) return;
  const int j0 = lo[node], j1 = hi[node];
  if (j0 < 0 || j1 > n_corners || j0 >= j1) return;
  double a[3] = {0.0, 0.0, 0.0};
  bool any = false;
  for (int base = j0; base < j1; base += 64) {  // (the bounds are the wavefront's: every lane runs every pass)
    const int j = base + lane;
    bool sel = false;
    double p[3] = {0.0, 0.0, 0.0};
    if (j < j1) {
      const uint32_t c = corner[j];
      if (c < (uint32_t)n_corners) {
        const uint32_t pt = c >> 2;
        sel = !mask || mask[pt] != 0;
        if (sel) {
          const double w = w4[c];
          p[0] = w * stage[3 * (size_t)pt]; p[1] = w * stage[3 * (size_t)pt + 1]; p[2] = w * stage[3 * (size_t)pt + 2];
        }
      }
    }
    unsigned long long m = __ballot(sel);
    if (m && !any) {
      a[0] = fext[3 * (size_t)node]; a[1] = fext[3 * (size_t)node + 1]; a[2] = fext[3 * (size_t)node + 2];
      any = true;
    }
    while (m) {  // ascending lanes = ascending corners
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      a[0] += __shfl(p[0], src); a[1] += __shfl(p[1], src); a[2] += __shfl(p[2], src);
    }
  }
  if (any && lane < 3) fext[3 * (size_t)node + lane] = lane == 0 ? a[0] : lane == 1 ? a[1] : a[2];
}

// ---- positions ----

// A thread per point: embed_point at x0 + q, the fp64 positions k_embed_pos of embed.hip keeps
__global__ __launch_bounds__(kB) void k_embed_cur(int n, int n_nodes, const int* __restrict__ vert_int, const double* __restrict__ w4, const double* __restrict__ x0,
                                                  const double* __restrict__ q, double* __restrict__ cur) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i < n) embed_point(i, n_nodes, vert_int, w4, x0, q, cur + 3 * (size_t)i);
}

// ---- the ray ----

struct Ray { double o[3], d[3], t_max; };

// Moeller-Trumbore on triangle tr, two-sided; false: no hit in [0, t_max]
__device__ __forceinline__ bool ray_triangle(const Ray& r, int tr, int n, const int* __restrict__ tris, const double* __restrict__ cur, double* t, double* u, double* v) {
  const int* f = tris + 3 * (size_t)tr;
  if ((unsigned)f[0] >= (unsigned)n || (unsigned)f[1] >= (unsigned)n || (unsigned)f[2] >= (unsigned)n) return false;  // (a list handed over on the device)
  const double* a = cur + 3 * (size_t)f[0];
  const double* b = cur + 3 * (size_t)f[1];
  const double* c = cur + 3 * (size_t)f[2];
  const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double pv[3] = {r.d[1] * e2[2] - r.d[2] * e2[1], r.d[2] * e2[0] - r.d[0] * e2[2], r.d[0] * e2[1] - r.d[1] * e2[0]};
  const double det = (e1[0] * pv[0] + e1[1] * pv[1]) + e1[2] * pv[2];
  if (!(det != 0.0) || det != det) return false;
  const double inv = 1.0 / det;
  const double tv[3] = {r.o[0] - a[0], r.o[1] - a[1], r.o[2] - a[2]};
  const double uu = ((tv[0] * pv[0] + tv[1] * pv[1]) + tv[2] * pv[2]) * inv;
  const double qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
  const double vv = ((r.d[0] * qv[0] + r.d[1] * qv[1]) + r.d[2] * qv[2]) * inv;
  const double tt = ((e2[0] * qv[0] + e2[1] * qv[1]) + e2[2] * qv[2]) * inv;
  if (!(uu >= 0.0 && vv >= 0.0 && uu + vv <= 1.0 && tt >= 0.0 && tt <= r.t_max)) return false;
  *t = tt; *u = uu; *v = vv;
  return true;
}

// A thread per triangle
__global__ __launch_bounds__(kB) void k_ray_part(int n_triangles, int n, const int* __restrict__ tris, const double* __restrict__ cur, Ray r, double* __restrict__ part_d,
                                                 int* __restrict__ part_i) {
  const int tr = blockIdx.x * kB + threadIdx.x;
  double d = INFINITY;
  int bi = INT_MAX;
  if (tr < n_triangles) {
    double t, u, v;
    if (ray_triangle(r, tr, n, tris, cur, &t, &u, &v)) { d = t; bi = tr; }
  }
  wg_best<int, Lowest>(d, bi);
  if (threadIdx.x == 0) { part_d[blockIdx.x] = d; part_i[blockIdx.x] = bi; }
}

// one workgroup: the minimum of the partials; the winner's triangle once more for its barycentrics
__global__ __launch_bounds__(kB) void k_ray_final(int n_part, const double* __restrict__ part_d, const int* __restrict__ part_i, int n_triangles, int n,
                                                  const int* __restrict__ tris, const double* __restrict__ cur, Ray r, EmbedPick* __restrict__ out) {
  double d = INFINITY;
  int bi = INT_MAX;
  fold_best<int, Lowest>(n_part, part_d, part_i, d, bi);
  wg_best<int, Lowest>(d, bi);
  if (threadIdx.x == 0) {
    EmbedPick p;
    p.t = p.u = p.v = 0.0; p.xyz[0] = p.xyz[1] = p.xyz[2] = 0.0; p.index = -1; p.pad = 0;
    double t, u, v;
    if ((unsigned)bi < (unsigned)n_triangles && ray_triangle(r, bi, n, tris, cur, &t, &u, &v)) {
      p.t = t; p.u = u; p.v = v; p.index = bi;
      for (int k = 0; k < 3; k++) p.xyz[k] = r.o[k] + t * r.d[k];
    }
    *out = p;
  }
}

// ---- the closest point ----

// A thread per point: d = dx dx + dy dy + dz dz (fb_fem_pick_vertex's rule)
__global__ __launch_bounds__(kB) void k_point_part(int n, const double* __restrict__ cur, double wx, double wy, double wz, double* __restrict__ part_d, int* __restrict__ part_i) {
  const int i = blockIdx.x * kB + threadIdx.x;
  double d = INFINITY;
  int bi = INT_MAX;
  if (i < n) {
    const double dx = cur[3 * (size_t)i] - wx, dy = cur[3 * (size_t)i + 1] - wy, dz = cur[3 * (size_t)i + 2] - wz;
    d = dx * dx + dy * dy + dz * dz;
    bi = i;
  }
  wg_best<int, Lowest>(d, bi);
  if (threadIdx.x == 0) { part_d[blockIdx.x] = d; part_i[blockIdx.x] = bi; }
}

__global__ __launch_bounds__(kB) void k_point_final(int n_part, const double* __restrict__ part_d, const int* __restrict__ part_i, int n, const double* __restrict__ cur,
                                                    EmbedPick* __restrict__ out) {
  double d = INFINITY;
  int bi = INT_MAX;
  fold_best<int, Lowest>(n_part, part_d, part_i, d, bi);
  wg_best<int, Lowest>(d, bi);
  if (threadIdx.x == 0) {
    EmbedPick p;
    p.t = d; p.u = p.v = 0.0; p.xyz[0] = p.xyz[1] = p.xyz[2] = 0.0; p.index = -1; p.pad = 0;
    if ((unsigned)bi < (unsigned)n) {
      p.index = bi;
      for (int k = 0; k < 3; k++) p.xyz[k] = cur[3 * (size_t)bi + k];
    }
    *out = p;
  }
}

// ---- stress ----

// A thread per point: the von Mises stress of its element
__global__ __launch_bounds__(kB) void k_point_stress(int n, const int* __restrict__ elem, int n_elements, const double* __restrict__ vm, float* __restrict__ out) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  const int e = elem[i];
  out[i] = (unsigned)e < (unsigned)n_elements ? (float)vm[e] : 0.0f;
}

}  // namespace

int embed_table_build(hipStream_t s, EmbedWork& EW, Embedding& E, int n_nodes, PlanWorkspace& W) {
  const int n = E.n_points;
  if ((long long)n * 4 > INT_MAX) return fail(FB_EINVAL, "%d embedded points are too many for the transposed table", n);
  const int nc = 4 * n;
  E.tr_valid = false;
  FB_TRY(E.tr_corner.alloc((size_t)nc)); FB_TRY(E.tr_lo.alloc((size_t)n_nodes)); FB_TRY(E.tr_hi.alloc((size_t)n_nodes));
  FB_TRY(E.tr_flag.alloc((size_t)n_nodes)); FB_TRY(E.tr_nodes.alloc((size_t)n_nodes)); FB_TRY(EW.tr_stats.reserve(2));
  FB_TRY(E.tr_lo.zero(s)); FB_TRY(E.tr_hi.zero(s));
  FB_TRY(W.keys.reserve(((size_t)nc + 1) / 2)); FB_TRY(W.keys_s.reserve(((size_t)nc + 1) / 2)); FB_TRY(W.vals.reserve((size_t)nc));
  uint32_t* ck = reinterpret_cast<uint32_t*>(W.keys.p);
  uint32_t* ck_s = reinterpret_cast<uint32_t*>(W.keys_s.p);
  FB_TRY(launch_1d(k_table_keys, nc, s, nc, n_nodes, E.vert_int.p, ck, W.vals.p));
  // the corners sorted stably by node keep their ascending order inside a node
  FB_TRY(sort_pairs(W.temp, s, ck, ck_s, W.vals.p, E.tr_corner.p, (size_t)nc, (unsigned)bits_of((long long)n_nodes + 1)));
  FB_TRY(launch_1d(k_run_bounds<>, nc, s, nc, ck_s, (uint32_t)n_nodes, E.tr_lo.p, E.tr_hi.p));
  FB_TRY(launch_1d(k_table_flags, n_nodes, s, n_nodes, E.tr_lo.p, E.tr_hi.p, E.tr_flag.p));
  FB_TRY(select_flagged(W.temp, s, rocprim::counting_iterator<int>(0), E.tr_flag.p, E.tr_nodes.p, EW.tr_stats.p, (size_t)n_nodes));
  FB_TRY(launch_grid(k_table_longest, dim3(1), s, n_nodes, E.tr_lo.p, E.tr_hi.p, EW.tr_stats.p + 1));
  int st[2] = {0, 0};
  FB_TRY(EW.tr_stats.download(st, 2, s));  // the host wait
  if (st[0] < 0 || st[0] > n_nodes || st[0] > nc || st[1] < 0 || st[1] > nc) return fail(FB_EDEVICE, "embedding table: %d nodes, longest run %d out of range", st[0], st[1]);
  E.tr_touched = st[0];
  E.tr_longest = st[1];
  E.tr_builds++;
  E.tr_valid = true;
  return FB_OK;
}

int embed_scatter(hipStream_t s, EmbedWork& EW, Embedding& E, int n_nodes, int n, const int* ids, const double* forces3, double* fext) {
  const int np = E.n_points;
  if (n <= 0) return FB_OK;
  if (!E.tr_valid) return fail(FB_EDEVICE, "embedding: no transposed table");
  FB_TRY(E.f_stage.alloc((size_t)3 * np));
  const int* d_ids = nullptr;
  if (!ids) {
    FB_TRY(E.f_stage.upload(forces3, (size_t)3 * np, s));
  } else {
    if (!E.f_mask.p) {
      FB_TRY(E.f_mask.alloc((size_t)np));
      FB_TRY(E.f_mask.zero(s));
    }
    // one upload: forces3[3 n] | ids[n]
    const size_t f_bytes = sizeof(double) * 3 * (size_t)n, bytes = f_bytes + sizeof(int) * (size_t)n;
    std::vector<unsigned char> host(bytes);
    memcpy(host.data(), forces3, f_bytes);
    memcpy(host.data() + f_bytes, ids, sizeof(int) * (size_t)n);
    FB_TRY(EW.touch_args.reserve(bytes));
    FB_HIP(hipMemcpyAsync(EW.touch_args.p, host.data(), bytes, hipMemcpyHostToDevice, s));
    FB_HIP(hipStreamSynchronize(s));  // (the staging vector leaves scope)
    d_ids = reinterpret_cast<const int*>(EW.touch_args.p + f_bytes);
    FB_TRY(launch_1d(k_stage_list, n, s, n, np, d_ids, reinterpret_cast<const double*>(EW.touch_args.p), E.f_stage.p, E.f_mask.p, 1));
  }
  if (E.tr_touched > 0)
    FB_TRY(launch_waves(k_scatter, E.tr_touched, s, E.tr_touched, E.tr_nodes.p, n_nodes, E.tr_lo.p, E.tr_hi.p, E.tr_corner.p, 4 * np, E.w.p, E.f_stage.p,
                        ids ? E.f_mask.p : nullptr, fext));
  if (ids) FB_TRY(launch_1d(k_stage_list, n, s, n, np, d_ids, nullptr, nullptr, E.f_mask.p, 0));  // the mask is zero again
  return FB_OK;
}

int embed_positions(hipStream_t s, Embedding& E, int n_nodes, const double* x0, const double* q) {
  FB_TRY(E.cur.alloc((size_t)3 * E.n_points));
  return launch_1d(k_embed_cur, E.n_points, s, E.n_points, n_nodes, E.vert_int.p, E.w.p, x0, q, E.cur.p);
}

int embed_pick_ray(hipStream_t s, EmbedWork& EW, Embedding& E, const double origin[3], const double dir[3], double t_max, EmbedPick* out) {
  const int nt = E.n_triangles;
  out->t = out->u = out->v = 0.0; out->xyz[0] = out->xyz[1] = out->xyz[2] = 0.0; out->index = -1; out->pad = 0;
  if (nt <= 0) return FB_OK;
  const int nblk = blocks_for(nt);
  FB_TRY(EW.pick_d.reserve((size_t)nblk)); FB_TRY(EW.pick_i.reserve((size_t)nblk)); FB_TRY(EW.pick_out.reserve(1));
  Ray r;
  for (int k = 0; k < 3; k++) { r.o[k] = origin[k]; r.d[k] = dir[k]; }
  r.t_max = t_max;
  FB_TRY(launch_1d(k_ray_part, nt, s, nt, E.n_points, E.tris.p, E.cur.p, r, EW.pick_d.p, EW.pick_i.p));
  FB_TRY(launch_grid(k_ray_final, dim3(1), s, nblk, EW.pick_d.p, EW.pick_i.p, nt, E.n_points, E.tris.p, E.cur.p, r, EW.pick_out.p));
  return EW.pick_out.download(out, 1, s);
}

int embed_pick_point(hipStream_t s, EmbedWork& EW, Embedding& E, const double wpos[3], EmbedPick* out) {
  const int n = E.n_points;
  const int nblk = blocks_for(n);
  FB_TRY(EW.pick_d.reserve((size_t)nblk)); FB_TRY(EW.pick_i.reserve((size_t)nblk)); FB_TRY(EW.pick_out.reserve(1));
  FB_TRY(launch_1d(k_point_part, n, s, n, E.cur.p, wpos[0], wpos[1], wpos[2], EW.pick_d.p, EW.pick_i.p));
  FB_TRY(launch_grid(k_point_final, dim3(1), s, nblk, EW.pick_d.p, EW.pick_i.p, n, E.cur.p, EW.pick_out.p));
  return EW.pick_out.download(out, 1, s);
}

int embed_stress(hipStream_t s, EmbedWork& EW, const Embedding& E, int n_elements, const double* vm, float* per_point) {
  const int n = E.n_points;
  FB_TRY(EW.vm_out.reserve((size_t)n));
  FB_TRY(launch_1d(k_point_stress, n, s, n, E.elem.p, n_elements, vm, EW.vm_out.p));
  if (per_point) FB_TRY(EW.vm_out.download(per_point, (size_t)n, s));
  return FB_OK;
}

}  // namespace fb

// ---- the C ABI ----

int fb_fem_embed_add_forces(fb_fem_t h, int id, int n, const int* point_ids, const double* forces3) {
  CHECK_HANDLE(h);
  // (the arguments first: a refused call searches nothing either)
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_embed is for unsharded handles");
  if (id < 0 || id >= kEmbedSlots || !h->embed.slot[id].live) return fail(FB_EINVAL, "no embedding %d", id);
  const int np = h->embed.slot[id].n_points;
  if (n < 0 || n > np) return fail(FB_EINVAL, "fb_fem_embed_add_forces: %d forces on an embedding of %d points", n, np);
  if (!point_ids && n != 0 && n != np) return fail(FB_EINVAL, "fb_fem_embed_add_forces: without a list n must be the %d points of the embedding, not %d", np, n);
  if (n == 0) return FB_OK;
  if (!forces3) return fail(FB_EINVAL, "fb_fem_embed_add_forces: null forces");
  for (int s = 0; s < n && point_ids; s++) {
    if (point_ids[s] < 0 || point_ids[s] >= np) return fail(FB_EINVAL, "fb_fem_embed_add_forces: point id %d (entry %d) outside [0, %d)", point_ids[s], s, np);
    if (s && point_ids[s] <= point_ids[s - 1]) return fail(FB_EINVAL, "fb_fem_embed_add_forces: the list is not strictly ascending at entry %d (%d after %d)", s, point_ids[s], point_ids[s - 1]);
  }
  for (size_t i = 0; i < (size_t)3 * n; i++)
    if (!std::isfinite(forces3[i])) return fail(FB_EINVAL, "fb_fem_embed_add_forces: component %zu of force %zu is not finite", i % 3, i / 3);
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  SlackScope slack(handle_slack_now(h));
  if (!E->tr_valid) FB_TRY(embed_table_build(h->stream, h->embed, *E, h->plan.n_global, h->plan_ws));
  return embed_scatter(h->stream, h->embed, *E, h->plan.n_global, n, point_ids, forces3, h->fext.p);
}

int fb_fem_embed_forces_info(fb_fem_t h, int id, int* n_table_builds, int* longest_run, int* n_nodes_touched) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_embed is for unsharded handles");
  if (id < 0 || id >= kEmbedSlots || !h->embed.slot[id].live) return fail(FB_EINVAL, "no embedding %d", id);
  const Embedding& E = h->embed.slot[id];
  if (n_table_builds) *n_table_builds = E.tr_builds;
  if (longest_run) *longest_run = E.tr_longest;
  if (n_nodes_touched) *n_nodes_touched = E.tr_touched;
  return FB_OK;
}

int fb_fem_embed_pick_ray(fb_fem_t h, int id, const double origin[3], const double dir[3], double t_max, int* triangle, double* t, double bary[2], double xyz[3]) {
  CHECK_HANDLE(h);
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  if (!origin || !dir) return fail(FB_EINVAL, "fb_fem_embed_pick_ray: null origin or direction");
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(origin[k]) || !std::isfinite(dir[k])) return fail(FB_EINVAL, "fb_fem_embed_pick_ray: origin or direction not finite");
  if (dir[0] == 0.0 && dir[1] == 0.0 && dir[2] == 0.0) return fail(FB_EINVAL, "fb_fem_embed_pick_ray: zero direction");
  if (t_max != t_max) return fail(FB_EINVAL, "fb_fem_embed_pick_ray: t_max is not a number");
  EmbedPick p;
  p.t = p.u = p.v = 0.0; p.xyz[0] = p.xyz[1] = p.xyz[2] = 0.0; p.index = -1; p.pad = 0;
  if (E->n_triangles > 0) {
    SlackScope slack(handle_slack_now(h));
    FB_TRY(embed_positions(h->stream, *E, h->plan.n_global, h->x0.p, h->q.p));
    FB_TRY(embed_pick_ray(h->stream, h->embed, *E, origin, dir, t_max, &p));
  }
  if (triangle) *triangle = p.index;
  if (t) *t = p.t;
  if (bary) { bary[0] = p.u; bary[1] = p.v; }
  if (xyz) { xyz[0] = p.xyz[0]; xyz[1] = p.xyz[1]; xyz[2] = p.xyz[2]; }
  return FB_OK;
}

int fb_fem_embed_pick_point(fb_fem_t h, int id, const double wpos[3], int* index, double xyz[3], double* dist2) {
  CHECK_HANDLE(h);
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  if (!wpos) return fail(FB_EINVAL, "fb_fem_embed_pick_point: null position");
  EmbedPick p;
  SlackScope slack(handle_slack_now(h));
  FB_TRY(embed_positions(h->stream, *E, h->plan.n_global, h->x0.p, h->q.p));
  FB_TRY(embed_pick_point(h->stream, h->embed, *E, wpos, &p));
  if (index) *index = p.index;
  if (xyz) { xyz[0] = p.xyz[0]; xyz[1] = p.xyz[1]; xyz[2] = p.xyz[2]; }
  if (dist2) *dist2 = p.t;
  return FB_OK;
}

int fb_fem_embed_stress(fb_fem_t h, int id, float* per_point) {
  CHECK_HANDLE(h);
  FB_TRY(stress_current(h, "fb_fem_embed_stress"));
  Embedding* E = nullptr;
  FB_TRY(embedding_current(h, id, &E));
  SlackScope slack(handle_slack_now(h));
  return embed_stress(h->stream, h->embed, *E, h->stress.n_elements, h->stress.vm.p, per_point);
}
