// The haptic probe on the device (haptic.h), hand-written for gfx950: ring-spread forces, picking, volume.
//
// Spread: no queue, no frontier list, no atomics and no data-dependent write index.  A byte per (source of the batch, node) holds the
// ring in which the source's breadth-first walk first reaches the node (0xFF: not yet).  Pass j is one launch over (element, source):
// an element with a node of ring j-1 stores j to those of its nodes still at 0xFF.  All concurrent stores to a byte carry the same
// value and a concurrent reader sees 0xFF or j, neither of which is j-1, so one array serves as the pass's input and output.  A last
// launch over the nodes adds mag[ring] * f_s for the sources in ascending order: every node receives its additions in the order of
// Deformable::applyHapticForces, one fp64 multiply and one fp64 add each (the unit is built with -ffp-contract=off).  Every index
// is the thread's own id, checked against the count, or a node id of the handle's element list, checked against n_nodes.
//
// Pick / box / volume: one thread per caller id (gathering through the renumbering map, so ascending caller order needs no sort) or per
// element; minima, counts and sums leave the workgroup as per-workgroup partials folded by a second, single-workgroup launch in a fixed
// order (workgroup.hip.h) -- no floating-point atomics, the same bits from call to call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "fem_handle.h"
#include "haptic.h"
#include "launch.hip.h"
#include "mesh_device.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

// ---- spread ----

// A thread per source, over ALL sources: the first occurrence of an id adds its force and those of the later occurrences, in order.
__global__ __launch_bounds__(kB) void k_hap_direct(int n, const int* __restrict__ ids, const double* __restrict__ f3, const int* __restrict__ new_of_old, int n_nodes,
                                                   double* __restrict__ fext) {
  const int s = blockIdx.x * kB + threadIdx.x;
  if (s >= n) return;
  const int id = ids[s];
  if ((unsigned)id >= (unsigned)n_nodes) return;  // (validated on the host already)
  for (int t = 0; t < s; t++)
    if (ids[t] == id) return;
  const int node = new_of_old ? new_of_old[id] : id;
  if ((unsigned)node >= (unsigned)n_nodes) return;
  double a[3] = {fext[3 * (size_t)node], fext[3 * (size_t)node + 1], fext[3 * (size_t)node + 2]};
  for (int t = s; t < n; t++)
    if (ids[t] == id) { a[0] += f3[3 * t]; a[1] += f3[3 * t + 1]; a[2] += f3[3 * t + 2]; }
  fext[3 * (size_t)node] = a[0]; fext[3 * (size_t)node + 1] = a[1]; fext[3 * (size_t)node + 2] = a[2];
}

// A thread per source of the batch: ring 0
__global__ __launch_bounds__(kB) void k_hap_seed(int nb, const int* __restrict__ ids, const int* __restrict__ new_of_old, int n_nodes, unsigned char* __restrict__ level) {
  const int s = blockIdx.x * kB + threadIdx.x;
  if (s >= nb) return;
  const int id = ids[s];
  if ((unsigned)id >= (unsigned)n_nodes) return;
  const int node = new_of_old ? new_of_old[id] : id;
  if ((unsigned)node >= (unsigned)n_nodes) return;
  level[(size_t)s * n_nodes + node] = 0;
}

// Pass j: a thread per (element, source of the batch = blockIdx.y)
__global__ __launch_bounds__(kB) void k_hap_ring(int n_tets, const int4* __restrict__ tets, int n_nodes, int j, unsigned char* level) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  const int4 t = tets[e];
  if ((unsigned)t.x >= (unsigned)n_nodes || (unsigned)t.y >= (unsigned)n_nodes || (unsigned)t.z >= (unsigned)n_nodes || (unsigned)t.w >= (unsigned)n_nodes) return;
  unsigned char* L = level + (size_t)blockIdx.y * n_nodes;
  const unsigned char before = (unsigned char)(j - 1), now = (unsigned char)j;
  const unsigned char a = L[t.x], b = L[t.y], c = L[t.z], d = L[t.w];
  if (a != before && b != before && c != before && d != before) return;
  if (a == 0xFF) L[t.x] = now;
  if (b == 0xFF) L[t.y] = now;
  if (c == 0xFF) L[t.z] = now;
  if (d == 0xFF) L[t.w] = now;
}

// A thread per node (internal id): the ring additions of the batch's sources, ascending
__global__ __launch_bounds__(kB) void k_hap_apply(int n_nodes, int nb, int size, const unsigned char* __restrict__ level, const double* __restrict__ f3,
                                                  const double* __restrict__ mag, double* __restrict__ fext) {
  const int node = blockIdx.x * kB + threadIdx.x;
  if (node >= n_nodes) return;
  double a[3];
  bool any = false;
  for (int s = 0; s < nb; s++) {
    const int l = level[(size_t)s * n_nodes + node];
    if (l < 1 || l > size - 1) continue;
    if (!any) { a[0] = fext[3 * (size_t)node]; a[1] = fext[3 * (size_t)node + 1]; a[2] = fext[3 * (size_t)node + 2]; any = true; }
    const double m = mag[l];
    a[0] += m * f3[3 * s]; a[1] += m * f3[3 * s + 1]; a[2] += m * f3[3 * s + 2];
  }
  if (any) { fext[3 * (size_t)node] = a[0]; fext[3 * (size_t)node + 1] = a[1]; fext[3 * (size_t)node + 2] = a[2]; }
}

// ---- pick ----

// (the (d, caller id) minimum over the workgroup: wg_best<int, Lowest>; node_position: mesh_device.hip.h)

// A thread per caller id: d = dx dx + dy dy + dz dz on x0 + q (VolMesh::findClosestVertex)
__global__ __launch_bounds__(kB) void k_pick_part(int n_nodes, const double* __restrict__ x0, const double* __restrict__ q, const int* __restrict__ new_of_old, double wx,
                                                  double wy, double wz, double* __restrict__ part_d, int* __restrict__ part_i) {
  const int i = blockIdx.x * kB + threadIdx.x;
  double d = INFINITY;
  int bi = INT_MAX;
  if (i < n_nodes) {
    double p[3];
    bool ok;
    node_position(i, new_of_old, n_nodes, x0, q, p, &ok);
    if (ok) {
      const double dx = p[0] - wx, dy = p[1] - wy, dz = p[2] - wz;
      d = dx * dx + dy * dy + dz * dz;
      bi = i;
    }
  }
  wg_best<int, Lowest>(d, bi);
  if (threadIdx.x == 0) { part_d[blockIdx.x] = d; part_i[blockIdx.x] = bi; }
}

// one workgroup: the minimum of the partials, the picked node's position
__global__ __launch_bounds__(kB) void k_pick_final(int n_part, const double* __restrict__ part_d, const int* __restrict__ part_i, int n_nodes, const double* __restrict__ x0,
                                                   const double* __restrict__ q, const int* __restrict__ new_of_old, PickResult* __restrict__ out) {
  double d = INFINITY;
  int bi = INT_MAX;
  fold_best<int, Lowest>(n_part, part_d, part_i, d, bi);
  wg_best<int, Lowest>(d, bi);
  if (threadIdx.x == 0) {
    PickResult r;
    r.dist2 = d; r.index = -1; r.pad = 0;
    r.xyz[0] = r.xyz[1] = r.xyz[2] = 0.0;
    if ((unsigned)bi < (unsigned)n_nodes) {
      bool ok;
      node_position(bi, new_of_old, n_nodes, x0, q, r.xyz, &ok);
      if (ok) r.index = bi;
    }
    *out = r;
  }
}

// ---- box ----

struct Box { double lo[3], hi[3]; };

// A thread per caller id.  WRITE = false: the hits of the workgroup.  WRITE = true: the hit's place is the hits of the workgroups before
// it plus its rank in the workgroup, and it is written only when that place lies below the capacity the buffers were sized from.
template <bool WRITE>
__global__ __launch_bounds__(kB) void k_box(int n_nodes, const double* __restrict__ x0, const double* __restrict__ q, const int* __restrict__ new_of_old, Box box,
                                            int* __restrict__ cnt, const int* __restrict__ off, int capacity, int* __restrict__ ids, double* __restrict__ xyz) {
  const int i = blockIdx.x * kB + threadIdx.x;
  double p[3] = {0.0, 0.0, 0.0};
  bool hit = false;
  if (i < n_nodes) {
    bool ok;
    node_position(i, new_of_old, n_nodes, x0, q, p, &ok);
    hit = ok && in_box(p, box.lo, box.hi);
  }
  int total;
  const int rank = wg_rank(hit, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    return;
  }
  if (!hit) return;
  const int pos = off[blockIdx.x] + rank;
  if (pos < 0 || pos >= capacity) return;
  ids[pos] = i;
  xyz[3 * (size_t)pos] = p[0]; xyz[3 * (size_t)pos + 1] = p[1]; xyz[3 * (size_t)pos + 2] = p[2];
}

// one workgroup: exclusive scan of the workgroups' counts, the total after the last
__global__ __launch_bounds__(kB) void k_box_scan(int n, const int* __restrict__ cnt, int* __restrict__ off) { wg_scan_partials<1>(n, cnt, off); }

// ---- volume ----

// A thread per element: tet_volume on x0 + q (Deformable::computeVolume)
__global__ __launch_bounds__(kB) void k_volume(int n_tets, const int4* __restrict__ tets, int n_nodes, const double* __restrict__ x0, const double* __restrict__ q,
                                               double* __restrict__ vol, double* __restrict__ part) {
  const int e = blockIdx.x * kB + threadIdx.x;
  double cur = 0.0;
  if (e < n_tets) {
    const int4 t = tets[e];
    const int id[4] = {t.x, t.y, t.z, t.w};
    double p[4][3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      ok = ok && (unsigned)id[k] < (unsigned)n_nodes;
      const size_t b = ok ? 3 * (size_t)id[k] : 0;
#pragma unroll
      for (int c = 0; c < 3; c++) p[k][c] = x0[b + c] + q[b + c];
    }
    cur = ok ? tet_volume(p) : 0.0;
    vol[e] = cur;
  }
  const double s = wg_sum(cur);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one workgroup: thread t adds the partials t, t + 256, ... in that order, then the same tree
__global__ __launch_bounds__(kB) void k_volume_final(int n_part, const double* __restrict__ part, double* __restrict__ total) {
  const double s = wg_sum(fold_sum(n_part, part));
  if (threadIdx.x == 0) *total = s;
}

}  // namespace

int haptic_spread(hipStream_t s, HapticWork& H, int n_nodes, int n_tets, const int4* tets, const int* new_of_old, int n, const int* ids, const double* forces3, int size,
                  double* fext) {
  if (n <= 0) return FB_OK;
  // one upload: forces3[3 n] | mag[size] | ids[n]
  const size_t n_dbl = (size_t)3 * n + (size_t)size;
  const size_t n_bytes = sizeof(double) * n_dbl + sizeof(int) * (size_t)n;
  if (n_bytes > kHapticArgBytes) return fail(FB_EINVAL, "haptic arguments of %zu bytes", n_bytes);
  if (!H.args_pinned) FB_HIP(hipHostMalloc((void**)&H.args_pinned, kHapticArgBytes, hipHostMallocDefault));
  if (!H.args_ev) FB_HIP(hipEventCreateWithFlags(&H.args_ev, hipEventDisableTiming));
  else FB_HIP(hipEventSynchronize(H.args_ev));  // the previous call's copy has read the staging (it completed long ago unless calls come back to back)
  double* hd = reinterpret_cast<double*>(H.args_pinned);
  memcpy(hd, forces3, sizeof(double) * 3 * (size_t)n);
  hd[3 * (size_t)n] = 1.0;  // (ring 0 is the source itself: the direct add)
  for (int j = 1; j < size; j++) hd[3 * (size_t)n + j] = 1.0 * (size - j) / static_cast<double>(size);
  memcpy(H.args_pinned + sizeof(double) * n_dbl, ids, sizeof(int) * (size_t)n);
  FB_TRY(H.args.reserve(kHapticArgBytes));
  FB_HIP(hipMemcpyAsync(H.args.p, H.args_pinned, n_bytes, hipMemcpyHostToDevice, s));
  FB_HIP(hipEventRecord(H.args_ev, s));
  const double* d_f3 = reinterpret_cast<const double*>(H.args.p);
  const double* d_mag = d_f3 + 3 * (size_t)n;
  const int* d_ids = reinterpret_cast<const int*>(H.args.p + sizeof(double) * n_dbl);
  FB_TRY(launch_1d(k_hap_direct, n, s, n, d_ids, d_f3, new_of_old, n_nodes, fext));
  return haptic_spread_rings(s, H, n_nodes, n_tets, tets, new_of_old, n, d_ids, d_f3, d_mag, size, fext);
}

int haptic_spread_rings(hipStream_t s, HapticWork& H, int n_nodes, int n_tets, const int4* tets, const int* new_of_old, int n, const int* d_ids, const double* d_f3,
                        const double* d_mag, int size, double* fext) {
  if (n <= 0 || size <= 1 || n_tets <= 0) return FB_OK;
  FB_TRY(H.level.reserve((size_t)std::min(n, kHapticBatch) * n_nodes));
  for (int base = 0; base < n; base += kHapticBatch) {  // ascending: the order of every node's additions
    const int nb = std::min(kHapticBatch, n - base);
    FB_HIP(hipMemsetAsync(H.level.p, 0xFF, (size_t)nb * n_nodes, s));
    FB_TRY(launch_1d(k_hap_seed, nb, s, nb, d_ids + base, new_of_old, n_nodes, H.level.p));
    for (int j = 1; j < size; j++) FB_TRY(launch_grid(k_hap_ring, dim3(blocks_for(n_tets), nb), s, n_tets, tets, n_nodes, j, H.level.p));
    FB_TRY(launch_1d(k_hap_apply, n_nodes, s, n_nodes, nb, size, H.level.p, d_f3 + 3 * (size_t)base, d_mag, fext));
  }
  return FB_OK;
}

int haptic_pick_vertex(hipStream_t s, HapticWork& H, int n_nodes, const double* x0, const double* q, const int* new_of_old, const double wpos[3], PickResult* out) {
  const int nblk = blocks_for(n_nodes);
  FB_TRY(H.pick_d.reserve((size_t)nblk)); FB_TRY(H.pick_i.reserve((size_t)nblk)); FB_TRY(H.pick_out.reserve(1));
  FB_TRY(launch_1d(k_pick_part, n_nodes, s, n_nodes, x0, q, new_of_old, wpos[0], wpos[1], wpos[2], H.pick_d.p, H.pick_i.p));
  FB_TRY(launch_grid(k_pick_final, dim3(1), s, nblk, H.pick_d.p, H.pick_i.p, n_nodes, x0, q, new_of_old, H.pick_out.p));
  return H.pick_out.download(out, 1, s);
}

int haptic_pick_box(hipStream_t s, HapticWork& H, int n_nodes, const double* x0, const double* q, const int* new_of_old, const double lo[3], const double hi[3], int capacity,
                    int* ids, double* xyz, int* n_found) {
  const int nblk = blocks_for(n_nodes);
  const int cap = std::min(capacity, n_nodes);  // (there are no more hits than nodes)
  FB_TRY(H.box_cnt.reserve((size_t)nblk)); FB_TRY(H.box_off.reserve((size_t)nblk + 1));
  Box box;
  for (int k = 0; k < 3; k++) { box.lo[k] = lo[k]; box.hi[k] = hi[k]; }
  FB_TRY(launch_1d(k_box<false>, n_nodes, s, n_nodes, x0, q, new_of_old, box, H.box_cnt.p, nullptr, 0, nullptr, nullptr));
  FB_TRY(launch_grid(k_box_scan, dim3(1), s, nblk, H.box_cnt.p, H.box_off.p));
  if (cap > 0) {
    FB_TRY(H.box_ids.reserve((size_t)cap)); FB_TRY(H.box_xyz.reserve((size_t)3 * cap));
    FB_TRY(launch_1d(k_box<true>, n_nodes, s, n_nodes, x0, q, new_of_old, box, nullptr, H.box_off.p, cap, H.box_ids.p, H.box_xyz.p));
  }
  int total = 0;
  FB_TRY(H.box_off.download(&total, 1, s, (size_t)nblk));
  if (total < 0 || total > n_nodes) return fail(FB_EDEVICE, "pick box: count %d out of range", total);
  const int n_out = std::min(total, cap);
  if (n_out > 0) {
    if (ids) FB_HIP(hipMemcpyAsync(ids, H.box_ids.p, sizeof(int) * (size_t)n_out, hipMemcpyDeviceToHost, s));
    if (xyz) FB_HIP(hipMemcpyAsync(xyz, H.box_xyz.p, sizeof(double) * 3 * (size_t)n_out, hipMemcpyDeviceToHost, s));
    FB_HIP(hipStreamSynchronize(s));
  }
  if (n_found) *n_found = total;
  return FB_OK;
}

int haptic_volume(hipStream_t s, HapticWork& H, int n_nodes, int n_tets, const int4* tets, const double* x0, const double* q, double* total, double* per_element) {
  const int nblk = blocks_for(n_tets);
  FB_TRY(H.vol.reserve((size_t)std::max(n_tets, 1))); FB_TRY(H.vol_part.reserve((size_t)nblk + 1));
  FB_TRY(launch_1d(k_volume, n_tets, s, n_tets, tets, n_nodes, x0, q, H.vol.p, H.vol_part.p));
  FB_TRY(launch_grid(k_volume_final, dim3(1), s, nblk, H.vol_part.p, H.vol_part.p + nblk));
  if (per_element && n_tets > 0) FB_HIP(hipMemcpyAsync(per_element, H.vol.p, sizeof(double) * (size_t)n_tets, hipMemcpyDeviceToHost, s));
  double t = 0.0;
  FB_TRY(H.vol_part.download(&t, 1, s, (size_t)nblk));
  if (total) *total = t;
  return FB_OK;
}

}  // namespace fb

// ---- the C ABI ----

namespace {
inline const int* new_of_old_dev(const fb_fem_s* h) { return h->ren.active ? h->ren.d_new_of_old.p : nullptr; }
}  // namespace

int fb_fem_add_haptic_forces(fb_fem_t h, int n, const int* node_ids, const double* forces3, int neighbourhood_size) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_add_haptic_forces is for unsharded handles");
  if (n < 0 || n > FB_HAPTIC_MAX_SOURCES) return fail(FB_EINVAL, "%d haptic sources: at most FB_HAPTIC_MAX_SOURCES = %d", n, FB_HAPTIC_MAX_SOURCES);
  if (neighbourhood_size < 1 || neighbourhood_size > 255) return fail(FB_EINVAL, "neighbourhood size %d outside [1, 255]", neighbourhood_size);
  if (n == 0) return FB_OK;
  if (!node_ids || !forces3) return fail(FB_EINVAL, "null haptic ids or forces");
  const int n_nodes = h->plan.n_global;
  for (int s = 0; s < n; s++)
    if (node_ids[s] < 0 || node_ids[s] >= n_nodes) return fail(FB_EINVAL, "haptic node id %d (source %d) outside [0, %d)", node_ids[s], s, n_nodes);
  return haptic_spread(h->stream, h->hap, n_nodes, h->plan.n_tets, h->tets.p, new_of_old_dev(h), n, node_ids, forces3, neighbourhood_size, h->fext.p);
}

int fb_fem_pick_vertex(fb_fem_t h, const double wpos[3], int* index, double xyz[3], double* dist2) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_pick_vertex is for unsharded handles");
  if (!wpos) return fail(FB_EINVAL, "null position");
  PickResult r;
  r.index = -1; r.dist2 = 0.0; r.xyz[0] = r.xyz[1] = r.xyz[2] = 0.0;
  if (h->plan.n_global > 0) FB_TRY(haptic_pick_vertex(h->stream, h->hap, h->plan.n_global, h->x0.p, h->q.p, new_of_old_dev(h), wpos, &r));
  if (index) *index = r.index;
  if (xyz) { xyz[0] = r.xyz[0]; xyz[1] = r.xyz[1]; xyz[2] = r.xyz[2]; }
  if (dist2) *dist2 = r.dist2;
  return FB_OK;
}

int fb_fem_pick_box(fb_fem_t h, const double lo[3], const double hi[3], int capacity, int* ids, double* xyz, int* n_found) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_pick_box is for unsharded handles");
  if (!lo || !hi || capacity < 0) return fail(FB_EINVAL, "bad box or capacity");
  if (capacity > 0 && !ids && !xyz) capacity = 0;  // (nowhere to put them: the count only)
  if (h->plan.n_global <= 0) { if (n_found) *n_found = 0; return FB_OK; }
  return haptic_pick_box(h->stream, h->hap, h->plan.n_global, h->x0.p, h->q.p, new_of_old_dev(h), lo, hi, capacity, ids, xyz, n_found);
}

int fb_fem_volume(fb_fem_t h, double* total, double* per_element) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_volume is for unsharded handles");
  return haptic_volume(h->stream, h->hap, h->plan.n_global, h->plan.n_tets, h->tets.p, h->x0.p, h->q.p, total, per_element);
}
