// The probe's box contact on the device (contact.h), hand-written for gfx950: the contact session and a ring spread without a source limit.
//
// Move: the tissue's float box, the box test with first-position capture per caller id, the compaction of the touched flags into the
// ascending list, the lexicographic (d, node, face) minimum and the force pass, all on the primitives of workgroup.hip.h.  Every
// kernel decides "miss" and "empty" for itself from the box and the count left on the device by the kernels before it, so the host waits
// once, for the info struct.  Counts and minima leave a workgroup as partials folded by a single-workgroup launch in a fixed order.
//
// Apply, by records: one wavefront (a workgroup of 64) per source walks its ball over the node adjacency (the plan's block pattern) with a
// visited table in LDS -- open addressing, a bounded probe count, the ring kept beside the id in arrival order -- and emits (target,
// source rank, ring) records behind an integer cursor.  The records are sorted by (target, source rank) and a thread per target segment
// does that node's additions in ascending source order, one fp64 multiply and one fp64 add per component (the unit is built with
// -ffp-contract=off): the same bits as Deformable::applyHapticForces.  No floating-point atomics.  A ball that overflows its table, or
// more records than the budget, sends the WHOLE apply to the level-array passes of haptic.hip (haptic_spread_rings): a mixed path would
// break the order.
//
// Every index is the thread's own id checked against its count, an id read from the handle checked against n_nodes, or a table slot
// masked to the table's size; every loop is bounded by a count known at launch or by a compile-time constant.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_prims.hip.h"
#include "fem_handle.h"
#include "contact.h"
#include "launch.hip.h"
#include "mesh_device.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

struct Tool {
  double lo[3], hi[3];
  float flo[3], fhi[3];
};

// AABB::intersect of the tissue's box with the tool's, strict: a miss on any axis with t_lo >= hi or t_hi <= lo
__device__ __forceinline__ bool ct_miss(const float* __restrict__ box6, const Tool& T) {
  bool miss = false;
#pragma unroll
  for (int k = 0; k < 3; k++) miss = miss || box6[k] >= T.fhi[k] || box6[3 + k] <= T.flo[k];
  return miss;
}

// d(k, j) = (s_j - p_k) . n_j with s = {lo, hi, lo, hi, lo, hi} and n = {-x, +x, -y, +y, -z, +z}, the whole dot product as vec3d::dot forms it
__device__ __forceinline__ double face_dot(const Tool& T, const double p[3], int j) {
  const double* s = (j & 1) ? T.hi : T.lo;
  double n[3] = {0.0, 0.0, 0.0};
  n[j >> 1] = (j & 1) ? 1.0 : -1.0;
  return (s[0] - p[0]) * n[0] + (s[1] - p[1]) * n[1] + (s[2] - p[2]) * n[2];
}

// ---- move ----

// A thread per node (internal order; min and max are exact in any order): the box of (float)(x0 + q)
__global__ __launch_bounds__(kB) void k_ct_tissue_box(int n_nodes, const double* __restrict__ x0, const double* __restrict__ q, float* __restrict__ part) {
  const int i = blockIdx.x * kB + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n_nodes) {
    const size_t b = 3 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; k++) lo[k] = hi[k] = (float)(x0[b + k] + q[b + k]);
  }
  wg_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

// A thread per caller id: a node inside the tool box enters the set with its current position unless it is in it; the workgroup's touched
// and new nodes
__global__ __launch_bounds__(kB) void k_ct_mark(int n_nodes, const double* __restrict__ x0, const double* __restrict__ q, const int* __restrict__ new_of_old, Tool T,
                                                const float* __restrict__ box6, unsigned char* __restrict__ touched, double* __restrict__ first, int* __restrict__ cnt) {
  const int i = blockIdx.x * kB + threadIdx.x;
  const bool miss = ct_miss(box6, T);
  bool in_set = false, is_new = false;
  if (i < n_nodes) {
    in_set = touched[i] != 0;
    if (!miss && !in_set) {
      double p[3];
      bool ok;
      node_position(i, new_of_old, n_nodes, x0, q, p, &ok);
      if (ok && in_box(p, T.lo, T.hi)) {
        touched[i] = 1;
        first[3 * (size_t)i] = p[0]; first[3 * (size_t)i + 1] = p[1]; first[3 * (size_t)i + 2] = p[2];
        in_set = is_new = true;
      }
    }
  }
  const int c_set = wg_count(in_set), c_new = wg_count(is_new);
  if (threadIdx.x == 0) { cnt[2 * (size_t)blockIdx.x] = c_set; cnt[2 * (size_t)blockIdx.x + 1] = c_new; }
}

// one workgroup: exclusive scan of the workgroups' touched counts; off[n] the total, off[n + 1] the new ones
__global__ __launch_bounds__(kB) void k_ct_scan(int n, const int* __restrict__ cnt, int* __restrict__ off) { wg_scan_partials<2>(n, cnt, off); }

// A thread per caller id: a touched node takes its place in the list, and brings its smallest d -- over the six faces ascending with a
// strict <, or for the face that stands -- to the workgroup's (d, node, face) minimum
__global__ __launch_bounds__(kB) void k_ct_face(int n_nodes, int n_blocks, Tool T, const float* __restrict__ box6, const unsigned char* __restrict__ touched,
                                                const double* __restrict__ first, const int* __restrict__ off, int face_in, int* __restrict__ ids,
                                                double* __restrict__ part_d, long long* __restrict__ part_k) {
  const int i = blockIdx.x * kB + threadIdx.x;
  const bool live = !ct_miss(box6, T) && off[n_blocks] > 0;
  const bool hit = live && i < n_nodes && touched[i] != 0;
  int total;
  const int rank = wg_rank(hit, &total);
  double d = INFINITY;
  long long key = LLONG_MAX;
  if (hit) {
    const int pos = off[blockIdx.x] + rank;
    if (pos >= 0 && pos < n_nodes) ids[pos] = i;
    const double p[3] = {first[3 * (size_t)i], first[3 * (size_t)i + 1], first[3 * (size_t)i + 2]};
    if (face_in < 0) {
      int best = 0;
      d = face_dot(T, p, 0);
      for (int j = 1; j < 6; j++) {
        const double dj = face_dot(T, p, j);
        if (dj < d) { d = dj; best = j; }
      }
      key = 8LL * i + best;
    } else {
      d = face_dot(T, p, face_in);
      key = 8LL * i + face_in;
    }
  }
  wg_best<long long, Lowest>(d, key);
  if (threadIdx.x == 0) { part_d[blockIdx.x] = d; part_k[blockIdx.x] = key; }
}

// one workgroup: the minimum of the partials; status, counts, face and closest node of this move
__global__ __launch_bounds__(kB) void k_ct_final(int n_part, int n_nodes, Tool T, const float* __restrict__ box6, const int* __restrict__ off,
                                                 const double* __restrict__ part_d, const long long* __restrict__ part_k, const double* __restrict__ first, int face_in,
                                                 fb_fem_contact_info* __restrict__ res) {
  double d = INFINITY;
  long long key = LLONG_MAX;
  fold_best<long long, Lowest>(n_part, part_d, part_k, d, key);
  wg_best<long long, Lowest>(d, key);
  if (threadIdx.x != 0) return;
  fb_fem_contact_info r;
  r.status = ct_miss(box6, T) ? FB_CONTACT_MISS : (off[n_part] > 0 ? FB_CONTACT_SET : FB_CONTACT_EMPTY);
  r.n_touched = off[n_part]; r.n_new = off[n_part + 1];
  r.face = face_in; r.closest_node = -1; r.n_pushing = 0; r.list_size = 0; r.n_clears = 0;
  r.contact_dist = 0.0;
  r.closest_point[0] = r.closest_point[1] = r.closest_point[2] = 0.0;
  const long long node = key >> 3;
  if (r.status == FB_CONTACT_SET && key != LLONG_MAX && node >= 0 && node < n_nodes) {
    r.face = (int)(key & 7);
    r.closest_node = (int)node;
    r.contact_dist = d;
    for (int k = 0; k < 3; k++) r.closest_point[k] = first[3 * (size_t)node + k];
  }
  *res = r;
}

// A thread per list entry: n_face * max(d(k, face) * coeff, 0); the workgroup's entries greater than zero
__global__ __launch_bounds__(kB) void k_ct_force(int n_nodes, Tool T, double coeff, const fb_fem_contact_info* __restrict__ res, const int* __restrict__ ids,
                                                 const double* __restrict__ first, double* __restrict__ forces, int* __restrict__ push_cnt) {
  const int s = blockIdx.x * kB + threadIdx.x;
  const int face = res->face;
  const bool live = res->status == FB_CONTACT_SET && face >= 0 && face < 6;
  bool pushing = false;
  if (live && s < n_nodes && s < res->n_touched) {
    const int id = ids[s];
    if ((unsigned)id < (unsigned)n_nodes) {
      const double p[3] = {first[3 * (size_t)id], first[3 * (size_t)id + 1], first[3 * (size_t)id + 2]};
      const double v = face_dot(T, p, face) * coeff;
      const double mag = v > 0.0 ? v : 0.0;  // (MATHMAX(v, 0))
      double n[3] = {0.0, 0.0, 0.0};
      n[face >> 1] = (face & 1) ? 1.0 : -1.0;
      forces[3 * (size_t)s] = n[0] * mag; forces[3 * (size_t)s + 1] = n[1] * mag; forces[3 * (size_t)s + 2] = n[2] * mag;
      pushing = mag > 0.0;
    }
  }
  const int c = wg_count(pushing);
  if (threadIdx.x == 0) push_cnt[blockIdx.x] = c;
}

// one workgroup: the pushing entries of all workgroups, the list's length
__global__ __launch_bounds__(kB) void k_ct_push_final(int n_part, const int* __restrict__ push_cnt, fb_fem_contact_info* __restrict__ res) {
  const int all = wg_sum(fold_sum(n_part, push_cnt));
  if (threadIdx.x != 0 || res->status != FB_CONTACT_SET) return;
  res->n_pushing = all;
  res->list_size = res->n_touched;
}

// ---- apply ----

__device__ __forceinline__ bool nonzero3(const double* f) { return f[0] != 0.0 || f[1] != 0.0 || f[2] != 0.0; }

// A thread per list entry: the force to its own node (the ids of a list differ, so no two threads meet)
__global__ __launch_bounds__(kB) void k_ct_direct(int n, const int* __restrict__ ids, const double* __restrict__ f3, const int* __restrict__ new_of_old, int n_nodes,
                                                  double* __restrict__ fext) {
  const int s = blockIdx.x * kB + threadIdx.x;
  if (s >= n) return;
  const int id = ids[s];
  if ((unsigned)id >= (unsigned)n_nodes || !nonzero3(f3 + 3 * (size_t)s)) return;
  const int node = new_of_old ? new_of_old[id] : id;
  if ((unsigned)node >= (unsigned)n_nodes) return;
#pragma unroll
  for (int c = 0; c < 3; c++) fext[3 * (size_t)node + c] += f3[3 * (size_t)s + c];
}

// A wavefront (the workgroup) per source with a force: its ball of rings 1 .. size-1 over the adjacency, then its records.
// tab: the visited nodes, open addressing; order / ring: the same nodes in arrival order, so that ring j's frontier is a range of it.
// The workgroup is one wavefront, and every __syncthreads() is reached by all 64 lanes: the loop bounds around them are read from LDS after
// a barrier or are kernel arguments.
__global__ __launch_bounds__(64) void k_ct_walk(int n, const int* __restrict__ ids, const double* __restrict__ f3, const int* __restrict__ new_of_old, int n_nodes,
                                                const int* __restrict__ bptr, const int* __restrict__ bcol, int n_blocks, int size, int rank_bits,
                                                unsigned long long capacity, unsigned long long* __restrict__ keys, unsigned char* __restrict__ rings,
                                                unsigned long long* __restrict__ walk) {
  __shared__ int tab[kContactTableSlots];
  __shared__ int order[kContactBallMax];
  __shared__ unsigned char ring[kContactBallMax];
  __shared__ int count, overflow;
  __shared__ unsigned long long base_sh;
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= n) return;  // (uniform over the workgroup)
  const int id = ids[s];
  if ((unsigned)id >= (unsigned)n_nodes || !nonzero3(f3 + 3 * (size_t)s)) return;
  const int root = new_of_old ? new_of_old[id] : id;
  if ((unsigned)root >= (unsigned)n_nodes) return;
  for (int k = lane; k < kContactTableSlots; k += 64) tab[k] = -1;
  __syncthreads();
  if (lane == 0) {
    tab[(unsigned)(root * 0x9E3779B1u) >> 21 & (kContactTableSlots - 1)] = root;
    order[0] = root; ring[0] = 0;
    count = 1; overflow = 0;
  }
  __syncthreads();
  int begin = 0;
  for (int j = 1; j < size; j++) {
    const int end = min(count, kContactBallMax);
    const bool stop = overflow != 0 || begin >= end;
    __syncthreads();  // (everybody has read count and overflow before the ring writes them)
    if (stop) break;
    for (int at = begin + lane; at < end; at += 64) {
      const int u = order[at];
      if ((unsigned)u >= (unsigned)n_nodes) continue;
      const int r0 = bptr[u], r1 = bptr[u + 1];
      if (r0 < 0 || r1 < r0 || r1 > n_blocks) continue;
      for (int p = r0; p < r1; p++) {
        const int v = bcol[p];
        if ((unsigned)v >= (unsigned)n_nodes || v == u) continue;
        unsigned slot = ((unsigned)(v * 0x9E3779B1u) >> 21) & (kContactTableSlots - 1);
        bool placed = false;
        for (int probe = 0; probe < kContactProbes; probe++) {
          const int old = atomicCAS(&tab[slot], -1, v);
          if (old == v) { placed = true; break; }
          if (old == -1) {
            const int pos = atomicAdd(&count, 1);
            if (pos >= 0 && pos < kContactBallMax) { order[pos] = v; ring[pos] = (unsigned char)j; }
            else overflow = 1;
            placed = true;
            break;
          }
          slot = (slot + 1) & (kContactTableSlots - 1);
        }
        if (!placed) overflow = 1;
      }
    }
    begin = end;
    __syncthreads();
  }
  __syncthreads();
  if (overflow != 0) {
    if (lane == 0) atomicOr(&walk[1], 1ull);
    return;
  }
  const int n_rec = min(count, kContactBallMax) - 1;
  if (n_rec <= 0) return;
  if (lane == 0) base_sh = atomicAdd(&walk[0], (unsigned long long)n_rec);
  __syncthreads();
  const unsigned long long base = base_sh;
  if (base + (unsigned long long)n_rec > capacity) return;  // (the host sees the cursor beyond the capacity: it grows the buffer and walks again, or falls back)
  for (int k = lane; k < n_rec; k += 64) {
    keys[base + k] = ((unsigned long long)(unsigned)order[1 + k] << rank_bits) | (unsigned long long)(unsigned)s;
    rings[base + k] = ring[1 + k];
  }
}

// A thread per record: the first of a target's segment does that node's additions in the segment's (= ascending source) order
__global__ __launch_bounds__(kB) void k_ct_segments(long long n_rec, const unsigned long long* __restrict__ keys, const unsigned char* __restrict__ rings, int rank_bits, int n,
                                                    const double* __restrict__ f3, const double* __restrict__ mag, int size, int n_nodes, double* __restrict__ fext,
                                                    unsigned long long* __restrict__ walk) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i >= n_rec) return;
  const unsigned long long t = keys[i] >> rank_bits;
  if (i > 0 && (keys[i - 1] >> rank_bits) == t) return;
  if (t >= (unsigned long long)n_nodes) return;
  const unsigned long long rank_mask = (1ull << rank_bits) - 1ull;
  double a[3] = {fext[3 * (size_t)t], fext[3 * (size_t)t + 1], fext[3 * (size_t)t + 2]};
  for (long long k = i; k < n_rec; k++) {
    const unsigned long long key = keys[k];
    if ((key >> rank_bits) != t) break;
    const unsigned long long r = key & rank_mask;
    const int l = rings[k];
    if (r >= (unsigned long long)n || l < 1 || l > size - 1) continue;
    const double m = mag[l];
    a[0] += m * f3[3 * (size_t)r]; a[1] += m * f3[3 * (size_t)r + 1]; a[2] += m * f3[3 * (size_t)r + 2];
  }
  fext[3 * (size_t)t] = a[0]; fext[3 * (size_t)t + 1] = a[1]; fext[3 * (size_t)t + 2] = a[2];
  atomicAdd(&walk[2], 1ull);
}

// ---- host ----

// `buf` covers n entries of `per` values: grown with its first n_old entries kept and the rest zero
template <class T>
int grow_keep(hipStream_t s, DevBuf<T>& buf, size_t n_old, size_t n, size_t per) {
  DevBuf<T> next;
  FB_TRY(next.alloc(n * per));
  FB_HIP(hipMemsetAsync(next.p, 0, sizeof(T) * n * per, s));
  if (n_old && buf.p) FB_HIP(hipMemcpyAsync(next.p, buf.p, sizeof(T) * n_old * per, hipMemcpyDeviceToDevice, s));
  FB_HIP(hipStreamSynchronize(s));  // (the old allocation is freed when `next` leaves)
  buf.swap(next);
  return FB_OK;
}

int ensure_state(hipStream_t s, ContactWork& C, int n_nodes) {
  if (C.n_state >= n_nodes && C.touched.p) return FB_OK;
  const size_t n_old = C.touched.p ? (size_t)C.n_state : 0, n = (size_t)n_nodes;
  FB_TRY(grow_keep(s, C.touched, n_old, n, 1));
  FB_TRY(grow_keep(s, C.first, n_old, n, 3));
  FB_TRY(grow_keep(s, C.ids, n_old, n, 1));
  FB_TRY(grow_keep(s, C.forces, n_old, n, 3));
  C.n_state = n_nodes;
  return FB_OK;
}

inline const int* new_of_old_dev(const fb_fem_s* h) { return h->ren.active ? h->ren.d_new_of_old.p : nullptr; }

int contact_move(fb_fem_s* h, const double lo[3], const double hi[3], double coeff, fb_fem_contact_info* out) {
  ContactWork& C = h->contact;
  hipStream_t s = h->stream;
  const int n_nodes = h->plan.n_global;
  FB_TRY(ensure_state(s, C, n_nodes));
  const int nblk = blocks_for(n_nodes);
  FB_TRY(C.box_part.reserve((size_t)6 * nblk)); FB_TRY(C.box6.reserve(6));
  FB_TRY(C.cnt.reserve((size_t)2 * nblk)); FB_TRY(C.off.reserve((size_t)nblk + 2));
  FB_TRY(C.part_d.reserve((size_t)nblk)); FB_TRY(C.part_k.reserve((size_t)nblk)); FB_TRY(C.push_cnt.reserve((size_t)nblk)); FB_TRY(C.res.reserve(1));
  Tool T;
  for (int k = 0; k < 3; k++) { T.lo[k] = lo[k]; T.hi[k] = hi[k]; T.flo[k] = (float)lo[k]; T.fhi[k] = (float)hi[k]; }
  const int* noo = new_of_old_dev(h);
  const int face_in = C.info.face;
  FB_TRY(launch_1d(k_ct_tissue_box, n_nodes, s, n_nodes, h->x0.p, h->q.p, C.box_part.p));
  FB_TRY(launch_grid(k_box_final<float>, dim3(1), s, nblk, C.box_part.p, C.box6.p));
  FB_TRY(launch_1d(k_ct_mark, n_nodes, s, n_nodes, h->x0.p, h->q.p, noo, T, C.box6.p, C.touched.p, C.first.p, C.cnt.p));
  FB_TRY(launch_grid(k_ct_scan, dim3(1), s, nblk, C.cnt.p, C.off.p));
  FB_TRY(launch_1d(k_ct_face, n_nodes, s, n_nodes, nblk, T, C.box6.p, C.touched.p, C.first.p, C.off.p, face_in, C.ids.p, C.part_d.p, C.part_k.p));
  FB_TRY(launch_grid(k_ct_final, dim3(1), s, nblk, n_nodes, T, C.box6.p, C.off.p, C.part_d.p, C.part_k.p, C.first.p, face_in, C.res.p));
  FB_TRY(launch_1d(k_ct_force, n_nodes, s, n_nodes, T, coeff, C.res.p, C.ids.p, C.first.p, C.forces.p, C.push_cnt.p));
  FB_TRY(launch_grid(k_ct_push_final, dim3(1), s, nblk, C.push_cnt.p, C.res.p));
  fb_fem_contact_info r;
  FB_TRY(C.res.download(&r, 1, s));
  if (r.status < FB_CONTACT_MISS || r.status > FB_CONTACT_SET || r.n_touched < 0 || r.n_touched > n_nodes || r.list_size < 0 || r.list_size > n_nodes || r.face < -1 || r.face > 5)
    return fail(FB_EDEVICE, "contact move: result out of range (status %d, %d touched, face %d)", r.status, r.n_touched, r.face);
  const int n_clears = C.info.n_clears;
  if (r.status == FB_CONTACT_SET) C.info = r;
  else { C.info.status = r.status; C.info.n_new = 0; }  // (nothing changed)
  C.info.n_clears = n_clears;
  if (out) *out = C.info;
  return FB_OK;
}

// the node adjacency of the current mesh on the device, internal ids: the device-built plan's pattern, or the host-built plan's uploaded once
// per mesh generation; false: none at hand (the level arrays sweep the elements instead)
int contact_pattern(fb_fem_s* h, const int** bptr, const int** bcol, int* n_blocks, bool* have) {
  ContactWork& C = h->contact;
  const FemPlan& P = h->plan;
  *have = false;
  if (h->device_plan) {
    if (!h->csr_ready || !h->d_bptr.p || !h->d_bcol.p) return FB_OK;
    *bptr = h->d_bptr.p; *bcol = h->d_bcol.p; *n_blocks = P.n_blocks; *have = true;
    return FB_OK;
  }
  if (P.bptr.size() != (size_t)P.n_owned + 1 || P.n_owned != P.n_global || (long long)P.bcol.size() < P.bptr.back()) return FB_OK;
  if (!C.pat_valid) {
    FB_TRY(C.pat_ptr.upload(P.bptr.data(), P.bptr.size(), h->stream));
    FB_TRY(C.pat_col.upload(P.bcol.data(), (size_t)std::max(1, P.bptr.back()), h->stream));
    C.pat_valid = true;
  }
  *bptr = C.pat_ptr.p; *bcol = C.pat_col.p; *n_blocks = P.bptr.back(); *have = true;
  return FB_OK;
}

long long record_budget() {
  const char* env = getenv("FEMBRAIN_CONTACT_MAX_RECORDS");
  if (env && *env) return std::max(0LL, atoll(env));
  return kContactMaxRecords;
}

int contact_apply(fb_fem_s* h, int size, fb_fem_contact_spread_info* out) {
  ContactWork& C = h->contact;
  hipStream_t s = h->stream;
  const int n_nodes = h->plan.n_global, n = C.info.list_size;
  fb_fem_contact_spread_info I = {n, C.info.n_pushing, FB_CONTACT_SPREAD_RECORDS, 0, 0};
  if (n <= 0 || C.info.n_pushing <= 0) { if (out) *out = I; return FB_OK; }  // (an empty list, or forces that are all zero: nothing to add)
  const int* noo = new_of_old_dev(h);
  FB_TRY(launch_1d(k_ct_direct, n, s, n, C.ids.p, C.forces.p, noo, n_nodes, h->fext.p));
  if (size <= 1 || h->plan.n_tets <= 0) { if (out) *out = I; return FB_OK; }
  if (C.mag_size != size) {
    double mag[256];
    mag[0] = 1.0;
    for (int j = 1; j < 256; j++) mag[j] = j < size ? 1.0 * (size - j) / static_cast<double>(size) : 0.0;
    FB_TRY(C.mag.upload(mag, 256, s));
    C.mag_size = size;
  }
  const int *bptr = nullptr, *bcol = nullptr;
  int n_blocks = 0;
  bool records = false;
  FB_TRY(contact_pattern(h, &bptr, &bcol, &n_blocks, &records));
  const long long budget = record_budget();
  const int rank_bits = bits_of(n), node_bits = bits_of(n_nodes);
  unsigned long long w[3] = {0, 0, 0};
  if (records) {
    FB_TRY(C.walk.reserve(3));
    for (int attempt = 0; attempt < 2; attempt++) {
      if (attempt == 0 && !C.keys.p) {  // (a first guess: a ring-2 ball of a tet mesh per pushing source; the walk says what it takes)
        const size_t guess = (size_t)std::min<long long>(std::max<long long>(budget, 1), std::max<long long>(4096, 64LL * C.info.n_pushing));
        FB_TRY(C.keys.reserve(guess)); FB_TRY(C.rings.reserve(guess));
      }
      const unsigned long long capacity = std::min(C.keys.n, C.rings.n);
      FB_TRY(C.walk.zero(s));
      FB_TRY(launch_shape(k_ct_walk, dim3((unsigned)n), dim3(64), s, n, C.ids.p, C.forces.p, noo, n_nodes, bptr, bcol, n_blocks, size, rank_bits, capacity, C.keys.p, C.rings.p,
                          C.walk.p));
      FB_TRY(C.walk.download(w, 2, s));
      if (w[1] != 0 || (long long)w[0] > budget) { records = false; break; }
      if (w[0] <= capacity) break;
      if (attempt == 1) return fail(FB_EDEVICE, "contact apply: %llu records after the buffer was grown to %llu", w[0], capacity);
      FB_TRY(C.keys.reserve((size_t)w[0])); FB_TRY(C.rings.reserve((size_t)w[0]));
    }
  }
  if (!records) {
    I.path = FB_CONTACT_SPREAD_LEVELS;
    I.n_targets = -1;
    I.n_records = w[1] != 0 ? -1 : (long long)w[0];
    FB_TRY(haptic_spread_rings(s, h->hap, n_nodes, h->plan.n_tets, h->tets.p, noo, n, C.ids.p, C.forces.p, C.mag.p, size, h->fext.p));
    if (out) *out = I;
    return FB_OK;
  }
  const long long n_rec = (long long)w[0];
  I.n_records = n_rec;
  if (n_rec > 0) {
    FB_TRY(C.keys_sorted.reserve((size_t)n_rec)); FB_TRY(C.rings_sorted.reserve((size_t)n_rec));
    FB_TRY(sort_pairs(C.temp, s, C.keys.p, C.keys_sorted.p, C.rings.p, C.rings_sorted.p, (size_t)n_rec, (unsigned)(rank_bits + node_bits)));
    FB_TRY(launch_1d(k_ct_segments, n_rec, s, n_rec, C.keys_sorted.p, C.rings_sorted.p, rank_bits, n, C.forces.p, C.mag.p, size, n_nodes, h->fext.p, C.walk.p));
    FB_TRY(C.walk.download(w, 3, s));
    I.n_targets = (int)w[2];
  }
  if (out) *out = I;
  return FB_OK;
}

}  // namespace

void contact_mesh_changed(ContactWork& C, bool in_place) {
  C.pat_valid = false;
  if (in_place || !C.touched.p) return;
  const int n_clears = C.info.n_clears + 1;
  C.info = fb_fem_contact_info{0, 0, 0, -1, -1, 0, 0, n_clears, 0.0, {0.0, 0.0, 0.0}};
  C.n_state = 0;  // (the next move starts from arrays of zeros sized for the new mesh)
}

}  // namespace fb

// ---- the C ABI ----

int fb_fem_contact_move(fb_fem_t h, const double lo[3], const double hi[3], double force_coeff, fb_fem_contact_info* out) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_contact_move is for unsharded handles");
  if (!lo || !hi) return fail(FB_EINVAL, "null tool box");
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || lo[k] > hi[k]) return fail(FB_EINVAL, "tool box [%g, %g] on axis %d", lo[k], hi[k], k);
  if (!std::isfinite(force_coeff)) return fail(FB_EINVAL, "force coefficient %g", force_coeff);
  if (h->plan.n_global <= 0 || h->plan.n_global >= (1 << 28)) return fail(FB_EINVAL, "fb_fem_contact_move: %d nodes", h->plan.n_global);
  return contact_move(h, lo, hi, force_coeff, out);
}

int fb_fem_contact_info_get(fb_fem_t h, fb_fem_contact_info* out) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_contact_info_get is for unsharded handles");
  if (!out) return fail(FB_EINVAL, "null contact info");
  *out = h->contact.info;
  return FB_OK;
}

int fb_fem_contact_reset(fb_fem_t h, int keep_face) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_contact_reset is for unsharded handles");
  ContactWork& C = h->contact;
  const int face = keep_face ? C.info.face : -1, n_clears = C.info.n_clears;
  if (C.touched.p && C.n_state > 0) FB_HIP(hipMemsetAsync(C.touched.p, 0, (size_t)C.n_state, h->stream));
  C.info = fb_fem_contact_info{0, 0, 0, face, -1, 0, 0, n_clears, 0.0, {0.0, 0.0, 0.0}};
  return FB_OK;
}

int fb_fem_read_contact(fb_fem_t h, int* ids, double* first_xyz, double* forces3) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_read_contact is for unsharded handles");
  ContactWork& C = h->contact;
  const int n = C.info.list_size;
  if (n <= 0 || n > C.n_state) return FB_OK;
  std::vector<int> host_ids((size_t)n);
  FB_TRY(C.ids.download(host_ids.data(), (size_t)n, h->stream));
  if (ids) memcpy(ids, host_ids.data(), sizeof(int) * (size_t)n);
  if (forces3) FB_TRY(C.forces.download(forces3, (size_t)3 * n, h->stream));
  if (first_xyz) {  // (an inspection call: the whole array comes back and the list's rows are taken from it)
    std::vector<double> all((size_t)3 * C.n_state);
    FB_TRY(C.first.download(all.data(), all.size(), h->stream));
    for (int k = 0; k < n; k++) {
      const int id = host_ids[(size_t)k];
      if (id < 0 || id >= C.n_state) return fail(FB_EDEVICE, "contact list entry %d is node %d", k, id);
      memcpy(first_xyz + 3 * (size_t)k, all.data() + 3 * (size_t)id, sizeof(double) * 3);
    }
  }
  return FB_OK;
}

int fb_fem_contact_apply(fb_fem_t h, int neighbourhood_size, fb_fem_contact_spread_info* out) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_contact_apply is for unsharded handles");
  if (neighbourhood_size < 1 || neighbourhood_size > 255) return fail(FB_EINVAL, "neighbourhood size %d outside [1, 255]", neighbourhood_size);
  return contact_apply(h, neighbourhood_size, out);
}
