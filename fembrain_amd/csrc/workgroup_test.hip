// The direct test of the in-workgroup primitives (workgroup.hip.h) and of k_run_bounds (mesh_device.hip.h): fb_test_workgroup of
// include/fembrain_hip_testing.h.  Every case is the two-launch pattern the mesh-side units use -- a thread per item with the idle threads
// of the last workgroup carrying the neutral value, per-workgroup partials, a single-workgroup final -- on the default stream of device 0.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/fembrain_hip_testing.h"
#include "common.h"
#include "launch.hip.h"
#include "mesh_device.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

constexpr int kGuard = FB_TEST_WG_GUARD;

__global__ __launch_bounds__(kB) void k_t_sum(int n, const double* __restrict__ v, double* __restrict__ part) {
  const int i = blockIdx.x * kB + threadIdx.x;
  const double s = wg_sum(i < n ? v[i] : 0.0);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(kB) void k_t_sum_final(int n_part, const double* __restrict__ part, double* __restrict__ out) {
  const double s = wg_sum(fold_sum(n_part, part));
  if (threadIdx.x == 0) *out = s;
}

template <class Key, class Better>
__global__ __launch_bounds__(kB) void k_t_best(int n, const double* __restrict__ v, const long long* __restrict__ keys, double worst, double* __restrict__ part_v,
                                               Key* __restrict__ part_k) {
  const int i = blockIdx.x * kB + threadIdx.x;
  double d = worst;
  Key k = std::numeric_limits<Key>::max();
  if (i < n) { d = v[i]; k = (Key)keys[i]; }
  wg_best<Key, Better>(d, k);
  if (threadIdx.x == 0) { part_v[blockIdx.x] = d; part_k[blockIdx.x] = k; }
}
template <class Key, class Better>
__global__ __launch_bounds__(kB) void k_t_best_final(int n_part, const double* __restrict__ part_v, const Key* __restrict__ part_k, double worst, double* __restrict__ out_v,
                                                     long long* __restrict__ out_k) {
  double d = worst;
  Key k = std::numeric_limits<Key>::max();
  fold_best<Key, Better>(n_part, part_v, part_k, d, k);
  wg_best<Key, Better>(d, k);
  if (threadIdx.x == 0) { *out_v = d; *out_k = (long long)k; }
}

// cnt[2 b] = the set flags of workgroup b, cnt[2 b + 1] = its items without one: the same primitive twice in one kernel
__global__ __launch_bounds__(kB) void k_t_count(int n, const unsigned char* __restrict__ flags, int* __restrict__ cnt) {
  const int i = blockIdx.x * kB + threadIdx.x;
  const bool on = i < n && flags[i] != 0;
  const int c_on = wg_count(on), c_off = wg_count(i < n && !on);
  if (threadIdx.x == 0) { cnt[2 * (size_t)blockIdx.x] = c_on; cnt[2 * (size_t)blockIdx.x + 1] = c_off; }
}
// one workgroup: the scan, and behind it in the same kernel off[n + 2] = the integer sum, off[n + 3] = the integer maximum of column 0
__global__ __launch_bounds__(kB) void k_t_scan(int n, const int* __restrict__ cnt, int* __restrict__ off) {
  wg_scan_partials<2>(n, cnt, off);
  int sum = 0, most = 0;
  for (int b = threadIdx.x; b < n; b += kB) { sum += cnt[2 * (size_t)b]; most = max(most, cnt[2 * (size_t)b]); }
  sum = wg_sum(sum);
  most = wg_max(most);
  if (threadIdx.x == 0) { off[n + 2] = sum; off[n + 3] = most; }
}
// out[i] = the set flags in front of item i; out[n .. n + 4) = what k_t_scan left behind the offsets
__global__ __launch_bounds__(kB) void k_t_rank(int n, const unsigned char* __restrict__ flags, const int* __restrict__ off, long long* __restrict__ out) {
  const int i = blockIdx.x * kB + threadIdx.x;
  int total;
  const int rank = wg_rank(i < n && flags[i] != 0, &total);
  if (i < n) out[i] = off[blockIdx.x] + rank;
  if (i < 4) out[n + i] = off[gridDim.x + i];
}

template <class T>
__global__ __launch_bounds__(kB) void k_t_box(int n, const double* __restrict__ xyz, T* __restrict__ part) {
  const int i = blockIdx.x * kB + threadIdx.x;
  T lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n)
    for (int k = 0; k < 3; k++) lo[k] = hi[k] = (T)xyz[3 * (size_t)i + k];
  wg_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

int run_sum(int n, const double* values, double* out_d) {
  const int nblk = blocks_for(n);
  DevBuf<double> v, part;
  FB_TRY(v.upload(values, (size_t)n, 0)); FB_TRY(part.alloc((size_t)nblk + 1));
  FB_TRY(launch_1d(k_t_sum, n, 0, n, v.p, part.p));
  FB_TRY(launch_grid(k_t_sum_final, dim3(1), 0, nblk, part.p, part.p + nblk));
  return part.download(out_d, 1, 0, (size_t)nblk);
}

template <class Key, class Better>
int run_best(int n, const double* values, const long long* keys, double worst, double* out_d, long long* out_i) {
  const int nblk = blocks_for(n);
  DevBuf<double> v, part_v;
  DevBuf<long long> k, out_k;
  DevBuf<Key> part_k;
  FB_TRY(v.upload(values, (size_t)n, 0)); FB_TRY(k.upload(keys, (size_t)n, 0));
  FB_TRY(part_v.alloc((size_t)nblk + 1)); FB_TRY(part_k.alloc((size_t)nblk)); FB_TRY(out_k.alloc(1));
  FB_TRY(launch_1d(k_t_best<Key, Better>, n, 0, n, v.p, k.p, worst, part_v.p, part_k.p));
  FB_TRY(launch_grid(k_t_best_final<Key, Better>, dim3(1), 0, nblk, part_v.p, part_k.p, worst, part_v.p + nblk, out_k.p));
  FB_TRY(part_v.download(out_d, 1, 0, (size_t)nblk));
  return out_k.download(out_i, 1, 0);
}

int run_ranks(int n, const unsigned char* flags, long long* out_i) {
  const int nblk = blocks_for(n);
  DevBuf<unsigned char> f;
  DevBuf<int> cnt, off;
  DevBuf<long long> out;
  FB_TRY(f.upload(flags, (size_t)n, 0));
  FB_TRY(cnt.alloc((size_t)2 * nblk)); FB_TRY(off.alloc((size_t)nblk + 4)); FB_TRY(out.alloc((size_t)n + 4));
  FB_TRY(launch_1d(k_t_count, n, 0, n, f.p, cnt.p));
  FB_TRY(launch_grid(k_t_scan, dim3(1), 0, nblk, cnt.p, off.p));
  FB_TRY(launch_1d(k_t_rank, n, 0, n, f.p, off.p, out.p));
  return out.download(out_i, (size_t)n + 4, 0);
}

template <class T>
int run_box(int n, const double* xyz, double* out_d) {
  const int nblk = blocks_for(n);
  DevBuf<double> p;
  DevBuf<T> part;
  FB_TRY(p.upload(xyz, (size_t)3 * n, 0)); FB_TRY(part.alloc((size_t)6 * nblk + 6));
  FB_TRY(launch_1d(k_t_box<T>, n, 0, n, p.p, part.p));
  FB_TRY(launch_grid(k_box_final<T>, dim3(1), 0, nblk, part.p, part.p + 6 * (size_t)nblk));
  T box[6];
  FB_TRY(part.download(box, 6, 0, (size_t)6 * nblk));
  for (int k = 0; k < 6; k++) out_d[k] = (double)box[k];
  return FB_OK;
}

int run_bounds(int n, int m, const long long* keys, long long* out_i) {
  const size_t len = (size_t)m + kGuard;
  for (int j = 0; j < n; j++)
    if (keys[j] < 0 || keys[j] >= (long long)len || (j && keys[j] < keys[j - 1])) return fail(FB_EINVAL, "fb_test_workgroup: key %d is not sorted or outside [0, %zu)", j, len);
  std::vector<uint32_t> k32((size_t)n);
  for (int j = 0; j < n; j++) k32[(size_t)j] = (uint32_t)keys[j];
  std::vector<int> init(2 * len, 0), got(2 * len);
  for (int g = 0; g < kGuard; g++) init[(size_t)m + g] = init[len + m + g] = -1;  // (nothing may write behind the m keys)
  DevBuf<uint32_t> k;
  DevBuf<int> lohi;
  FB_TRY(k.upload(k32, 0)); FB_TRY(lohi.upload(init, 0));
  FB_TRY(launch_1d(k_run_bounds<>, n, 0, n, k.p, (uint32_t)m, lohi.p, lohi.p + len));
  FB_TRY(lohi.download(got.data(), got.size(), 0));
  for (size_t j = 0; j < got.size(); j++) out_i[j] = got[j];
  return FB_OK;
}

}  // namespace
}  // namespace fb

int fb_test_workgroup(int what, int n, int m, const double* values, const long long* keys, const unsigned char* flags, double* out_d, long long* out_i) {
  using namespace fb;
  if (n < 1 || n > (1 << 24)) return fail(FB_EINVAL, "fb_test_workgroup: %d items outside [1, 2^24]", n);
  const bool best = what >= FB_TEST_WG_BEST_LOW_INT && what <= FB_TEST_WG_BEST_HIGH_LL, box = what == FB_TEST_WG_BOX_FLOAT || what == FB_TEST_WG_BOX_DOUBLE;
  if (what != FB_TEST_WG_SUM && !best && what != FB_TEST_WG_RANKS && !box && what != FB_TEST_WG_RUN_BOUNDS) return fail(FB_EINVAL, "fb_test_workgroup: no case %d", what);
  if ((what == FB_TEST_WG_SUM || best || box) && (!values || !out_d)) return fail(FB_EINVAL, "fb_test_workgroup: case %d needs values and out_d", what);
  if ((best || what == FB_TEST_WG_RUN_BOUNDS) && (!keys || !out_i)) return fail(FB_EINVAL, "fb_test_workgroup: case %d needs keys and out_i", what);
  if (what == FB_TEST_WG_BEST_LOW_INT || what == FB_TEST_WG_BEST_HIGH_INT)
    for (int j = 0; j < n; j++)
      if (keys[j] < INT_MIN || keys[j] > INT_MAX) return fail(FB_EINVAL, "fb_test_workgroup: key %d does not fit an int", j);
  if (what == FB_TEST_WG_RANKS && (!flags || !out_i)) return fail(FB_EINVAL, "fb_test_workgroup: case %d needs flags and out_i", what);
  if (what == FB_TEST_WG_RUN_BOUNDS && (m < 1 || m > (1 << 24))) return fail(FB_EINVAL, "fb_test_workgroup: %d keys outside [1, 2^24]", m);
  FB_HIP(hipSetDevice(0));
  switch (what) {
    case FB_TEST_WG_SUM: return run_sum(n, values, out_d);
    case FB_TEST_WG_BEST_LOW_INT: return run_best<int, Lowest>(n, values, keys, INFINITY, out_d, out_i);
    case FB_TEST_WG_BEST_HIGH_INT: return run_best<int, Highest>(n, values, keys, -INFINITY, out_d, out_i);
    case FB_TEST_WG_BEST_LOW_LL: return run_best<long long, Lowest>(n, values, keys, INFINITY, out_d, out_i);
    case FB_TEST_WG_BEST_HIGH_LL: return run_best<long long, Highest>(n, values, keys, -INFINITY, out_d, out_i);
    case FB_TEST_WG_RANKS: return run_ranks(n, flags, out_i);
    case FB_TEST_WG_BOX_FLOAT: return run_box<float>(n, values, out_d);
    case FB_TEST_WG_BOX_DOUBLE: return run_box<double>(n, values, out_d);
    default: return run_bounds(n, m, keys, out_i);
  }
}
