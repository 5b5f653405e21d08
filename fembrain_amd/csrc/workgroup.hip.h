// The in-workgroup folds, ranks and scans of the mesh-side kernels (surface, haptic, contact, stress, parts, embed, embed_touch, renumber),
// written once for workgroups of kB = 256 threads: four wavefronts of 64.
//
// The contract of everything below:
//  - Every thread of the workgroup calls a wg_* primitive (every lane of the wavefront a wf_* one), idle threads with the neutral value:
//    0, false, the worst (value, key) pair, the empty box (+inf / -inf).
//  - Where the result is: wg_sum, wg_max, wg_count and wg_rank return it to every thread; wg_best leaves it in thread 0 (the other
//    threads hold their wavefront's); wg_box writes the workgroup's six values through its threads 0..5; wg_scan_partials writes its
//    array.  Of the wavefront level, wf_sum(double) is valid in lane 0 only, everything else in every lane.
//  - The result does not depend on the launch shape.  Minima, maxima, integer sums and counts are exact in any order.  The fp64 sum is one
//    fixed tree: each wavefront folds its upper half onto its lower (__shfl_down by 32, 16, .. 1), then (w0 + w1) + (w2 + w3) -- the
//    same bits from call to call.  A best pair is the lexicographic optimum of (value, key): of equal values the lowest key wins, which
//    is a total order, so the pairing inside the fold does not matter.
//  - A primitive may be called any number of times in one kernel, and different primitives one after another: each one that goes through
//    LDS ends with a barrier behind its last read, so its words are free when it returns.  (Two barriers a call; nothing for the caller
//    to remember.)
//  - Partials leave a workgroup through thread 0 (or wg_box's six threads) and a second, single-workgroup launch folds them: thread t
//    takes the partials t, t + 256, ... in that order (fold_sum, fold_best, k_box_final) and the same primitive folds the threads.
//    No floating-point atomics, no counter to reset.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.hip.h"

namespace fb {

constexpr int kWaves = kB / 64;

// ---- (value, key) orders: better(v, k, than_v, than_k) ----
// (written out, not one derived from the other by negating values: the order of +-0 and a NaN that never wins stay what they are)
struct Lowest {
  template <class Key>
  __device__ __forceinline__ bool operator()(double v, Key k, double bv, Key bk) const { return v < bv || (v == bv && k < bk); }
};
struct Highest {
  template <class Key>
  __device__ __forceinline__ bool operator()(double v, Key k, double bv, Key bk) const { return v > bv || (v == bv && k < bk); }
};

// ---- the wavefront: no LDS, no barrier ----

__device__ __forceinline__ double wf_sum(double v) {  // the tree's value in lane 0
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o);
  return v;
}
__device__ __forceinline__ int wf_sum(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wf_max(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float lower_of(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float higher_of(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double lower_of(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double higher_of(double a, double b) { return fmax(a, b); }
template <class T>
__device__ __forceinline__ T wf_min(T v) {
  for (int o = 32; o >= 1; o >>= 1) v = lower_of(v, __shfl_xor(v, o));
  return v;
}
template <class T>
__device__ __forceinline__ T wf_max(T v) {
  for (int o = 32; o >= 1; o >>= 1) v = higher_of(v, __shfl_xor(v, o));
  return v;
}
// one exchange of the butterfly, with the lane o away (a caller that folds several pairs interleaves their steps: stress.hip)
template <class Key, class Better>
__device__ __forceinline__ void wf_best_step(double& v, Key& k, int o) {
  const double ov = __shfl_xor(v, o);
  const Key ok = __shfl_xor(k, o);
  if (Better()(ov, ok, v, k)) { v = ov; k = ok; }
}
template <class Key, class Better>
__device__ __forceinline__ void wf_best(double& v, Key& k) {
  for (int o = 32; o >= 1; o >>= 1) wf_best_step<Key, Better>(v, k, o);
}
// the wavefront's set flags, and those of the lanes below this one
__device__ __forceinline__ int wf_count(bool flag) { return __popcll(__ballot(flag)); }
__device__ __forceinline__ int wf_rank(bool flag) { return __popcll(__ballot(flag) & ((1ull << (threadIdx.x & 63)) - 1ull)); }

// ---- the workgroup ----

__device__ __forceinline__ double wg_sum(double v) {
  static_assert(kWaves == 4, "the sum's tree is written for four wavefronts");
  v = wf_sum(v);
  __shared__ double sh[kWaves];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return s;
}

__device__ __forceinline__ int wg_sum(int v) {
  v = wf_sum(v);
  __shared__ int sh[kWaves];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < kWaves; w++) s += sh[w];
  __syncthreads();
  return s;
}

__device__ __forceinline__ int wg_max(int v) {
  v = wf_max(v);
  __shared__ int sh[kWaves];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  for (int w = 0; w < kWaves; w++) v = max(v, sh[w]);
  __syncthreads();
  return v;
}

// the best (value, key) of the workgroup; in thread 0
template <class Key, class Better>
__device__ __forceinline__ void wg_best(double& v, Key& k) {
  wf_best<Key, Better>(v, k);
  __shared__ double sv[kWaves];
  __shared__ Key sk[kWaves];
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; sk[threadIdx.x >> 6] = k; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kWaves; w++)
      if (Better()(sv[w], sk[w], v, k)) { v = sv[w]; k = sk[w]; }
  __syncthreads();
}

// the flagged threads of the workgroup in front of this one, in thread order (a flagged thread's place in the compaction); *total: all
__device__ __forceinline__ int wg_rank(bool flag, int* total) {
  const int in_wave = wf_count(flag), wave = threadIdx.x >> 6;
  __shared__ int wc[kWaves];
  if ((threadIdx.x & 63) == 0) wc[wave] = in_wave;
  __syncthreads();
  int before = wf_rank(flag), all = 0;
  for (int w = 0; w < kWaves; w++) {
    if (w < wave) before += wc[w];
    all += wc[w];
  }
  __syncthreads();
  *total = all;
  return before;
}
__device__ __forceinline__ int wg_count(bool flag) {
  int total;
  wg_rank(flag, &total);
  return total;
}

// the box of the threads' boxes: out6 receives lo[3], hi[3]
template <class T>
__device__ __forceinline__ void wg_box(T* lo, T* hi, T* __restrict__ out6) {
  __shared__ T sh[kWaves][6];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    lo[k] = wf_min(lo[k]);
    hi[k] = wf_max(hi[k]);
    if ((threadIdx.x & 63) == 0) { sh[wave][k] = lo[k]; sh[wave][3 + k] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    T r = sh[0][threadIdx.x];
    for (int w = 1; w < kWaves; w++) r = threadIdx.x < 3 ? lower_of(r, sh[w][threadIdx.x]) : higher_of(r, sh[w][threadIdx.x]);
    out6[threadIdx.x] = r;
  }
  __syncthreads();
}

// One workgroup over n entries of NC interleaved per-workgroup counts (cnt[NC b + c]): off[b] = the sum of column 0 in front of entry b,
// off[n] its total, off[n + c] the total of column c.  Thread t owns the consecutive run of ceil(n / kB) entries, its base is the sum of
// the runs before it.
template <int NC>
__device__ __forceinline__ void wg_scan_partials(int n, const int* __restrict__ cnt, int* __restrict__ off) {
  const int per = (n + kB - 1) / kB;
  const int first = min((int)threadIdx.x * per, n), last = min(first + per, n);
  __shared__ int sh[NC][kB];
#pragma unroll
  for (int c = 0; c < NC; c++) {
    int mine = 0;
    for (int b = first; b < last; b++) mine += cnt[NC * (size_t)b + c];
    sh[c][threadIdx.x] = mine;
  }
  __syncthreads();
  int base = 0;
  for (int t = 0; t < (int)threadIdx.x; t++) base += sh[0][t];
  for (int b = first; b < last; b++) { off[b] = base; base += cnt[NC * (size_t)b]; }
  if (threadIdx.x == kB - 1) {
    off[n] = base;
    for (int c = 1; c < NC; c++) {
      int all = 0;
      for (int t = 0; t < kB; t++) all += sh[c][t];
      off[n + c] = all;
    }
  }
  __syncthreads();
}

// ---- the single-workgroup final's opening: thread t folds the partials t, t + kB, ... in that order ----

__device__ __forceinline__ double fold_sum(int n_part, const double* __restrict__ part) {
  double v = 0.0;
  for (int b = threadIdx.x; b < n_part; b += kB) v += part[b];
  return v;
}
__device__ __forceinline__ int fold_sum(int n_part, const int* __restrict__ part) {
  int v = 0;
  for (int b = threadIdx.x; b < n_part; b += kB) v += part[b];
  return v;
}
// (v, k) come in as the worst pair
template <class Key, class Better>
__device__ __forceinline__ void fold_best(int n_part, const double* __restrict__ part_v, const Key* __restrict__ part_k, double& v, Key& k) {
  for (int b = threadIdx.x; b < n_part; b += kB)
    if (Better()(part_v[b], part_k[b], v, k)) { v = part_v[b]; k = part_k[b]; }
}

namespace {

// the box of n_part six-value partials (each unit gets its own copy of the kernel)
template <class T>
__global__ __launch_bounds__(kB) void k_box_final(int n_part, const T* __restrict__ part, T* __restrict__ box) {
  T lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < n_part; b += kB)
    for (int k = 0; k < 3; k++) { lo[k] = lower_of(lo[k], part[6 * (size_t)b + k]); hi[k] = higher_of(hi[k], part[6 * (size_t)b + 3 + k]); }
  wg_box(lo, hi, box);
}

}  // namespace
}  // namespace fb
