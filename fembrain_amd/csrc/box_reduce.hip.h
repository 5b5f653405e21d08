// The float bounding box of a launch's points, shared by the units that report one (surface.hip, embed.hip): every workgroup folds its
// threads' boxes into a six-float partial, k_box_final folds the partials (a second, single-workgroup launch: no counter to reset, and
// min / max are exact in any order).  Each unit gets its own copy of the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.hip.h"

namespace fb {
namespace {

__device__ __forceinline__ void box_merge(float* lo, float* hi) {  // over the wavefront
#pragma unroll
  for (int k = 0; k < 3; k++)
    for (int d = 32; d >= 1; d >>= 1) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], d));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d));
    }
}

// every thread of the workgroup calls it with its own box (empty: +inf / -inf); out6 receives lo[3], hi[3] of the workgroup
__device__ __forceinline__ void box_workgroup(float* lo, float* hi, float* __restrict__ out6) {
  box_merge(lo, hi);
  __shared__ float sh[kB / 64][6];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; k++) { sh[wave][k] = lo[k]; sh[wave][3 + k] = hi[k]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    float r = sh[0][threadIdx.x];
    for (int w = 1; w < kB / 64; w++) r = threadIdx.x < 3 ? fminf(r, sh[w][threadIdx.x]) : fmaxf(r, sh[w][threadIdx.x]);
    out6[threadIdx.x] = r;
  }
}

__global__ __launch_bounds__(kB) void k_box_final(int n_part, const float* __restrict__ part, float* __restrict__ box) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < n_part; b += kB)
    for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], part[6 * (size_t)b + k]); hi[k] = fmaxf(hi[k], part[6 * (size_t)b + 3 + k]); }
  box_workgroup(lo, hi, box);
}

}  // namespace
}  // namespace fb
