// The lexicographic (value, id) minimum of a workgroup of kB threads: what fb_fem_pick_vertex (haptic.hip) and the picks on an
// embedding (embed_touch.hip) fold their per-thread candidates with.  Of equal values the lowest id wins, whatever the launch shape.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.hip.h"

namespace fb {

__device__ __forceinline__ bool closer(double d, int i, double bd, int bi) { return d < bd || (d == bd && i < bi); }

// (d, id) minimum over the workgroup, lexicographic; valid in thread 0
__device__ __forceinline__ void pick_reduce(double& d, int& i) {
  for (int o = 32; o >= 1; o >>= 1) {
    const double od = __shfl_xor(d, o);
    const int oi = __shfl_xor(i, o);
    if (closer(od, oi, d, i)) { d = od; i = oi; }
  }
  __shared__ double sd[kB / 64];
  __shared__ int si[kB / 64];
  if ((threadIdx.x & 63) == 0) { sd[threadIdx.x >> 6] = d; si[threadIdx.x >> 6] = i; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kB / 64; w++)
      if (closer(sd[w], si[w], d, i)) { d = sd[w]; i = si[w]; }
}

}  // namespace fb
