// The launch shape of the mesh-side host drivers (plan_device, delta, renumber, subdivide, surface, haptic, contact, stress, parts, embed):
// workgroups of kB threads, no dynamic LDS, a grid that covers n work items, and the error check that belongs to every launch.
#pragma once
#include "common.h"

namespace fb {

constexpr int kB = 256;

// workgroups for a thread per item; never an empty grid (n == 0 runs one idle workgroup)
inline dim3 grid_for(long long n) { return dim3((unsigned)std::max<long long>(1, (n + kB - 1) / kB)); }
inline int blocks_for(long long n) { return (int)grid_for(n).x; }  // (the number of per-workgroup partials such a launch leaves)
// ... for a wavefront per item (one 64-row slice, one slot)
inline dim3 wave_grid_for(long long n) { return dim3((unsigned)std::max<long long>(1, (n + kB / 64 - 1) / (kB / 64))); }

// bits that hold every id in [0, n), at least one
inline int bits_of(long long n) {
  int b = 1;
  while ((1LL << b) < n) b++;
  return b;
}

// The kernel's own parameter types convert the arguments (nullptr, int -> long long, pointer -> pointer to const), as a direct launch would.
template <class... P, class... A>
int launch_shape(void (*k)(P...), dim3 grid, dim3 block, hipStream_t s, A... a) {
  hipLaunchKernelGGL(k, grid, block, 0, s, static_cast<P>(a)...);
  FB_HIP(hipGetLastError());
  return FB_OK;
}
template <class... P, class... A>
int launch_grid(void (*k)(P...), dim3 grid, hipStream_t s, A... a) {
  return launch_shape(k, grid, dim3(kB), s, a...);
}
template <class... P, class... A>
int launch_1d(void (*k)(P...), long long n, hipStream_t s, A... a) {
  return launch_grid(k, grid_for(n), s, a...);
}
template <class... P, class... A>
int launch_waves(void (*k)(P...), long long n, hipStream_t s, A... a) {
  return launch_grid(k, wave_grid_for(n), s, a...);
}

}  // namespace fb
