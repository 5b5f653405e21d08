// The per-element and per-node expressions that more than one mesh-side unit evaluates (surface, haptic, contact, parts, embed, embed_touch),
// each written once with its operand order: the units are built with -ffp-contract=off and promise the same bits wherever the same
// quantity is formed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hip.h"

namespace fb {

__device__ __forceinline__ int tet_node(const int4& t, int k) { return k == 0 ? t.x : k == 1 ? t.y : k == 2 ? t.z : t.w; }

__device__ __forceinline__ void sort3(unsigned& a, unsigned& b, unsigned& c) {
  unsigned t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
}

// |u . (v x w)| / 6 with u, v, w = p0 - p3, p1 - p3, p2 - p3 (Deformable::computeVolume)
__device__ __forceinline__ double tet_volume(const double p[4][3]) {
  const double u[3] = {p[0][0] - p[3][0], p[0][1] - p[3][1], p[0][2] - p[3][2]}, v[3] = {p[1][0] - p[3][0], p[1][1] - p[3][1], p[1][2] - p[3][2]},
               w[3] = {p[2][0] - p[3][0], p[2][1] - p[3][1], p[2][2] - p[3][2]};
  return fabs(u[0] * (v[1] * w[2] - v[2] * w[1]) + u[1] * (v[2] * w[0] - v[0] * w[2]) + u[2] * (v[0] * w[1] - v[1] * w[0])) / 6.0;
}

// Point i of a binding (four internal nodes, four weights): ((w0 p0 + w1 p1) + w2 p2) + w3 p3 in fp64 with p = x0 + q, or the rest
// positions where q is null.  A node outside [0, n_nodes) reads node 0.
__device__ __forceinline__ void embed_point(int i, int n_nodes, const int* __restrict__ vert_int, const double* __restrict__ w4, const double* __restrict__ x0,
                                            const double* __restrict__ q, double out[3]) {
  double pk[4][3], w[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int nd = vert_int[4 * (size_t)i + k];
    if (nd < 0 || nd >= n_nodes) nd = 0;
    const size_t b = 3 * (size_t)nd;
    w[k] = w4[4 * (size_t)i + k];
#pragma unroll
    for (int c = 0; c < 3; c++) pk[k][c] = q ? x0[b + c] + q[b + c] : x0[b + c];
  }
#pragma unroll
  for (int c = 0; c < 3; c++) out[c] = ((w[0] * pk[0][c] + w[1] * pk[1][c]) + w[2] * pk[2][c]) + w[3] * pk[3][c];
}

// caller id -> internal node -> x0 + q; *ok false (and p zero) for an id the map sends outside [0, n_nodes)
__device__ __forceinline__ void node_position(int i, const int* __restrict__ new_of_old, int n_nodes, const double* __restrict__ x0, const double* __restrict__ q, double p[3],
                                              bool* ok) {
  const int node = new_of_old ? new_of_old[i] : i;
  *ok = (unsigned)node < (unsigned)n_nodes;
  if (!*ok) { p[0] = p[1] = p[2] = 0.0; return; }
  const size_t b = 3 * (size_t)node;
  p[0] = x0[b] + q[b]; p[1] = x0[b + 1] + q[b + 1]; p[2] = x0[b + 2] + q[b + 2];
}

// inclusive on every side
__device__ __forceinline__ bool in_box(const double p[3], const double* lo, const double* hi) {
  return p[0] >= lo[0] && p[0] <= hi[0] && p[1] >= lo[1] && p[1] <= hi[1] && p[2] >= lo[2] && p[2] <= hi[2];
}

namespace {

// A thread per entry of a sorted key array: the first of a run of equal keys writes the run's start, the last its end (lo / hi zeroed
// before: an absent key has an empty run).  A key that is not below n_keys -- the tail that stands for "no such id" -- writes nothing.
// (A template, launched as k_run_bounds<>, so that only the units that launch it carry a copy of the kernel.)
template <class Count = long long>
__global__ __launch_bounds__(kB) void k_run_bounds(Count n, const uint32_t* __restrict__ keys_s, uint32_t n_keys, int* __restrict__ lo, int* __restrict__ hi) {
  const Count j = (Count)blockIdx.x * kB + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = keys_s[j];
  if (k >= n_keys) return;
  if (j == 0 || keys_s[j - 1] != k) lo[k] = (int)j;
  if (j + 1 == n || keys_s[j + 1] != k) hi[k] = (int)(j + 1);
}

}  // namespace
}  // namespace fb
