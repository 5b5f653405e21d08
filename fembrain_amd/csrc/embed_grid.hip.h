// What the two units of the embedding search (embed.hip, embed_closest.hip) both evaluate, each written once: the search grid as a kernel
// sees it with its cell function, an element's vertices, its centre and the distance of a point from a centre.  The units are built with
// -ffp-contract=off, so one function is one sequence of roundings wherever it is called: the closest centre of the full scan and of the
// search through the centre grid are compared on the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "embed.h"
#include "mesh_device.hip.h"

namespace fb {

// the search grid as the kernels see it
struct GridDev {
  double lo[3], hi[3], inv[3], pad;
  int dim[3];
  int n_wide;
  const int *cell_lo, *cell_hi, *cell_elem, *wide;
};

inline GridDev grid_dev(const EmbedGrid& G) {
  GridDev g;
  for (int k = 0; k < 3; k++) { g.lo[k] = G.lo[k]; g.hi[k] = G.hi[k]; g.inv[k] = G.inv[k]; g.dim[k] = G.dim[k]; }
  g.pad = G.pad;
  g.n_wide = G.n_wide;
  g.cell_lo = G.cell_lo.p; g.cell_hi = G.cell_hi.p; g.cell_elem = G.cell_elem.p; g.wide = G.wide.p;
  return g;
}

// the cell of a coordinate that is not below the grid's lower bound; the caller has decided that already
__device__ __forceinline__ int cell_of(const GridDev& g, int k, double x) {
  const double c = (x - g.lo[k]) * g.inv[k];
  return c >= (double)(g.dim[k] - 1) ? g.dim[k] - 1 : (int)c;
}
// ... of any coordinate, clamped into the grid: decided on the coordinate, before any index is formed.  Monotone in x: the subtraction,
// the product with a positive number and the truncation each are.
__device__ __forceinline__ int cell_clamped(const GridDev& g, int k, double x) { return x >= g.lo[k] ? cell_of(g, k, x) : 0; }

__device__ __forceinline__ void load_tet(const int4* __restrict__ tets, const double* __restrict__ x0, int e, double (*v)[3]) {
  const int4 t = tets[e];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double* p = x0 + 3 * (size_t)tet_node(t, k);
    v[k][0] = p[0]; v[k][1] = p[1]; v[k][2] = p[2];
  }
}

// the centre of an element: the mean of the four vertices, summed in order and scaled by 1.0 / 4
__device__ __forceinline__ void tet_centre(const double (*v)[3], double* c) {
#pragma unroll
  for (int k = 0; k < 3; k++) c[k] = (((v[0][k] + v[1][k]) + v[2][k]) + v[3][k]) * (1.0 / 4);
}
// the distance of the point p from the centre c
__device__ __forceinline__ double centre_distance(const double* p, const double* c) {
  const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}

}  // namespace fb
