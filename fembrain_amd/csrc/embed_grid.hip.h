// What the units that search through a grid (embed.hip, embed_closest.hip, face_search.hip.h) all evaluate, each written once: the search grid
// as a kernel sees it with its cell function, an element's vertices, its centre, the distance of a point from a centre, the weights of a point
// in an element, and the slab of a cell as the ring searches widen it.  The units are built with
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


// determinant of the rows a, b, c (mat3d.h det: the six products in its order)
__device__ __forceinline__ double det3(const double* a, const double* b, const double* c) {
  return (-a[2] * b[1] * c[0] + a[1] * b[2] * c[0] + a[2] * b[0] * c[1] - a[0] * b[2] * c[1] - a[1] * b[0] * c[2] + a[0] * b[1] * c[2]);
}
// determinant of [a 1; b 1; c 1; d 1] (TetMesh::getTetDeterminant)
__device__ __forceinline__ double tet_det(const double* a, const double* b, const double* c, const double* d) {
  return (-det3(b, c, d) + det3(a, c, d) - det3(a, b, d) + det3(a, b, c));
}
// the four weights of p in the element v; true when all are >= 0 (a flat element has none: NaN or infinite weights compare false)
__device__ __forceinline__ bool bary(const double (*v)[3], const double* p, double* w) {
  const double d0 = tet_det(v[0], v[1], v[2], v[3]);
  w[0] = tet_det(p, v[1], v[2], v[3]) / d0;
  w[1] = tet_det(v[0], p, v[2], v[3]) / d0;
  w[2] = tet_det(v[0], v[1], p, v[3]) / d0;
  w[3] = tet_det(v[0], v[1], v[2], p) / d0;
  return w[0] >= 0 && w[1] >= 0 && w[2] >= 0 && w[3] >= 0;
}

// ---- the search through a grid of points (embed_closest.hip, face_search.hip.h) ----
constexpr double kRingGrow = 1.0 + 0x1p-40;  // what a distance, its square and a root are widened by: far above their roundings

// the gap between x and the slab of cell j on axis k, widened by 2^-10 of a cell and open outward at both ends of the axis
__device__ __forceinline__ double slab_gap(const GridDev& g, int k, int j, double h, double x) {
  const double s = h * 0x1p-10;
  const double below = j > 0 ? (g.lo[k] + j * h - s) - x : 0.0, above = j < g.dim[k] - 1 ? x - (g.lo[k] + (j + 1) * h + s) : 0.0;
  return fmax(0.0, fmax(below, above));
}

}  // namespace fb
