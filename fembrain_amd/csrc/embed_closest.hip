// The closest centre for the points no element contains, through a grid of the centres (embed.h, EmbedCentreGrid), hand-written for gfx950.
//
// The rule is embed.hip's: the least centre_distance, of equal distances the lowest element, a distance that is not below DBL_MAX never
// wins, element 0 where none does.  k_closest tests every centre of the mesh for every point; here a point looks at the centres of the
// cells that could hold a closer one and at no others, and the answer is the same bits: tet_centre and centre_distance (embed_grid.hip.h)
// are the scan's, on the same operands.
//
// The centre grid: a thread per element forms its centre and the key of its cell in the element grid's box and dim[3] (clamped per axis,
// so every centre has a cell) and counts it into its cell (an integer atomic: any order); one stable sort by cell, so elements ascend
// inside a cell; an exclusive scan of the counts gives cell_start[cells + 1], and because x runs fastest in the key a run of cells along
// x is ONE range of the sorted arrays; a last pass stores the centres in sorted order, 24 bytes each.  No host wait: every size is known.
//
// The search, one wavefront per point, lanes striding over a row's centres (k_ring):
//  1. Shells of cells around the point's cell (the point clamped into the grid on each axis) until one holds a centre, then one more:
//     a candidate (best_d, best_e).
//  2. Every cell the box [p - D, p + D] overlaps, D = best_d (1 + 2^-40), widened by one cell on every side, row by row; per row (y, z)
//     the x-range that is left of D after the row's distance in y and z.  best_d tightens as it goes.
// Why no centre outside the visited cells can have a distance <= best_d:
//  - Let c be a centre whose COMPUTED distance d(p, c) is <= best_d.  centre_distance makes nine roundings, so the exact distance is at
//    most d (1 + 2^-50) < D, and so is each of |c_x - p_x|, |c_y - p_y|, |c_z - p_z|.
//  - cell_clamped is monotone (a subtraction, a product with a positive number, a truncation and two clamps, each monotone), so from
//    c_k >= p_k - D follows cell(c_k) >= cell(p_k - D) wherever p_k - D is formed exactly.  It is formed with one rounding, relative to
//    the RESULT: where the result lies in the box that is 2^-53 of a coordinate of the box, which embed_ring_covers has checked to be
//    below 2^-13 of a cell; where it lies outside the clamp decides.  A whole cell on either side covers that.
//  - A centre whose computed cell on the axis y is j has lo + j h - s <= c_y <= lo + (j + 1) h + s with s = h 2^-10: the cell
//    coordinate (c_y - lo) inv carries three roundings of at most 2^-53 each on a value of at most 1024, that is 2^-41 cells, and
//    the edges lo + j h as formed here a rounding of the coordinate, below 2^-12 of a cell (embed_ring_covers); the first and the last
//    cell of an axis are taken as unbounded outward, so the clamps need no argument.  The gap g_y between p_y and that widened slab is
//    therefore at most |c_y - p_y|, g_z likewise, and (c_x - p_x)^2 <= D^2 - g_y^2 - g_z^2: a row with g_y^2 + g_z^2 > D^2 (1 + 2^-40)
//    holds no such centre, and in any other row c lies in the x-range of the root of the difference, by the argument above.
//  - Tightening best_d only removes centres that could no longer win under (d, e): a centre with d == best_d and a lower element is
//    still inside, because every comparison above is <=.
// Every loop is bounded by numbers the host knows: shells by the largest dim, rows by dim[1] dim[2], a row by n_tets; and a point that
// has tested more than `budget` centres stops, is flagged, and goes with the other far points to k_closest / k_closest_final unchanged.
// No floating-point atomics, no spinning; the counters leave through per-workgroup partials and one fold, nothing to reset.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include "device_prims.hip.h"
#include "embed.h"
#include "embed_grid.hip.h"
#include "launch.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

// the centre grid as the search sees it
struct CentreDev {
  int n;  // centres
  const int* cell_start;
  const double* centre;
  const int* elem;
};

__device__ __forceinline__ int centre_cell(const GridDev& g, const double* c) {
  return (cell_clamped(g, 2, c[2]) * g.dim[1] + cell_clamped(g, 1, c[1])) * g.dim[0] + cell_clamped(g, 0, c[0]);
}

// A thread per element: (cell of its centre, element), and the cell's count
__global__ __launch_bounds__(kB) void k_centre_keys(int n_tets, GridDev g, const int4* __restrict__ tets, const double* __restrict__ x0, uint32_t* __restrict__ keys,
                                                    uint32_t* __restrict__ vals, int* __restrict__ cnt) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  double v[4][3], c[3];
  load_tet(tets, x0, e, v);
  tet_centre(v, c);
  const int cell = centre_cell(g, c);  // in [0, cells): each factor is clamped
  keys[e] = (uint32_t)cell;
  vals[e] = (uint32_t)e;
  atomicAdd(cnt + cell, 1);
}

// A thread per sorted entry: its centre, formed again from the element (the same function: the same bits)
__global__ __launch_bounds__(kB) void k_centre_store(int n_tets, const int* __restrict__ elem, const int4* __restrict__ tets, const double* __restrict__ x0,
                                                     double* __restrict__ centre) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_tets) return;
  int e = elem[j];
  if (e < 0 || e >= n_tets) e = 0;
  double v[4][3], c[3];
  load_tet(tets, x0, e, v);
  tet_centre(v, c);
  centre[3 * (size_t)j] = c[0]; centre[3 * (size_t)j + 1] = c[1]; centre[3 * (size_t)j + 2] = c[2];
}

// (kRingGrow and slab_gap: embed_grid.hip.h)

// One wavefront per point without a containing element (ext_ids[t]).  Everything that decides a branch is the same in every lane: the
// ranges come from cell_start, the best pair is folded over the wavefront whenever a lane has improved it.
__global__ __launch_bounds__(kB) void k_ring(int n_ext, const int* __restrict__ ext_ids, int n, const double* __restrict__ loc, GridDev g, CentreDev cg, long long budget,
                                             int* __restrict__ elem, unsigned char* __restrict__ far_flag, long long* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = blockIdx.x * kWaves + wave;
  int i = t < n_ext ? ext_ids[t] : -1;
  if (i >= n) i = -1;
  long long tested = 0;
  bool far = false;
  if (i >= 0) {
    const double p[3] = {loc[3 * (size_t)i], loc[3 * (size_t)i + 1], loc[3 * (size_t)i + 2]};
    double bd = DBL_MAX;
    int be = INT_MAX;
    // the centres of the cells x0c .. x1c of the row that begins at cell `row`: one range
    auto scan_cells = [&](int row, int x0c, int x1c) {
      const int j0 = max(cg.cell_start[row + x0c], 0), j1 = min(cg.cell_start[row + x1c + 1], cg.n);
      bool improved = false;
      for (int j = j0 + lane; j < j1; j += 64) {
        const double c[3] = {cg.centre[3 * (size_t)j], cg.centre[3 * (size_t)j + 1], cg.centre[3 * (size_t)j + 2]};
        const int e = cg.elem[j];
        const double d = centre_distance(p, c);
        if (d < DBL_MAX && Lowest()(d, e, bd, be)) { bd = d; be = e; improved = true; }
      }
      if (__any(improved)) wf_best<int, Lowest>(bd, be);
      if (j1 > j0) tested += j1 - j0;
      if (tested > budget) far = true;
      return j1 > j0;
    };
    int pc[3], rmax = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      pc[k] = cell_clamped(g, k, p[k]);
      rmax = max(rmax, max(pc[k], g.dim[k] - 1 - pc[k]));
    }
    // 1. shells until one holds a centre, and the one after it
    int stop = -1;
    for (int r = 0; r <= rmax && !far; r++) {
      bool got = false;
      const int z1 = min(pc[2] + r, g.dim[2] - 1), y1 = min(pc[1] + r, g.dim[1] - 1), xa = pc[0] - r, xb = pc[0] + r;
      for (int z = max(pc[2] - r, 0); z <= z1 && !far; z++)
        for (int y = max(pc[1] - r, 0); y <= y1 && !far; y++) {
          const int row = (z * g.dim[1] + y) * g.dim[0];
          if (z == pc[2] - r || z == pc[2] + r || y == pc[1] - r || y == pc[1] + r) {  // a row of the shell's faces: all of it
            got |= scan_cells(row, max(xa, 0), min(xb, g.dim[0] - 1));
          } else {  // its two ends
            if (xa >= 0) got |= scan_cells(row, xa, xa);
            if (xb < g.dim[0] && !far) got |= scan_cells(row, xb, xb);
          }
        }
      if (got && stop < 0) stop = r + 1;
      if (r == stop) break;
    }
    // 2. every cell that could hold a centre at a distance <= best_d
    if (!far) {
      const bool none = !(bd < DBL_MAX);  // (no centre below DBL_MAX so far: the whole grid)
      const double D0 = bd * kRingGrow;
      const double h[3] = {1.0 / g.inv[0], 1.0 / g.inv[1], 1.0 / g.inv[2]};
      const int z0 = none ? 0 : max(cell_clamped(g, 2, p[2] - D0) - 1, 0), z1 = none ? g.dim[2] - 1 : min(cell_clamped(g, 2, p[2] + D0) + 1, g.dim[2] - 1);
      const int y0 = none ? 0 : max(cell_clamped(g, 1, p[1] - D0) - 1, 0), y1 = none ? g.dim[1] - 1 : min(cell_clamped(g, 1, p[1] + D0) + 1, g.dim[1] - 1);
      for (int z = z0; z <= z1 && !far; z++) {
        const double gz = slab_gap(g, 2, z, h[2], p[2]);
        int ya = y0, yb = y1;  // the rows of this layer that are left of D after its distance in z: the x-range's argument with g_y = 0
        {
          const double D = bd * kRingGrow, D2 = D * D * kRingGrow;
          if (D2 < DBL_MAX) {
            if (gz * gz > D2) continue;
            const double rem = sqrt(D2 - gz * gz) * kRingGrow;
            ya = max(y0, cell_clamped(g, 1, p[1] - rem) - 1);
            yb = min(y1, cell_clamped(g, 1, p[1] + rem) + 1);
          }
        }
        for (int y = ya; y <= yb && !far; y++) {
          int xa = 0, xb = g.dim[0] - 1;
          const double D = bd * kRingGrow, D2 = D * D * kRingGrow;
          if (D2 < DBL_MAX) {  // (else the square is out of range: the whole row)
            const double gy = slab_gap(g, 1, y, h[1], p[1]);
            const double g2 = gy * gy + gz * gz;
            if (g2 > D2) continue;
            const double rem = sqrt(D2 - g2) * kRingGrow;
            xa = max(cell_clamped(g, 0, p[0] - rem) - 1, 0);
            xb = min(cell_clamped(g, 0, p[0] + rem) + 1, g.dim[0] - 1);
          }
          scan_cells((z * g.dim[1] + y) * g.dim[0], xa, xb);
        }
      }
    }
    if (lane == 0) {
      far_flag[t] = far ? 1 : 0;
      if (!far) elem[i] = be == INT_MAX ? 0 : be;
    }
  } else if (t < n_ext && lane == 0) {
    far_flag[t] = 0;
  }
  // the workgroup's counters: far points | centres tested | the most of one point
  __shared__ long long sh[kWaves][3];
  if (lane == 0) { sh[wave][0] = far ? 1 : 0; sh[wave][1] = tested; sh[wave][2] = tested; }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long a = 0, b = 0, c = 0;
    for (int w = 0; w < kWaves; w++) { a += sh[w][0]; b += sh[w][1]; c = max(c, sh[w][2]); }
    part[3 * (size_t)blockIdx.x] = a; part[3 * (size_t)blockIdx.x + 1] = b; part[3 * (size_t)blockIdx.x + 2] = c;
  }
}

// one workgroup: the partials folded (integer sums and a maximum: any order)
__global__ __launch_bounds__(kB) void k_ring_fold(int n_part, const long long* __restrict__ part, long long* __restrict__ out3) {
  long long a = 0, b = 0, c = 0;
  for (int k = threadIdx.x; k < n_part; k += kB) { a += part[3 * (size_t)k]; b += part[3 * (size_t)k + 1]; c = max(c, part[3 * (size_t)k + 2]); }
  __shared__ long long sh[kB][3];
  sh[threadIdx.x][0] = a; sh[threadIdx.x][1] = b; sh[threadIdx.x][2] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kB; k++) { a += sh[k][0]; b += sh[k][1]; c = max(c, sh[k][2]); }
    out3[0] = a; out3[1] = b; out3[2] = c;
  }
}

}  // namespace

bool embed_ring_covers(const EmbedGrid& G) {
  for (int k = 0; k < 3; k++) {
    const double cell = (G.hi[k] - G.lo[k]) / G.dim[k];
    if (!(std::ldexp(std::max(std::fabs(G.lo[k]), std::fabs(G.hi[k])), -40) <= cell)) return false;
  }
  return true;
}

int embed_centre_grid_build(hipStream_t s, EmbedWork& EW, const EmbedMesh& M, PlanWorkspace& W) {
  const EmbedGrid& G = EW.grid;
  EmbedCentreGrid& C = EW.cgrid;
  C.valid = false;
  if (!G.valid) return fail(FB_EDEVICE, "embedding: no search grid under the centre grid");
  const size_t n = (size_t)M.n_tets, n_cells = (size_t)G.dim[0] * G.dim[1] * G.dim[2];
  FB_TRY(C.cell_cnt.alloc(n_cells + 1)); FB_TRY(C.cell_start.alloc(n_cells + 1)); FB_TRY(C.centre.alloc(3 * n)); FB_TRY(C.elem.alloc(n));
  FB_TRY(C.cell_cnt.zero(s));
  // (the sort's arrays are the plan builder's, as in embed_grid_build)
  FB_TRY(W.keys.reserve((n + 1) / 2)); FB_TRY(W.keys_s.reserve((n + 1) / 2)); FB_TRY(W.vals.reserve(n));
  uint32_t* ck = reinterpret_cast<uint32_t*>(W.keys.p);
  uint32_t* ck_s = reinterpret_cast<uint32_t*>(W.keys_s.p);
  FB_TRY(launch_1d(k_centre_keys, M.n_tets, s, M.n_tets, grid_dev(G), M.tets, M.x0, ck, W.vals.p, C.cell_cnt.p));
  FB_TRY(sort_pairs(W.temp, s, ck, ck_s, W.vals.p, reinterpret_cast<uint32_t*>(C.elem.p), n, (unsigned)bits_of((long long)n_cells)));
  FB_TRY(exclusive_scan(W.temp, s, C.cell_cnt.p, C.cell_start.p, 0, n_cells + 1));
  FB_TRY(launch_1d(k_centre_store, M.n_tets, s, M.n_tets, C.elem.p, M.tets, M.x0, C.centre.p));
  C.valid = true;
  C.n_builds++;
  return FB_OK;
}

int embed_closest_ring(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, PlanWorkspace& W, int n_ext, long long budget, int* n_far) {
  if (!EW.cgrid.valid) FB_TRY(embed_centre_grid_build(s, EW, M, W));
  const EmbedCentreGrid& C = EW.cgrid;
  const int nblk = (int)wave_grid_for(n_ext).x;
  FB_TRY(EW.far_flag.reserve((size_t)n_ext)); FB_TRY(EW.far_ids.reserve((size_t)n_ext)); FB_TRY(EW.ring_part.reserve((size_t)3 * nblk + 4));
  long long* out = EW.ring_part.p + 3 * (size_t)nblk;
  const CentreDev cg = {M.n_tets, C.cell_start.p, C.centre.p, C.elem.p};
  FB_TRY(launch_waves(k_ring, n_ext, s, n_ext, EW.ext_ids.p, E.n_points, E.loc.p, grid_dev(EW.grid), cg, budget, E.elem.p, EW.far_flag.p, EW.ring_part.p));
  FB_TRY(launch_grid(k_ring_fold, dim3(1), s, nblk, EW.ring_part.p, out));
  FB_TRY(select_flagged(W.temp, s, EW.ext_ids.p, EW.far_flag.p, EW.far_ids.p, out + 3, (size_t)n_ext));
  long long r[4] = {0, 0, 0, 0};
  FB_TRY(EW.ring_part.download(r, 4, s, 3 * (size_t)nblk));  // the host wait
  if (r[0] < 0 || r[0] > n_ext || r[3] != r[0] || r[1] < 0 || r[2] < 0)
    return fail(FB_EDEVICE, "embedding: %lld far points (%lld listed) of %d out of range", r[0], r[3], n_ext);
  E.search.path = FB_EMBED_CLOSEST_RING;
  E.search.n_outside = n_ext;
  E.search.n_far = (int)r[0];
  E.search.tested = r[1];
  E.search.max_one = (int)std::min<long long>(r[2], INT_MAX);
  *n_far = (int)r[0];
  return FB_OK;
}

}  // namespace fb
