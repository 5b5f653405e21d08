// Deformable::cut (include/fembrain/Deformable.h) on a small cantilever: CuttableMesh::cut's return codes, and the host copy of the
// mesh (cells(), the rest positions) equal to what the handle holds after a cut.  Prints "cut_deformable ok" on success.
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "fembrain/Deformable.h"

using PS::FEM::Deformable;
using PS::FEM::vec3d;

#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } \
  } while (0)

// one quad about the plane x = const centred on the mid-section, slightly tilted so that it passes no node
static std::vector<vec3d> plane(double x, double half) {
  const double c = 0.15;
  return {vec3d(x - 0.013 * half, c - half, c - half), vec3d(x + 0.007 * half, c - half, c + half), vec3d(x - 0.007 * half, c + half, c - half),
          vec3d(x + 0.013 * half, c + half, c + half)};
}

int main() {
  const int nx = 8, ny = 4, nz = 4;
  const double h = 0.1;
  std::vector<double> xyz;
  for (int i = 0; i < nx; i++)
    for (int j = 0; j < ny; j++)
      for (int k = 0; k < nz; k++) { xyz.push_back(i * h); xyz.push_back(j * h); xyz.push_back(k * h); }
  auto id = [&](int i, int j, int k) { return (i * ny + j) * nz + k; };
  std::vector<int> tets;
  for (int i = 0; i + 1 < nx; i++)
    for (int j = 0; j + 1 < ny; j++)
      for (int k = 0; k + 1 < nz; k++) {  // 6 tets around the cube diagonal (0 -> 7)
        const int c[8] = {id(i, j, k), id(i + 1, j, k), id(i, j + 1, k), id(i + 1, j + 1, k), id(i, j, k + 1), id(i + 1, j, k + 1), id(i, j + 1, k + 1), id(i + 1, j + 1, k + 1)};
        const int t[6][4] = {{0, 1, 3, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 6, 4, 7}, {0, 4, 5, 7}, {0, 5, 1, 7}};
        for (int e = 0; e < 6; e++) {
          int v4[4] = {c[t[e][0]], c[t[e][1]], c[t[e][2]], c[t[e][3]]};
          double a[3][3];
          for (int r = 0; r < 3; r++)
            for (int q = 0; q < 3; q++) a[r][q] = xyz[3 * v4[r + 1] + q] - xyz[3 * v4[0] + q];
          const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
          if (det < 0) std::swap(v4[2], v4[3]);  // positively oriented
          tets.insert(tets.end(), v4, v4 + 4);
        }
      }
  std::vector<int> fixed;
  for (int j = 0; j < ny; j++)
    for (int k = 0; k < nz; k++) fixed.push_back(id(0, j, k));
  Deformable d((int)(xyz.size() / 3), xyz.data(), (int)(tets.size() / 4), tets.data(), fixed);
  // (at rest: the blade positions below are in the rest frame; the cut tests the current shape)
  const std::vector<vec3d> seg = {vec3d(0.37, -1, 0), vec3d(0.37, 1, 0)};
  const size_t cells0 = d.countCells();
  EXPECT(d.cut(seg, std::vector<vec3d>(3), true) == CUT_ERR_INVALID_INPUT_ARG);
  EXPECT(d.cut(std::vector<vec3d>(1), plane(0.35, 2.0), true) == CUT_ERR_INVALID_INPUT_ARG);
  EXPECT(d.cut(seg, plane(5.0, 0.1), true) == 0);                            // nowhere near the mesh
  EXPECT(d.cut(seg, plane(0.35, 0.07), true) == CUT_ERR_UNHANDLED_CUT_STATE);  // stops inside the mesh
  EXPECT(d.cut(seg, plane(0.35, 2.0), false) == CUT_ERR_USER_CANCELLED_CUT);
  EXPECT(d.countCells() == cells0);
  const int n = d.cut(seg, plane(0.35, 2.0), true);
  EXPECT(n > 0);
  EXPECT(d.countCells() > cells0);
  fb_fem_t hd = d.getIntegrator()->handle();
  std::vector<double> rest((size_t)3 * fb_fem_num_nodes(hd));
  std::vector<int> el((size_t)4 * fb_fem_num_tets(hd));
  EXPECT(fb_fem_read_mesh(hd, rest.data(), el.data()) == FB_OK);
  EXPECT(el == d.cells());
  EXPECT(d.countNodes() * 3 == rest.size());
  d.timestep();
  std::printf("cut_deformable ok: %d cells subdivided, %u cells, %u nodes\n", n, d.countCells(), d.countNodes());
  return 0;
}
