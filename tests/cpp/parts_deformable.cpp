// Deformable::countDisjointParts / getDisjointParts / splitParts / readPart (include/fembrain/Deformable.h) on a small cantilever: one
// part before the cut, two after it, the reference's grouping, the cut opened by splitParts and the free part as a mesh of its own.
// Prints "parts_deformable ok" on success.
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "fembrain/Deformable.h"

using PS::FEM::Deformable;
using PS::FEM::U32;
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
  EXPECT(d.countDisjointParts() == 1);
  const std::vector<vec3d> seg = {vec3d(0.37, -1, 0), vec3d(0.37, 1, 0)};
  const std::vector<vec3d> quad = plane(0.35, 2.0);
  EXPECT(d.cut(seg, quad, true) > 0);
  EXPECT(d.countDisjointParts() == 2);
  std::vector<std::vector<U32> > groups;
  EXPECT(d.getDisjointParts(groups) == 2 && groups.size() == 2);
  EXPECT(groups[0].size() + groups[1].size() == d.countCells());
  EXPECT(groups[0][0] == 0);  // the part of cell 0 comes first
  for (size_t g = 0; g < 2; g++)
    for (size_t i = 1; i < groups[g].size(); i++) EXPECT(groups[g][i] > groups[g][i - 1]);
  // every cell of a part lies on one side of the cut
  const std::vector<int>& cells = d.cells();
  std::vector<double> rest0((size_t)3 * d.countNodes());
  std::vector<int> el0;
  d.getIntegrator()->ReadMesh(rest0, el0);
  for (size_t g = 0; g < 2; g++) {
    int right = 0;
    for (size_t i = 0; i < groups[g].size(); i++) {
      double cx = 0;
      for (int k = 0; k < 4; k++) cx += rest0[3 * (size_t)cells[4 * (size_t)groups[g][i] + k]];
      right += cx * 0.25 > 0.35;
    }
    EXPECT(right == 0 || right == (int)groups[g].size());
  }
  // the cut opens: the span of the mesh along x grows by twice the distance (the quad's normal is close to the x axis)
  EXPECT(d.splitParts(quad.data(), 0.05));
  std::vector<double> rest1;
  d.getIntegrator()->ReadMesh(rest1, el0);
  double lo0 = 1e300, hi0 = -1e300, lo1 = 1e300, hi1 = -1e300;
  for (size_t n = 0; n < rest0.size(); n += 3) {
    lo0 = std::min(lo0, rest0[n]); hi0 = std::max(hi0, rest0[n]);
    lo1 = std::min(lo1, rest1[n]); hi1 = std::max(hi1, rest1[n]);
  }
  EXPECT(std::fabs((hi1 - lo1) - (hi0 - lo0)) > 0.099 && std::fabs((hi1 - lo1) - (hi0 - lo0)) < 0.1001);
  EXPECT(d.countDisjointParts() == 2);
  // the free part (the one without cell 0: cell 0 sits at the clamp) as a mesh of its own
  std::vector<double> pxyz;
  std::vector<U32> pcells;
  d.readPart(1, pxyz, pcells);
  EXPECT(pcells.size() == 4 * groups[1].size());
  EXPECT(pcells[0] == 0 && pcells[1] == 1 && pcells[2] == 2 && pcells[3] == 3);  // nodes in order of first use
  U32 top = 0;
  for (size_t i = 0; i < pcells.size(); i++) top = std::max(top, pcells[i]);
  EXPECT(3 * ((size_t)top + 1) == pxyz.size());
  for (int k = 0; k < 4; k++)
    for (int a = 0; a < 3; a++) EXPECT(pxyz[3 * (size_t)k + a] == rest1[3 * (size_t)cells[4 * (size_t)groups[1][0] + k] + a]);
  bool threw = false;
  try { d.readPart(2, pxyz, pcells); } catch (const std::exception&) { threw = true; }
  EXPECT(threw);
  std::vector<int> pc(pcells.begin(), pcells.end());
  Deformable piece((int)(pxyz.size() / 3), pxyz.data(), (int)(pc.size() / 4), pc.data(), std::vector<int>());
  EXPECT(piece.countDisjointParts() == 1);
  d.timestep();
  piece.timestep();
  std::printf("parts_deformable ok: parts of %zu and %zu cells, the free part has %zu nodes\n", groups[0].size(), groups[1].size(), pxyz.size() / 3);
  return 0;
}
