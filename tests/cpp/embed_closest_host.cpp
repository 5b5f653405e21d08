// PS::FEM::EmbeddedMesh::searchInfo (include/fembrain/EmbeddedMesh.h) from a C++ host program: a closed surface drawn around a small beam,
// every vertex outside the tets, bound through the centre grid.  Prints the counts and the search info; tests/test_cpp_embed_closest.py
// reads them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "fembrain/EmbeddedMesh.h"

using PS::FEM::Deformable;
using PS::FEM::EmbeddedMesh;
using PS::FEM::U32;

#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } \
  } while (0)

int main() {
  // (384 points on 1,056 tets: the automatic rule would scan, and the default budget is for meshes where a scan costs something)
  setenv("FEMBRAIN_EMBED_CLOSEST", "ring", 1);
  setenv("FEMBRAIN_EMBED_RING_BUDGET", "1000000", 1);
  const int nx = 12, ny = 5, nz = 5;
  const double h = 0.1;
  std::vector<double> xyz;
  for (int i = 0; i < nx; i++)
    for (int j = 0; j < ny; j++)
      for (int k = 0; k < nz; k++) { xyz.push_back(i * h); xyz.push_back(j * h); xyz.push_back(k * h); }
  auto id = [&](int i, int j, int k) { return (i * ny + j) * nz + k; };
  std::vector<int> tets;
  for (int i = 0; i + 1 < nx; i++)
    for (int j = 0; j + 1 < ny; j++)
      for (int k = 0; k + 1 < nz; k++) {  // 6 tets around the cube diagonal (0 -> 7), as tests/cpp/embed_host.cpp makes them
        const int c[8] = {id(i, j, k), id(i + 1, j, k), id(i, j + 1, k), id(i + 1, j + 1, k), id(i, j, k + 1), id(i + 1, j, k + 1), id(i, j + 1, k + 1), id(i + 1, j + 1, k + 1)};
        const int t[6][4] = {{0, 1, 3, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 6, 4, 7}, {0, 4, 5, 7}, {0, 5, 1, 7}};
        for (int e = 0; e < 6; e++) {
          int v4[4] = {c[t[e][0]], c[t[e][1]], c[t[e][2]], c[t[e][3]]};
          if (e & 1) std::swap(v4[2], v4[3]);
          tets.insert(tets.end(), v4, v4 + 4);
        }
      }
  std::vector<int> fixed;
  for (int j = 0; j < ny; j++)
    for (int k = 0; k < nz; k++) fixed.push_back(id(0, j, k));
  // the drawn mesh: 24 x 16 points of an ellipsoid through the corners of the beam's box and 5 % more, and the triangles between them
  const int mu = 24, mv = 16;
  const double pi = 3.14159265358979323846, half[3] = {0.5 * (nx - 1) * h, 0.5 * (ny - 1) * h, 0.5 * (nz - 1) * h}, grow = 1.05 * std::sqrt(3.0);
  std::vector<double> pts;
  std::vector<int> tri;
  for (int a = 0; a < mu; a++)
    for (int b = 0; b < mv; b++) {
      const double phi = 2.0 * pi * (a + 0.37) / mu, th = pi * (b + 0.5) / mv;
      const double u[3] = {std::sin(th) * std::cos(phi), std::sin(th) * std::sin(phi), std::cos(th)};
      for (int k = 0; k < 3; k++) pts.push_back(half[k] + grow * half[k] * u[k]);
    }
  for (int a = 0; a < mu; a++)
    for (int b = 0; b + 1 < mv; b++) {
      const int a1 = (a + 1) % mu, p0 = a * mv + b, p1 = a1 * mv + b, p2 = a * mv + b + 1, p3 = a1 * mv + b + 1;
      const int two[6] = {p0, p1, p2, p1, p3, p2};
      tri.insert(tri.end(), two, two + 6);
    }
  Deformable d((int)(xyz.size() / 3), xyz.data(), (int)(tets.size() / 4), tets.data(), fixed);
  EmbeddedMesh* m = d.embed(pts, tri);
  EXPECT(m->countVertices() == (U32)(mu * mv) && m->countExternal() == (U32)(mu * mv));
  const fb_fem_embed_search_info si = m->searchInfo();
  EXPECT(si.path == FB_EMBED_CLOSEST_RING && si.n_outside == mu * mv && si.centre_grid_builds == 1);
  EXPECT(si.centres_tested > 0 && si.max_centres_one_point > 0 && si.n_far == 0);
  for (int step = 0; step < 2; step++) d.timestep();
  m->applyDisplacements();
  std::printf("n_tets = %d\nn_points = %u\nn_external = %u\n", (int)(tets.size() / 4), m->countVertices(), m->countExternal());
  std::printf("search = %d %d %d %d %d %lld\n", si.path, si.n_outside, si.n_far, si.centre_grid_builds, si.max_centres_one_point, si.centres_tested);
  std::printf("embed_closest_host = ok\n");
  return 0;
}
