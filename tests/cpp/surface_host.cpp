// PS::FEM::SurfaceMesh (include/fembrain/SurfaceMesh.h) over a Deformable: counts, faceAt, vertexAt and normalAt after steps and after
// Deformable::cut.  Prints the arrays and the mesh and state they belong to; tests/test_cpp_surface.py compares them with the
// restatement (tests/surfref.py).
#include <cstdio>
#include <utility>
#include <vector>

#include "fembrain/SurfaceMesh.h"

using PS::FEM::Deformable;
using PS::FEM::SurfaceMesh;
using PS::FEM::U32;
using PS::FEM::vec3d;

#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } \
  } while (0)

static std::vector<vec3d> plane(double x, double half) {
  const double c = 0.15;
  return {vec3d(x - 0.013 * half, c - half, c - half), vec3d(x + 0.007 * half, c - half, c + half), vec3d(x - 0.007 * half, c + half, c - half),
          vec3d(x + 0.013 * half, c + half, c + half)};
}

static int dump(const char* tag, Deformable& d) {
  SurfaceMesh* s = d.surfaceMesh();
  s->applyDisplacements();
  fb_fem_t h = d.getIntegrator()->handle();
  std::vector<double> rest((size_t)3 * fb_fem_num_nodes(h)), q(rest.size());
  std::vector<int> el((size_t)4 * fb_fem_num_tets(h));
  EXPECT(fb_fem_read_mesh(h, rest.data(), el.data()) == FB_OK);
  EXPECT(fb_fem_get_state(h, q.data(), nullptr, nullptr) == FB_OK);
  std::printf("%s_rest =", tag);
  for (double x : rest) std::printf(" %.17g", x);
  std::printf("\n%s_q =", tag);
  for (double x : q) std::printf(" %.17g", x);
  std::printf("\n%s_tets =", tag);
  for (int x : el) std::printf(" %d", x);
  std::printf("\n%s_faces =", tag);
  for (U32 f = 0; f < s->countFaceElements(); f++) std::printf(" %u %u %u", s->faceAt(f).x, s->faceAt(f).y, s->faceAt(f).z);
  std::printf("\n%s_compact =", tag);
  for (U32 f = 0; f < s->countFaceElements(); f++) std::printf(" %u %u %u", s->faceCompactAt(f).x, s->faceCompactAt(f).y, s->faceCompactAt(f).z);
  std::printf("\n%s_ids =", tag);
  for (U32 i = 0; i < s->countVertices(); i++) std::printf(" %u", s->vertexIdAt(i));
  std::printf("\n%s_xyz =", tag);
  for (U32 i = 0; i < s->countVertices(); i++) std::printf(" %.9g %.9g %.9g", s->vertexAt(i).x, s->vertexAt(i).y, s->vertexAt(i).z);
  std::printf("\n%s_normals =", tag);
  for (U32 i = 0; i < s->countVertices(); i++) std::printf(" %.9g %.9g %.9g", s->normalAt(i).x, s->normalAt(i).y, s->normalAt(i).z);
  std::printf("\n%s_box = %.9g %.9g %.9g %.9g %.9g %.9g\n", tag, s->aabbLower().x, s->aabbLower().y, s->aabbLower().z, s->aabbUpper().x, s->aabbUpper().y, s->aabbUpper().z);
  double dist = -1.0;
  vec3d p;
  const int far_node = s->findClosestVertex(vec3d(10.0, 0.15, 0.15), dist, p);
  std::printf("%s_closest = %d %.9g\n", tag, far_node, dist);
  return 0;
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
      for (int k = 0; k + 1 < nz; k++) {  // 6 tets around the cube diagonal (0 -> 7), in both orientations (every other one is left negative)
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
  Deformable d((int)(xyz.size() / 3), xyz.data(), (int)(tets.size() / 4), tets.data(), fixed);
  SurfaceMesh* s = d.surfaceMesh();
  EXPECT(s == d.surfaceMesh());
  const U32 faces0 = s->countFaceElements(), verts0 = s->countVertices();
  EXPECT(faces0 == 2 * 2 * ((nx - 1) * (ny - 1) + (nx - 1) * (nz - 1) + (ny - 1) * (nz - 1)));
  EXPECT(verts0 == (U32)(nx * ny * nz - (nx - 2) * (ny - 2) * (nz - 2)));
  for (int step = 0; step < 3; step++) d.timestep();
  if (dump("steps", d)) return 1;
  EXPECT(s->countFaceElements() == faces0);
  const std::vector<vec3d> seg = {vec3d(0.37, -1, 0), vec3d(0.37, 1, 0)};
  EXPECT(d.cut(seg, plane(0.35, 2.0), true) > 0);
  EXPECT(s->countFaceElements() > faces0 && s->countVertices() > verts0);  // the next access has re-read the topology
  for (int step = 0; step < 2; step++) d.timestep();
  if (dump("cut", d)) return 1;
  std::printf("surface_host = ok\n");
  return 0;
}
