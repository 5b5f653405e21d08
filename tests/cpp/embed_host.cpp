// PS::FEM::EmbeddedMesh (include/fembrain/EmbeddedMesh.h) through Deformable::embed and directly over a HipIntegrator: counts, vertexAt and
// normalAt after steps and after Deformable::cut.  Prints the arrays and the mesh and state they belong to; tests/test_cpp_embed.py
// compares them with the restatement (tests/embedref.py).
#include <cstdio>
#include <utility>
#include <vector>

#include "fembrain/EmbeddedMesh.h"

using PS::FEM::Deformable;
using PS::FEM::EmbeddedMesh;
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

static int dump(const char* tag, Deformable& d, EmbeddedMesh& m) {
  m.applyDisplacements();
  fb_fem_t h = d.getIntegrator()->handle();
  std::vector<double> rest((size_t)3 * fb_fem_num_nodes(h)), q(rest.size()), w, loc;
  std::vector<int> el((size_t)4 * fb_fem_num_tets(h)), be, bv;
  EXPECT(fb_fem_read_mesh(h, rest.data(), el.data()) == FB_OK);
  EXPECT(fb_fem_get_state(h, q.data(), nullptr, nullptr) == FB_OK);
  m.readBinding(be, bv, w, loc);
  std::printf("%s_rest =", tag);
  for (double x : rest) std::printf(" %.17g", x);
  std::printf("\n%s_q =", tag);
  for (double x : q) std::printf(" %.17g", x);
  std::printf("\n%s_tets =", tag);
  for (int x : el) std::printf(" %d", x);
  std::printf("\n%s_elements =", tag);
  for (int x : be) std::printf(" %d", x);
  std::printf("\n%s_vertices =", tag);
  for (int x : bv) std::printf(" %d", x);
  std::printf("\n%s_weights =", tag);
  for (double x : w) std::printf(" %.17g", x);
  std::printf("\n%s_loc =", tag);
  for (double x : loc) std::printf(" %.17g", x);
  std::printf("\n%s_xyz =", tag);
  for (U32 i = 0; i < m.countVertices(); i++) std::printf(" %.9g %.9g %.9g", m.vertexAt(i).x, m.vertexAt(i).y, m.vertexAt(i).z);
  std::printf("\n%s_normals =", tag);
  for (U32 i = 0; i < m.countVertices(); i++) std::printf(" %.9g %.9g %.9g", m.normalAt(i).x, m.normalAt(i).y, m.normalAt(i).z);
  std::printf("\n%s_box = %.9g %.9g %.9g %.9g %.9g %.9g\n", tag, m.aabbLower().x, m.aabbLower().y, m.aabbLower().z, m.aabbUpper().x, m.aabbUpper().y, m.aabbUpper().z);
  std::printf("%s_counts = %u %u %u %d\n", tag, m.countVertices(), m.countTriangles(), m.countExternal(), m.info().n_rebound);
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
  // the drawn mesh: a 12 x 7 sheet through the body, off the lattice, and its triangles
  const int mu = 12, mv = 7;
  std::vector<double> pts;
  std::vector<int> tri;
  for (int a = 0; a < mu; a++)
    for (int b = 0; b < mv; b++) {
      const double s = 0.031 + 0.0577 * a, u = 0.023 + 0.0413 * b;
      pts.push_back(s); pts.push_back(u); pts.push_back(0.071 + 0.11 * s + 0.37 * u);
    }
  for (int a = 0; a + 1 < mu; a++)
    for (int b = 0; b + 1 < mv; b++) {
      const int p0 = a * mv + b, p1 = (a + 1) * mv + b, p2 = a * mv + b + 1, p3 = (a + 1) * mv + b + 1;
      const int two[6] = {p0, p1, p2, p1, p3, p2};
      tri.insert(tri.end(), two, two + 6);
    }
  Deformable d((int)(xyz.size() / 3), xyz.data(), (int)(tets.size() / 4), tets.data(), fixed);
  EmbeddedMesh* m = d.embed(pts, tri);
  EXPECT(m->id() == 0 && m->countVertices() == (U32)(mu * mv) && m->countTriangles() == (U32)(2 * (mu - 1) * (mv - 1)) && m->countExternal() == 0);
  {
    EmbeddedMesh second(d.getIntegrator(), pts, std::vector<int>());  // directly over the integrator, released at the end of the scope
    EXPECT(second.id() == 1 && second.countTriangles() == 0);
    second.applyDisplacements();
    m->applyDisplacements();
    EXPECT(second.positions() == m->positions());
  }
  EmbeddedMesh* again = d.embed(pts);
  EXPECT(again->id() == 1);  // the slot is reused
  for (int step = 0; step < 3; step++) d.timestep();
  if (dump("steps", d, *m)) return 1;
  const std::vector<vec3d> seg = {vec3d(0.37, -1, 0), vec3d(0.37, 1, 0)};
  EXPECT(d.cut(seg, plane(0.35, 2.0), true) > 0);
  for (int step = 0; step < 2; step++) d.timestep();
  if (dump("cut", d, *m)) return 1;
  EXPECT(m->info().n_rebound > 0);
  std::printf("embed_host = ok\n");
  return 0;
}
