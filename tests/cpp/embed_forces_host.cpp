// The way back from a PS::FEM::EmbeddedMesh (include/fembrain/EmbeddedMesh.h) over a Deformable: addForces with and without a list,
// pickRay, pickPoint, touch and applyStress after steps.  Prints what it gave them and what came back, with the mesh, state and binding
// they belong to; tests/test_cpp_embed_forces.py reproduces the values with numpy.
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

static void print_doubles(const char* key, const std::vector<double>& a) {
  std::printf("%s =", key);
  for (double x : a) std::printf(" %.17g", x);
  std::printf("\n");
}
static void print_ints(const char* key, const std::vector<int>& a) {
  std::printf("%s =", key);
  for (int x : a) std::printf(" %d", x);
  std::printf("\n");
}
static void print_forces(const char* key, Deformable& d) {
  std::vector<double> f;
  d.externalForces(f);
  print_doubles(key, f);
}
static void print_hit(const char* key, const vec3d& o, const vec3d& dir, const EmbeddedMesh::RayHit& hit) {
  std::printf("%s = %.17g %.17g %.17g %.17g %.17g %.17g %d %.17g %.17g %.17g %.17g %.17g %.17g\n", key, o.x, o.y, o.z, dir.x, dir.y, dir.z, hit.triangle, hit.t, hit.u,
              hit.v, hit.point.x, hit.point.y, hit.point.z);
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
        for (int e = 0; e < 6; e++) tets.insert(tets.end(), {c[t[e][0]], c[t[e][1]], c[t[e][2]], c[t[e][3]]});
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
  const int np = (int)m->countVertices();
  EXPECT(np == mu * mv && m->countExternal() == 0);
  for (int step = 0; step < 3; step++) d.timestep();

  // the mesh, the state and the binding everything below belongs to
  fb_fem_t fh = d.getIntegrator()->handle();
  std::vector<double> rest((size_t)3 * fb_fem_num_nodes(fh)), q(rest.size()), w, loc;
  std::vector<int> el((size_t)4 * fb_fem_num_tets(fh)), be, bv;
  EXPECT(fb_fem_read_mesh(fh, rest.data(), el.data()) == FB_OK);
  EXPECT(fb_fem_get_state(fh, q.data(), nullptr, nullptr) == FB_OK);
  m->readBinding(be, bv, w, loc);
  print_doubles("rest", rest);
  print_doubles("q", q);
  print_ints("tets", el);
  print_ints("elements", be);
  print_ints("vertices", bv);
  print_doubles("weights", w);
  print_ints("triangles", m->triangles());

  // forces: a list, then every point, on top of a uniform load
  d.getIntegrator()->SetUniformForce(1, -300.0);
  print_forces("f_base", d);
  const std::vector<int> ids = {2, 17, 18, 40, 83};
  std::vector<vec3d> fl;
  for (size_t s = 0; s < ids.size(); s++) fl.push_back(vec3d(1.5 + 0.25 * s, -7.0 + 1.125 * s, 0.375 * s));
  m->addForces(ids, fl);
  print_ints("list_ids", ids);
  std::printf("list_forces =");
  for (const vec3d& f : fl) std::printf(" %.17g %.17g %.17g", f.x, f.y, f.z);
  std::printf("\n");
  print_forces("f_list", d);
  std::vector<vec3d> fa;
  for (int p = 0; p < np; p++) fa.push_back(vec3d(0.01 * p - 0.3, 2.0 - 0.03 * p, 0.5 + 0.001 * p * p));
  m->addForces(fa);
  std::printf("all_forces =");
  for (const vec3d& f : fa) std::printf(" %.17g %.17g %.17g", f.x, f.y, f.z);
  std::printf("\n");
  print_forces("f_all", d);
  bool refused = false;
  try {
    m->addForces(std::vector<int>{5, 3}, std::vector<vec3d>(2));
  } catch (const std::exception&) { refused = true; }
  EXPECT(refused);

  // picks at the current state
  m->applyDisplacements();
  const vec3d o1(0.2913, 0.1307, 1.0), d1(0.013, -0.021, -1.0), o2(0.4471, 0.0929, -0.8), d2(-0.05, 0.04, 1.7);
  print_hit("ray1", o1, d1, m->pickRay(o1, d1));
  print_hit("ray2", o2, d2, m->pickRay(o2, d2));
  print_hit("ray_miss", o1, vec3d(0, 0, 1), m->pickRay(o1, vec3d(0, 0, 1)));
  print_hit("ray_short", o1, d1, m->pickRay(o1, d1, 0.25));
  EXPECT(m->pickRay(o1, d1).triangle >= 0 && m->pickRay(o1, vec3d(0, 0, 1)).triangle == -1 && m->pickRay(o1, d1, 0.25).triangle == -1);
  vec3d at;
  const vec3d wp(0.31, 0.12, 0.17);
  const int best = m->pickPoint(wp, at);
  std::printf("point = %.17g %.17g %.17g %d %.17g %.17g %.17g\n", wp.x, wp.y, wp.z, best, at.x, at.y, at.z);

  // a click that pulls
  d.getIntegrator()->SetUniformForce(1, -300.0);
  const vec3d pull(4.0, -25.0, 1.5);
  EXPECT(d.touchEmbedded(m, o1, vec3d(0, 0, 1), pull) == -1);
  print_forces("f_untouched", d);
  const int hit = d.touchEmbedded(m, o1, d1, pull);
  std::printf("touch = %d %.17g %.17g %.17g\n", hit, pull.x, pull.y, pull.z);
  print_forces("f_touch", d);

  // colour
  bool stale = false;
  try {
    m->applyStress();
  } catch (const std::exception&) { stale = true; }
  EXPECT(stale);  // (no computeStress yet)
  d.computeStress();
  std::vector<double> vm;
  d.readStress(vm);
  print_doubles("von_mises", vm);
  m->applyStress();
  std::printf("stress =");
  for (U32 i = 0; i < m->countVertices(); i++) std::printf(" %.9g", m->stressAt(i));
  std::printf("\nembed_forces_host = ok\n");
  return 0;
}
