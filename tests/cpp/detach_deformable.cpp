// Deformable::detachPart / convertDisjointPartsToMeshes (include/fembrain/Deformable.h) on a cube cut twice into four parts: a part
// detached and kept, then every part a body of its own, the original left with one part, a step of every body.
// Prints "detach_deformable ok" on success.
#include <algorithm>
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

// one quad about the plane x = const (axis 0) or y = const (axis 1), slightly tilted so that it passes no node
static std::vector<vec3d> plane(int axis, double at, double half) {
  const double c = 0.25;
  const double d[4] = {-0.013 * half, 0.007 * half, -0.007 * half, 0.013 * half};
  const double u[4] = {c - half, c - half, c + half, c + half}, w[4] = {c - half, c + half, c - half, c + half};
  std::vector<vec3d> q;
  for (int i = 0; i < 4; i++) q.push_back(axis == 0 ? vec3d(at + d[i], u[i], w[i]) : vec3d(u[i], at + d[i], w[i]));
  return q;
}

static bool step_converges(Deformable& d) {
  d.getIntegrator()->SetUniformForce(1, -10000.0);
  return d.getIntegrator()->DoTimestep() == 0;
}

int main() {
  const int n = 6;
  const double h = 0.1;
  std::vector<double> xyz;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++)
      for (int k = 0; k < n; k++) { xyz.push_back(i * h); xyz.push_back(j * h); xyz.push_back(k * h); }
  auto id = [&](int i, int j, int k) { return (i * n + j) * n + k; };
  std::vector<int> tets;
  for (int i = 0; i + 1 < n; i++)
    for (int j = 0; j + 1 < n; j++)
      for (int k = 0; k + 1 < n; k++) {  // 6 tets around the cube diagonal (0 -> 7)
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
  for (int j = 0; j < n; j++)
    for (int k = 0; k < n; k++) fixed.push_back(id(0, j, k));
  Deformable d((int)(xyz.size() / 3), xyz.data(), (int)(tets.size() / 4), tets.data(), fixed);
  // fewer than two parts: nothing happens
  std::vector<Deformable*> bodies;
  EXPECT(d.convertDisjointPartsToMeshes(bodies) == 0 && bodies.empty());
  const std::vector<vec3d> seg = {vec3d(0.27, -1, 0), vec3d(0.27, 1, 0)};
  EXPECT(d.cut(seg, plane(0, 0.245, 2.0), true) > 0);
  EXPECT(d.cut(seg, plane(1, 0.255, 2.0), true) > 0);
  EXPECT(d.countDisjointParts() == 4);
  const size_t cells_before = d.countCells(), nodes_before = d.countNodes();
  d.setDampingStiffnessCoeff(0.05);   // away from the defaults (0.01, 0.0333): what a detached body must take over
  d.getIntegrator()->SetTimestep(0.02);
  std::vector<std::vector<U32> > groups;
  EXPECT(d.getDisjointParts(groups) == 4);

  // one part detached and kept: a body of its own with the part's cells, the original as it was
  bool threw = false;
  try { d.detachPart(4, false); } catch (const std::exception&) { threw = true; }
  EXPECT(threw);
  Deformable* copy = d.detachPart(2, false);
  EXPECT(copy->countCells() == groups[2].size() && copy->countDisjointParts() == 1);
  EXPECT(d.countCells() == cells_before && d.countDisjointParts() == 4);
  // the piece's host side knows the parameters it inherited: setting ONE damping coefficient leaves the other as the parent had it, so
  // the body steps bit for bit like a second copy nobody touched
  EXPECT(copy->getIntegrator()->GetTimestep() == 0.02 && copy->getDampingStiffnessCoeff() == 0.05);
  Deformable* twin = d.detachPart(2, false);
  copy->setDampingMassCoeff(0.0);
  EXPECT(step_converges(*copy) && step_converges(*twin));
  const double* qa = copy->getIntegrator()->Getq();
  const double* qb = twin->getIntegrator()->Getq();
  double largest = 0.0;
  for (int i = 0; i < copy->getIntegrator()->Getr(); i++) {
    EXPECT(qa[i] == qb[i]);
    largest = std::max(largest, std::fabs(qa[i]));
  }
  EXPECT(largest > 0.0);
  delete copy;
  delete twin;

  // every part a body, the original left with part 0
  EXPECT(d.convertDisjointPartsToMeshes(bodies) == 4 && bodies.size() == 3);
  EXPECT(d.countDisjointParts() == 1);
  EXPECT(d.countCells() == groups[0].size() && d.countNodes() == nodes_before);
  size_t total = d.countCells();
  for (size_t b = 0; b < bodies.size(); b++) {
    EXPECT(bodies[b]->countCells() == groups[b + 1].size());   // ascending part order
    EXPECT(bodies[b]->countDisjointParts() == 1);
    total += bodies[b]->countCells();
  }
  EXPECT(total == cells_before);
  EXPECT(d.convertDisjointPartsToMeshes(bodies) == 0 && bodies.size() == 3);
  EXPECT(step_converges(d));
  for (size_t b = 0; b < bodies.size(); b++) {
    EXPECT(step_converges(*bodies[b]));
    bodies[b]->timestep();   // ... and the per-step driver runs on a detached body
  }
  std::printf("detach_deformable ok: bodies of %u, %u, %u and %u cells\n", d.countCells(), bodies[0]->countCells(), bodies[1]->countCells(), bodies[2]->countCells());
  for (size_t b = 0; b < bodies.size(); b++) delete bodies[b];
  return 0;
}
