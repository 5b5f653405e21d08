// Host program over ONE PS::FEM::Deformable: a beam clamped at one end whose other end a tool grips, drags and twists for three steps
// (grip / moveGrip / gripForce: the held nodes follow, the tissue's force comes back from the device), then lets go (releaseGrip) for
// one more step, gravity off.  What the reference only flags (IAvatar::grip(), IScalpel.cpp:42-44).
// Prints one KEY=VALUE line per fact for tests/test_cpp_motion.py, which runs the Python driver through the same sequence.
#include <cstdio>
#include <vector>

#include "fembrain/Deformable.h"

// meshgen.truth_cube(nx, ny, nz, h) in its own arithmetic
static void cube(int nx, int ny, int nz, double h, std::vector<double>& v, std::vector<int>& t) {
  const double start[3] = {-(double)nx / 2.0 * h, 0.0 * h, -(double)nz / 2.0 * h};
  for (int i = 0; i < nx; i++) for (int j = 0; j < ny; j++) for (int k = 0; k < nz; k++) {
    v.push_back(start[0] + (double)i * h); v.push_back(start[1] + (double)j * h); v.push_back(start[2] + (double)k * h);
  }
  for (int i = 0; i < nx - 1; i++) for (int j = 0; j < ny - 1; j++) for (int k = 0; k < nz - 1; k++) {
    int c[8];
    for (int q = 0; q < 8; q++) c[q] = (i + ((q >> 2) & 1)) * ny * nz + (j + ((q >> 1) & 1)) * nz + k + (q & 1);
    const int pat[6][4] = {{0, 2, 4, 1}, {6, 2, 1, 4}, {6, 2, 3, 1}, {6, 4, 1, 5}, {6, 1, 3, 5}, {6, 3, 7, 5}};
    for (int a = 0; a < 6; a++) for (int b = 0; b < 4; b++) t.push_back(c[pat[a][b]]);
  }
}

static double weighted(const std::vector<double>& x) {
  double s = 0.0;
  for (size_t i = 0; i < x.size(); i++) s += x[i] * (double)(i % 7 + 1);
  return s;
}

int main() {
  const int nx = 6, ny = 3, nz = 3;
  std::vector<double> v;
  std::vector<int> t, fixed, held;
  cube(nx, ny, nz, 0.1, v, t);
  const int n = nx * ny * nz;
  for (int i = 0; i < ny * nz; i++) { fixed.push_back(i); held.push_back(n - ny * nz + i); }
  PS::FEM::Deformable D(n, v.data(), (int)t.size() / 4, t.data(), fixed);
  D.setGravity(false);

  const fb_fem_motion_info at_grip = D.grip((int)held.size(), held.data());
  std::printf("GRIP_DOFS=%d\nGRIP_NODES=%d\n", at_grip.n_dofs, at_grip.n_grasp_nodes);
  const double pivot[3] = {v[3 * (size_t)held[4]], v[3 * (size_t)held[4] + 1], v[3 * (size_t)held[4] + 2]};  // the middle of the held face
  for (int r = 0; r < 3; r++) {
    // a rotation about x by a rational angle (the same bits in any language): c = (m^2 - 1) / (m^2 + 1), s = 2 m / (m^2 + 1)
    const double m = 60.0 / (double)(r + 1), c = (m * m - 1.0) / (m * m + 1.0), s = 2.0 * m / (m * m + 1.0);
    const double R[9] = {1.0, 0.0, 0.0, 0.0, c, -s, 0.0, s, c}, shift[3] = {0.002 * (double)(r + 1), 0.0, 0.0};
    D.moveGrip(R, shift, pivot);
    D.timestep();
    double f[3];
    D.gripForce(f);
    std::printf("FORCE_%d=%.17g,%.17g,%.17g\nITERS_%d=%d\n", r, f[0], f[1], f[2], r, D.integrator()->GetLastIterations());
  }
  const fb_fem_motion_info held_info = D.integrator()->MotionInfo();
  std::printf("LISTED=%d\nTOUCHED=%d\nLONGEST=%d\nBUILDS=%d\n", held_info.n_listed_elements, held_info.n_touched_nodes, held_info.longest_run, held_info.table_builds);
  std::vector<double> q((size_t)D.getDof()), react;
  D.integrator()->GetqState(q.data());
  double sum3[3];
  D.integrator()->ReadReactions(&react, sum3);
  std::printf("QSUM_HELD=%.17g\nREACT=%.17g\n", weighted(q), weighted(react));

  D.releaseGrip();
  std::vector<int> dofs;
  D.integrator()->ReadConstrainedDofs(dofs);
  const fb_fem_motion_info after = D.integrator()->MotionInfo();
  std::printf("FIXED_AFTER=%d\nSET_AFTER=%d\n", (int)dofs.size(), after.n_dofs);
  D.timestep();
  D.integrator()->GetqState(q.data());
  std::printf("QSUM_FREE=%.17g\nITERS_FREE=%d\n", weighted(q), D.integrator()->GetLastIterations());
  return 0;
}
