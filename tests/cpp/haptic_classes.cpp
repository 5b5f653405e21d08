// Host program over PS::FEM::Deformable with a probe on: a truth cube whose far corner column is picked, pulled for two steps through
// the device spread (fb_fem_add_haptic_forces under Deformable::timestep), then picked around, measured and summed.
// Prints one KEY=VALUE line per fact for tests/test_cpp_haptic.py, which runs the Python driver through the same sequence.
#include <cstdio>
#include <vector>

#include "fembrain/Deformable.h"

int main() {
  // meshgen.truth_cube(5, 5, 5, 0.1) in its own arithmetic: start + index * cellsize
  const int n = 5;
  const double h = 0.1, start[3] = {-(double)n / 2.0 * h, 0.0 * h, -(double)n / 2.0 * h};
  std::vector<double> v;
  std::vector<int> t;
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) for (int k = 0; k < n; k++) {
    v.push_back(start[0] + (double)i * h); v.push_back(start[1] + (double)j * h); v.push_back(start[2] + (double)k * h);
  }
  for (int i = 0; i < n - 1; i++) for (int j = 0; j < n - 1; j++) for (int k = 0; k < n - 1; k++) {
    int c[8];
    for (int q = 0; q < 8; q++) c[q] = (i + ((q >> 2) & 1)) * n * n + (j + ((q >> 1) & 1)) * n + k + (q & 1);
    const int pat[6][4] = {{0, 2, 4, 1}, {6, 2, 1, 4}, {6, 2, 3, 1}, {6, 4, 1, 5}, {6, 1, 3, 5}, {6, 3, 7, 5}};
    for (int a = 0; a < 6; a++) for (int b = 0; b < 4; b++) t.push_back(c[pat[a][b]]);
  }
  std::vector<int> fixed;
  for (int a = 0; a < n * n; a++) fixed.push_back(a);
  PS::FEM::Deformable d(n * n * n, v.data(), (int)t.size() / 4, t.data(), fixed);

  PS::FEM::vec3d hit;
  const bool clamped = d.hapticStart(PS::FEM::vec3d(-10.0, 0.23, 10.0));   // lands on the clamped plane: refused
  d.hapticEnd();
  const bool started = d.hapticStart(PS::FEM::vec3d(10.0, 0.23, 10.0));
  const int picked = d.pickVertex(PS::FEM::vec3d(10.0, 0.23, 10.0), hit);
  std::vector<int> idx;
  std::vector<PS::FEM::vec3d> frc;
  idx.push_back(picked); frc.push_back(PS::FEM::vec3d(0.0, 2500.0, 300.0));
  idx.push_back(picked - 1); frc.push_back(PS::FEM::vec3d(-200.0, 900.0, 0.0));
  d.hapticSetCurrentForces(idx, frc);
  const double vol0 = d.computeVolume();
  d.timestep();
  d.timestep();

  const int again = d.pickVertex(PS::FEM::vec3d(10.0, 0.23, 10.0), hit);
  std::vector<PS::FEM::vec3d> found;
  std::vector<int> foundIdx;
  // a box of one and a half cells around where the pulled corner has got to (the body sags: a box fixed in space would be left behind)
  const int nbox = d.pickVertices(PS::FEM::vec3d(hit.x - 0.15, hit.y - 0.15, hit.z - 0.15), PS::FEM::vec3d(hit.x + 0.15, hit.y + 0.15, hit.z + 0.15), found, foundIdx);
  long long idsum = 0;
  for (size_t i = 0; i < foundIdx.size(); i++) idsum += (long long)foundIdx[i] * (long long)(i + 1);
  std::vector<double> per(d.countCells(), 0.0);
  const double vol = d.computeVolume(per.data(), d.countCells());
  double persum = 0.0;
  for (size_t e = 0; e < per.size(); e++) persum += per[e];
  const double* q = d.integrator()->Getq();
  double qsum = 0.0;
  for (unsigned i = 0; i < d.getDof(); i++) qsum += q[i] * (double)(i % 7 + 1);
  std::printf("CLAMPED_START=%d\nSTARTED=%d\nPICKED=%d\nPICKED_AGAIN=%d\nPICK_XYZ=%.17g,%.17g,%.17g\n", clamped ? 1 : 0, started ? 1 : 0, picked, again, hit.x, hit.y, hit.z);
  std::printf("BOX=%d\nBOX_IDSUM=%lld\nBOX_LAST=%.17g,%.17g,%.17g\n", nbox, idsum, found.empty() ? 0.0 : found.back().x, found.empty() ? 0.0 : found.back().y,
              found.empty() ? 0.0 : found.back().z);
  std::printf("VOL0=%.17g\nVOL=%.17g\nVOL_PERSUM=%.17g\nVOL_CHANGED=%d\nQSUM=%.17g\nITERS=%d\n", vol0, vol, persum, d.isVolumeChanged() ? 1 : 0, qsum,
              d.integrator()->GetLastIterations());
  return 0;
}
