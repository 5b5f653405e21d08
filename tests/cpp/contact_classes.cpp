// Host program over PS::FEM::AvatarProbe and PS::FEM::Deformable: a tool box lowered onto the top of a clamped truth cube over three
// moves with a step after each (the contact session and its spread run on the device: fb_fem_contact_move / fb_fem_contact_apply under
// Deformable::timestep), then the probe's mouse-up and one more step.
// Prints one KEY=VALUE line per fact for tests/test_cpp_contact.py, which runs the Python driver through the same sequence.
#include <cstdio>
#include <vector>

#include "fembrain/AvatarProbe.h"

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
  d.setHapticForceRadius(3);

  PS::FEM::AvatarProbe probe(&d);
  probe.setForceCoeff(21345.73);
  const int idle = probe.onTranslate(PS::FEM::vec3d(-1.0, -1.0, -1.0), PS::FEM::vec3d(1.0, 1.0, 1.0));   // no probing in progress: nothing happens
  std::printf("IDLE=%d\nIDLE_TOUCHED=%d\n", idle, d.integrator()->ContactInfo().n_touched);
  probe.start();
  const double top = start[1] + 4.0 * h, depth[3] = {0.02, 0.06, 0.12};
  for (int k = 0; k < 3; k++) {
    const int status = probe.onTranslate(PS::FEM::vec3d(-1.25, top - depth[k], -1.25), PS::FEM::vec3d(1.15, top + 1.0, 1.15));
    const fb_fem_contact_info& c = probe.lastContact();
    std::printf("STATUS%d=%d\nTOUCHED%d=%d\nNEW%d=%d\nFACE%d=%d\nFACENAME%d=%s\nCLOSEST%d=%d\nPUSHING%d=%d\nDIST%d=%.17g\nPOINT%d=%.17g,%.17g,%.17g\n", k, status, k, probe.countTouched(), k,
                c.n_new, k, probe.contactFace(), k, PS::FEM::AvatarProbe::faceName(probe.contactFace()), k, probe.closestVertex(), k, c.n_pushing, k, probe.contactDist(), k,
                probe.closestPoint().x, probe.closestPoint().y, probe.closestPoint().z);
    d.timestep();
  }
  std::vector<int> ids;
  std::vector<double> first, forces;
  d.integrator()->ReadContact(ids, first, forces);
  long long idsum = 0;
  double fsum = 0.0;
  for (size_t i = 0; i < ids.size(); i++) { idsum += (long long)ids[i] * (long long)(i + 1); fsum += forces[3 * i + 1] * (double)(i % 5 + 1); }
  std::printf("LIST=%d\nLIST_IDSUM=%lld\nLIST_FSUM=%.17g\n", (int)ids.size(), idsum, fsum);
  probe.end();
  d.timestep();
  const fb_fem_contact_info after = d.integrator()->ContactInfo();
  const double* q = d.integrator()->Getq();
  double qsum = 0.0;
  for (unsigned i = 0; i < d.getDof(); i++) qsum += q[i] * (double)(i % 7 + 1);
  std::printf("END_LIST=%d\nEND_FACE=%d\nIN_PROGRESS=%d\nQSUM=%.17g\nITERS=%d\n", after.list_size, after.face, d.isHapticInProgress() ? 1 : 0, qsum, d.integrator()->GetLastIterations());
  return 0;
}
