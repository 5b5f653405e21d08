// Host program over ONE PS::FEM::Deformable that holds two cubes, a small one sunk into a corner of a flat one (bodycontactref's "two_way"
// as one mesh): selfCollide once in both modes (the contact forces of fb_fem_self_contact in the external force vector), then
// setSelfCollision and three rounds of timestep(), gravity off: the two cubes push each other apart.
// Prints one KEY=VALUE line per fact for tests/test_cpp_self_contact.py, which runs the Python driver through the same sequence.
#include <cstdio>
#include <vector>

#include "fembrain/Deformable.h"

// meshgen.truth_cube(nx, ny, nz, h) in its own arithmetic, start + index * cellsize, then moved by `shift`; node ids from `base`
static void cube(int nx, int ny, int nz, double h, const double* shift, int base, std::vector<double>& v, std::vector<int>& t) {
  const double start[3] = {-(double)nx / 2.0 * h, 0.0 * h, -(double)nz / 2.0 * h};
  for (int i = 0; i < nx; i++) for (int j = 0; j < ny; j++) for (int k = 0; k < nz; k++) {
    v.push_back((start[0] + (double)i * h) + shift[0]); v.push_back((start[1] + (double)j * h) + shift[1]); v.push_back((start[2] + (double)k * h) + shift[2]);
  }
  for (int i = 0; i < nx - 1; i++) for (int j = 0; j < ny - 1; j++) for (int k = 0; k < nz - 1; k++) {
    int c[8];
    for (int q = 0; q < 8; q++) c[q] = base + (i + ((q >> 2) & 1)) * ny * nz + (j + ((q >> 1) & 1)) * nz + k + (q & 1);
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
  const int a[3] = {4, 4, 4}, b[3] = {6, 3, 6};
  const double h = 0.1, stiffness = 200.0, none[3] = {0.0, 0.0, 0.0}, off[3] = {0.1291, 0.1637, 0.0559};
  const double start_a[3] = {-(double)a[0] / 2.0 * h, 0.0 * h, -(double)a[2] / 2.0 * h}, start_b[3] = {-(double)b[0] / 2.0 * h, 0.0 * h, -(double)b[2] / 2.0 * h};
  double shift[3];
  for (int k = 0; k < 3; k++) shift[k] = (start_b[k] + off[k]) - start_a[k];
  std::vector<double> v;
  std::vector<int> t;
  cube(a[0], a[1], a[2], h, shift, 0, v, t);
  const int na = (int)v.size() / 3;
  cube(b[0], b[1], b[2], h, none, na, v, t);
  PS::FEM::Deformable D((int)v.size() / 3, v.data(), (int)t.size() / 4, t.data());
  D.setGravity(false);

  const int modes[2] = {FB_SELF_CONTACT_ANY, FB_SELF_CONTACT_OTHER_PARTS};
  for (int m = 0; m < 2; m++) {
    D.integrator()->SetExternalForcesToZero();
    const fb_fem_self_contact_info info = D.selfCollide(stiffness, 0.0, modes[m]);
    std::printf("N_%d=%d\nPOINTS_%d=%d\nPARTS_BUILDS_%d=%d\nMAXDEPTH_%d=%.17g\nON_POINTS_%d=%.17g,%.17g,%.17g\nON_FACES_%d=%.17g,%.17g,%.17g\n", m, info.n_contacts, m, info.n_points, m,
                info.n_parts_builds, m, info.max_depth, m, info.force_on_points[0], info.force_on_points[1], info.force_on_points[2], m, info.force_on_faces[0],
                info.force_on_faces[1], info.force_on_faces[2]);
    std::vector<int> node, element, face;
    std::vector<double> closest, bary, depth, f;
    D.integrator()->ReadSelfContact(info.n_contacts, node, element, face, closest, bary, depth);
    long long idsum = 0;
    for (size_t i = 0; i < node.size(); i++) idsum += (long long)(node[i] + 3 * element[i] + 7 * face[i]) * (long long)(i + 1);
    D.externalForces(f);
    std::printf("IDSUM_%d=%lld\nDEPTHSUM_%d=%.17g\nFEXT_%d=%.17g\n", m, idsum, m, weighted(depth), m, weighted(f));
  }
  std::printf("CAPPED=%.17g\n", D.selfCollide(stiffness, 0.01).max_depth);

  D.setSelfCollision(true, stiffness);
  for (int r = 0; r < 3; r++) D.timestep();
  std::vector<double> q((size_t)D.getDof());
  D.integrator()->GetqState(q.data());
  std::printf("QSUM=%.17g\nITERS=%d\n", weighted(q), D.integrator()->GetLastIterations());
  D.setSelfCollision(false);
  std::printf("OFF=%d\n", D.getSelfCollision() ? 0 : 1);
  return 0;
}
