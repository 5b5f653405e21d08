// Host program over two PS::FEM::Deformable bodies, body_contact_classes.cpp's pair: a small cube sunk into the top of a clamped larger
// one.  Two frictionless rounds of timestep() on both set them moving; then setContactFriction on both, one collideWith (the forces of
// fb_fem_body_contact_friction in both external force vectors, its classes, maxima and per-contact records), three more rounds through
// the timestep() opt-in, a selfCollide, and friction off again.
// Prints one KEY=VALUE line per fact for tests/test_cpp_friction.py, which runs the Python driver through the same sequence.
#include <cstdio>
#include <vector>

#include "fembrain/Deformable.h"

// meshgen.truth_cube(n, n, n, h) in its own arithmetic, start + index * cellsize, then moved by `shift`
static void cube(int n, double h, const double* shift, std::vector<double>& v, std::vector<int>& t) {
  const double start[3] = {-(double)n / 2.0 * h, 0.0 * h, -(double)n / 2.0 * h};
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) for (int k = 0; k < n; k++) {
    v.push_back((start[0] + (double)i * h) + shift[0]); v.push_back((start[1] + (double)j * h) + shift[1]); v.push_back((start[2] + (double)k * h) + shift[2]);
  }
  for (int i = 0; i < n - 1; i++) for (int j = 0; j < n - 1; j++) for (int k = 0; k < n - 1; k++) {
    int c[8];
    for (int q = 0; q < 8; q++) c[q] = (i + ((q >> 2) & 1)) * n * n + (j + ((q >> 1) & 1)) * n + k + (q & 1);
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
  const int na = 3, nb = 5;
  const double h = 0.1, stiffness = 200.0, mu = 0.5, slip = 0.15, damping = 5.0, none[3] = {0.0, 0.0, 0.0}, off[3] = {0.1291, 0.3637, 0.0559};
  const double start_a[3] = {-(double)na / 2.0 * h, 0.0 * h, -(double)na / 2.0 * h}, start_b[3] = {-(double)nb / 2.0 * h, 0.0 * h, -(double)nb / 2.0 * h};
  double shift[3];
  for (int k = 0; k < 3; k++) shift[k] = (start_b[k] + off[k]) - start_a[k];
  std::vector<double> va, vb;
  std::vector<int> ta, tb, fixed;
  cube(na, h, shift, va, ta);
  cube(nb, h, none, vb, tb);
  for (int a = 0; a < nb * nb; a++) fixed.push_back(a);
  PS::FEM::Deformable A(na * na * na, va.data(), (int)ta.size() / 4, ta.data()), B(nb * nb * nb, vb.data(), (int)tb.size() / 4, tb.data(), fixed);
  A.setGravity(false);
  B.setGravity(false);

  // moving: two frictionless rounds
  A.setCollisionBody(&B, stiffness);
  B.setCollisionBody(&A, stiffness);
  for (int r = 0; r < 2; r++) {
    A.timestep();
    B.timestep();
  }

  A.setContactFriction(mu, slip, damping);
  B.setContactFriction(mu, slip, damping);
  A.integrator()->SetExternalForcesToZero();
  B.integrator()->SetExternalForcesToZero();
  const fb_fem_body_contact_info info = A.collideWith(B, stiffness);
  const fb_fem_contact_friction_info fi = A.lastContactFriction();
  std::printf("N_AB=%d\nN_BA=%d\nON_A=%.17g,%.17g,%.17g\nON_B=%.17g,%.17g,%.17g\n", info.n_contacts[0], info.n_contacts[1], info.force_on_a[0], info.force_on_a[1],
              info.force_on_a[2], info.force_on_b[0], info.force_on_b[1], info.force_on_b[2]);
  std::printf("CLASSES=%d,%d,%d,%d,%d,%d\nMAXIMA=%.17g,%.17g,%.17g\nFRICTION_AB=%.17g,%.17g,%.17g\nFRICTION_BA=%.17g,%.17g,%.17g\n", fi.n_sticking[0], fi.n_sticking[1],
              fi.n_sliding[0], fi.n_sliding[1], fi.n_separating[0], fi.n_separating[1], fi.max_slip_speed, fi.max_normal_force, fi.max_stick_rate,
              fi.friction_on_points[0][0], fi.friction_on_points[0][1], fi.friction_on_points[0][2], fi.friction_on_points[1][0], fi.friction_on_points[1][1],
              fi.friction_on_points[1][2]);
  std::vector<double> N, slip3, friction3, fa, fb;
  A.integrator()->ReadBodyContactFriction(FB_BODY_A_INTO_B, info.n_contacts[0], N, slip3, friction3);
  A.externalForces(fa);
  B.externalForces(fb);
  std::printf("NSUM=%.17g\nSLIPSUM=%.17g\nFRICSUM=%.17g\nFEXT_A=%.17g\nFEXT_B=%.17g\n", weighted(N), weighted(slip3), weighted(friction3), weighted(fa), weighted(fb));

  for (int r = 0; r < 3; r++) {
    A.timestep();
    B.timestep();
  }
  std::vector<double> qa((size_t)A.getDof()), qb((size_t)B.getDof());
  A.integrator()->GetqState(qa.data());
  B.integrator()->GetqState(qb.data());
  std::printf("QSUM_A=%.17g\nQSUM_B=%.17g\nITERS_A=%d\nITERS_B=%d\n", weighted(qa), weighted(qb), A.integrator()->GetLastIterations(), B.integrator()->GetLastIterations());

  // the body against itself through the friction entry point (one convex part: nothing to meet), then friction off: the frictionless call
  const fb_fem_self_contact_info self = A.selfCollide(stiffness, 0.0, FB_SELF_CONTACT_ANY);
  std::printf("SELF=%d,%d\n", self.n_points, self.n_contacts);
  A.setContactFriction(0.0, 0.0, 0.0);
  A.integrator()->SetExternalForcesToZero();
  B.integrator()->SetExternalForcesToZero();
  const fb_fem_body_contact_info plain = A.collideWith(B, stiffness);
  std::printf("PLAIN_ON_A=%.17g,%.17g,%.17g\n", plain.force_on_a[0], plain.force_on_a[1], plain.force_on_a[2]);
  return 0;
}
