// Host program over ONE PS::FEM::Deformable, the 9 x 9 x 9-node cube clamped at its bottom plane, and a rigid tool of a capsule, a sphere
// and an axis-aligned box over its top face: collideTool once without and once with friction (the forces of fb_fem_tool_contact in the
// external force vector, the wrench the tissue returns), then setTool and three rounds of timestep() with the tool lowered each round,
// gravity off.  Prints one KEY=VALUE line per fact for tests/test_cpp_tool_contact.py, which runs the Python driver through the same
// sequence.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fembrain/Deformable.h"

// meshgen.truth_cube(n, n, n, h) in its own arithmetic, start + index * cellsize
static void cube(int n, double h, std::vector<double>& v, std::vector<int>& t, std::vector<int>& bottom) {
  const double start[3] = {-(double)n / 2.0 * h, 0.0 * h, -(double)n / 2.0 * h};
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) for (int k = 0; k < n; k++) {
    if (j == 0) bottom.push_back((int)v.size() / 3);
    v.push_back(start[0] + (double)i * h); v.push_back(start[1] + (double)j * h); v.push_back(start[2] + (double)k * h);
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

// the tool with its lowest point `drop` below where it starts
static fb_tool tool_at(double drop) {
  fb_tool T;
  memset(&T, 0, sizeof(T));
  T.n_shapes = 3;
  fb_tool_shape& cap = T.shapes[0];
  cap.kind = FB_TOOL_CAPSULE;
  cap.a[0] = -0.3; cap.a[1] = 0.85 - drop; cap.a[2] = -0.2;
  cap.b[0] = 0.2; cap.b[1] = 0.9 - drop; cap.b[2] = 0.1;
  cap.size[0] = 0.18;
  fb_tool_shape& tip = T.shapes[1];
  tip.kind = FB_TOOL_SPHERE;
  tip.a[0] = -0.037; tip.a[1] = 0.85 - drop; tip.a[2] = -0.054;
  tip.size[0] = 0.25;
  fb_tool_shape& box = T.shapes[2];
  box.kind = FB_TOOL_BOX;
  box.a[0] = 0.21; box.a[1] = 0.83 - drop; box.a[2] = 0.19;
  box.size[0] = 0.12; box.size[1] = 0.09; box.size[2] = 0.15;
  box.R[0] = box.R[4] = box.R[8] = 1.0;
  T.origin[0] = 0.1; T.origin[1] = 0.9 - drop; T.origin[2] = -0.2;
  return T;
}

static void print_info(const char* tag, const fb_fem_tool_contact_info& I) {
  std::printf("N_%s=%d\nPOINTS_%s=%d\nBY_SHAPE_%s=%d,%d,%d\nCLASSES_%s=%d,%d,%d\nMAXDEPTH_%s=%.17g\n", tag, I.n_contacts, tag, I.n_points, tag, I.contacts_by_shape[0],
              I.contacts_by_shape[1], I.contacts_by_shape[2], tag, I.n_separating, I.n_sticking, I.n_sliding, tag, I.max_depth);
  std::printf("ON_TOOL_%s=%.17g,%.17g,%.17g\nTORQUE_%s=%.17g,%.17g,%.17g\n", tag, I.force_on_tool[0], I.force_on_tool[1], I.force_on_tool[2], tag, I.torque_on_tool[0],
              I.torque_on_tool[1], I.torque_on_tool[2]);
}

int main() {
  const int n = 9;
  const double stiffness = 1000.0;
  std::vector<double> v, f;
  std::vector<int> t, bottom;
  cube(n, 0.1, v, t, bottom);
  PS::FEM::Deformable D((int)v.size() / 3, v.data(), (int)t.size() / 4, t.data(), bottom);
  D.setGravity(false);

  // one direct call without friction, one with
  fb_tool T = tool_at(0.0);
  D.integrator()->SetExternalForcesToZero();
  fb_fem_tool_contact_info info = D.collideTool(T, stiffness);
  print_info("PLAIN", info);
  std::vector<int> node, shape;
  std::vector<double> depth, normal, force, N, slip, friction;
  D.integrator()->ReadToolContact(info.n_contacts, node, shape, depth, normal, force);
  long long idsum = 0;
  for (size_t i = 0; i < node.size(); i++) idsum += (long long)(node[i] + 3 * shape[i]) * (long long)(i + 1);
  D.externalForces(f);
  std::printf("IDSUM=%lld\nDEPTHSUM=%.17g\nFORCESUM=%.17g\nFEXT_PLAIN=%.17g\n", idsum, weighted(depth), weighted(force), weighted(f));
  std::printf("WRENCH=%.17g,%.17g\n", D.toolForce().y, D.toolTorque().z);

  D.setContactFriction(0.4, 0.3, 40.0);
  T.velocity[0] = 0.3; T.velocity[1] = -0.2; T.velocity[2] = 0.1;
  T.omega[0] = 0.5; T.omega[1] = 1.0; T.omega[2] = -0.7;
  D.integrator()->SetExternalForcesToZero();
  info = D.collideTool(T, stiffness, 0.04, FB_TOOL_ALL_NODES);
  print_info("FRICTION", info);
  D.integrator()->ReadToolContactFriction(info.n_contacts, N, slip, friction);
  D.externalForces(f);
  std::printf("NSUM=%.17g\nSLIPSUM=%.17g\nFRICTIONSUM=%.17g\nFEXT_FRICTION=%.17g\n", weighted(N), weighted(slip), weighted(friction), weighted(f));

  // the tool in timestep(): lowered by 0.01 per round, with friction
  for (int r = 1; r <= 3; r++) {
    fb_tool moved = tool_at(0.01 * r);
    moved.velocity[1] = -0.01 / 0.0333;
    D.setTool(moved, stiffness);
    D.timestep();
  }
  std::vector<double> q((size_t)D.getDof());
  D.integrator()->GetqState(q.data());
  print_info("STEPPED", D.lastToolContact());
  std::printf("QSUM=%.17g\nITERS=%d\n", weighted(q), D.integrator()->GetLastIterations());
  D.clearTool();
  std::printf("OFF=%d\n", D.hasTool() ? 0 : 1);
  return 0;
}
