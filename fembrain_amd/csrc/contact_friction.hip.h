// Coulomb friction and damping of a contact, for body_contact.hip and self_contact.hip: the law of include/fembrain_hip.h ("Friction and
// damping of a contact"), written once, the side record it leaves per contact, the pass that looks for a velocity that is not finite,
// and what the host makes of the side records.  The searches, BodyContactRec and the scatter know nothing of it: the friction instances
// of k_contact_force (contact_force.hip.h) write the TOTAL force into rec[t].f, where k_contact_segments and the host sums find it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "body_contact.h"
#include "launch.hip.h"

namespace fb {
namespace {

// the three numbers of fb_fem_contact_friction_params, as the kernels take them
struct FrictionLaw {
  double mu, slip_speed, damping;
};

// the velocity of internal node nd (a node out of range: at rest)
__device__ __forceinline__ void node_velocity(const double* __restrict__ qvel, int n_nodes, int nd, double* v) {
  const bool ok = (unsigned)nd < (unsigned)n_nodes;
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = ok ? qvel[3 * (size_t)nd + k] : 0.0;
}

// The law.  p the point, (c, b, d) the closest point, its weights and |c - p| > 0 as bc_finish left them, vp the point's velocity,
// vt the three corners'.  F: the total force on the point's node; o: what fb_fem_read_*_contact_friction hands back.
// Every operation in the header's order; the unit is built without contraction.
__device__ __forceinline__ void contact_friction_law(const double* p, const double* c, const double* b, double d, double stiffness, double depth_cap, const FrictionLaw& L,
                                                     const double* vp, const double (*vt)[3], double* F, ContactFrictionRec& o) {
  const double depth = depth_cap > 0.0 ? fmin(d, depth_cap) : d;
  const double sd = stiffness * depth;
  double n[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    n[k] = (c[k] - p[k]) / d;
    const double vf = (b[0] * vt[0][k] + b[1] * vt[1][k]) + b[2] * vt[2][k];
    w[k] = vp[k] - vf;
  }
  const double vn = (w[0] * n[0] + w[1] * n[1]) + w[2] * n[2];
  double N = sd - L.damping * vn;
  if (!(N > 0.0)) N = 0.0;  // no adhesion
  double t[3];
#pragma unroll
  for (int k = 0; k < 3; k++) t[k] = w[k] - vn * n[k];
  const double s = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  const double den = fmax(s, L.slip_speed);
  const double g = den > 0.0 ? (L.mu * N) / den : 0.0;  // (den == 0 needs slip_speed == 0, which the call admits only with mu == 0)
  o.N = N;
  o.s = s;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double f = g * t[k];
    F[k] = N * n[k] - f;
    o.t[k] = t[k];
    o.mf[k] = -f;
  }
}

// A thread per DOF: a velocity that is not finite raises the flag (every writer stores the same value)
__global__ __launch_bounds__(kB) void k_cf_finite(long long n, const double* __restrict__ qvel, double* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i < n && !(fabs(qvel[i]) <= DBL_MAX)) *flag = 1.0;
}

// ---- host ----

// the penalty's two numbers as the calls accept them (here, where tool_contact.hip finds it too); who: "body contact" / "self contact" / "tool contact"
int check_penalty(const char* who, double stiffness, double depth_cap) {
  if (!std::isfinite(stiffness) || stiffness < 0.0) return fail(FB_EINVAL, "%s stiffness %g", who, stiffness);
  if (!std::isfinite(depth_cap) || depth_cap < 0.0) return fail(FB_EINVAL, "%s depth cap %g", who, depth_cap);
  return FB_OK;
}

// fb_fem_contact_friction_params as the calls accept them
int check_friction(const fb_fem_contact_friction_params* fr, const char* who) {
  if (!fr) return fail(FB_EINVAL, "%s: null friction parameters", who);
  if (!std::isfinite(fr->mu) || fr->mu < 0.0) return fail(FB_EINVAL, "%s: friction coefficient %g", who, fr->mu);
  if (!std::isfinite(fr->slip_speed) || fr->slip_speed < 0.0) return fail(FB_EINVAL, "%s: slip speed %g", who, fr->slip_speed);
  if (!std::isfinite(fr->damping) || fr->damping < 0.0) return fail(FB_EINVAL, "%s: contact damping %g", who, fr->damping);
  if (fr->mu > 0.0 && fr->slip_speed == 0.0) return fail(FB_EINVAL, "%s: friction needs a slip speed above zero", who);
  if (fr->reserved != 0.0) return fail(FB_EINVAL, "%s: reserved must be zero", who);
  return FB_OK;
}

// The classes, maxima and the sum of (-f) of one direction, in record order.  recs and side run in parallel; a record with d == 0 is
// degenerate and belongs to no class.
void friction_sums(const std::vector<BodyContactRec>& recs, const std::vector<ContactFrictionRec>& side, const fb_fem_contact_friction_params& fr, int dir,
                   fb_fem_contact_friction_info& I) {
  for (size_t i = 0; i < recs.size() && i < side.size(); i++) {
    if (!(recs[i].d > 0.0)) continue;
    const ContactFrictionRec& o = side[i];
    if (o.N == 0.0) I.n_separating[dir]++;
    else if (o.s < fr.slip_speed) I.n_sticking[dir]++;
    else I.n_sliding[dir]++;
    I.max_slip_speed = std::max(I.max_slip_speed, o.s);
    I.max_normal_force = std::max(I.max_normal_force, o.N);
    if (fr.slip_speed > 0.0) I.max_stick_rate = std::max(I.max_stick_rate, fr.mu * o.N / fr.slip_speed);
    for (int k = 0; k < 3; k++) I.friction_on_points[dir][k] += o.mf[k];
  }
}

// what the two read calls hand back
void read_friction(const std::vector<ContactFrictionRec>& v, double* normal_force, double* slip3, double* friction3) {
  for (size_t i = 0; i < v.size(); i++) {
    if (normal_force) normal_force[i] = v[i].N;
    for (int k = 0; k < 3; k++) {
      if (slip3) slip3[3 * i + k] = v[i].t[k];
      if (friction3) friction3[3 * i + k] = v[i].mf[k];
    }
  }
}

}  // namespace
}  // namespace fb
