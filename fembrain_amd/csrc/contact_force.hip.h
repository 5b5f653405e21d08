// The force stage of the two contact units (body_contact.hip, self_contact.hip), written once: from the records a search left
// (face_search.hip.h) the force of every contact, frictionless or under the law of contact_friction.hip.h, the records of the nodes it
// acts on, their stable sort by node and the scatter that adds a node's segment in record order.  No floating-point atomics.
// kRecs, the records per contact, is what tells the units apart:
//  3  two bodies: the point's node belongs to P, where the contacts of a direction are different nodes, so its +F is added in place;
//     the three corners of the face in T are the records (node, 3 contact + corner);
//  4  one body: a node can be pushed as a point and push back as a corner in one call, so all four contributions are records
//     (node, 4 contact + r), r = 0 the point's +F, r = 1..3 the corners' (-F) b_k.
// Friction is a compile-time choice: the frictionless kernels never read a velocity.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "contact_friction.hip.h"
#include "face_search.hip.h"

namespace fb {
namespace {

// A thread per contact: F, its addition to the point's own node (kRecs == 3) and the records.  Under friction F is the law's total --
// normal force with damping, minus the friction -- from the velocities of the point's node and of the face's corners, read from the
// handles' own qvel arrays (internal order, as the positions), and side[t] holds N, |t|, t, -f: zero for a contact that pushes nothing.
template <int kRecs, bool kFriction>
__global__ __launch_bounds__(kB) void k_contact_force(SearchDev S, double stiffness, double depth_cap, FrictionLaw law, const double* __restrict__ qvel_p,
                                                      const double* __restrict__ qvel_t, BodyContactRec* __restrict__ rec, ContactFrictionRec* __restrict__ side,
                                                      double* __restrict__ fext_p, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  static_assert(kRecs == 3 || kRecs == 4, "the corners of the face, and the point's node where it is a record");
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= S.n_contacts) return;
  double p[3] = {0.0, 0.0, 0.0};
  const int vr = contact_point(S, t, p);
  const BodyContactRec r = rec[t];
  const bool push = vr >= 0 && (unsigned)r.face < (unsigned)S.nf && r.d > 0.0;
  ContactFrictionRec o = {0.0, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (push) {
    const int nd = S.vnode[vr];
    double F[3];
    if constexpr (kFriction) {
      double vp[3], vt[3][3];
      node_velocity(qvel_p, S.n_nodes_p, nd, vp);
#pragma unroll
      for (int k = 0; k < 3; k++) node_velocity(qvel_t, S.n_nodes_t, S.faces_int[3 * (size_t)r.face + k], vt[k]);
      contact_friction_law(p, r.c, r.b, r.d, stiffness, depth_cap, law, vp, vt, F, o);
    } else {
      const double depth = depth_cap > 0.0 ? fmin(r.d, depth_cap) : r.d;
      const double sd = stiffness * depth;
#pragma unroll
      for (int k = 0; k < 3; k++) F[k] = sd * ((r.c[k] - p[k]) / r.d);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if constexpr (kRecs == 3) fext_p[3 * (size_t)nd + k] += F[k];
      rec[t].f[k] = F[k];
    }
  } else {
    rec[t].d = 0.0;  // (nothing is pushed: degenerate, or no face left)
  }
  if constexpr (kFriction) side[t] = o;
#pragma unroll
  for (int k = 0; k < kRecs; k++) {
    const int corner = k - (kRecs - 3);  // (-1: the point)
    int nd = !push ? S.n_nodes_t : corner < 0 ? S.vnode[vr] : S.faces_int[3 * (size_t)r.face + corner];
    if ((unsigned)nd >= (unsigned)S.n_nodes_t) nd = S.n_nodes_t;  // (no node: sorted behind every node, and skipped)
    keys[kRecs * (size_t)t + k] = (uint32_t)nd;
    vals[kRecs * (size_t)t + k] = (uint32_t)(kRecs * t + k);
  }
}

// A thread per sorted record: the first of a node's segment does that node's additions in record order, however many they are
template <int kRecs>
__global__ __launch_bounds__(kB) void k_contact_segments(int n_rec, const uint32_t* __restrict__ keys_s, const uint32_t* __restrict__ vals_s, int n_contacts, int n_nodes,
                                                         const BodyContactRec* __restrict__ rec, double* __restrict__ fext) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_rec) return;
  const uint32_t node = keys_s[i];
  if (node >= (uint32_t)n_nodes || (i > 0 && keys_s[i - 1] == node)) return;
  double a[3] = {fext[3 * (size_t)node], fext[3 * (size_t)node + 1], fext[3 * (size_t)node + 2]};
  for (int k = i; k < n_rec && keys_s[k] == node; k++) {
    const uint32_t v = vals_s[k];
    const uint32_t t = v / (uint32_t)kRecs, which = v % (uint32_t)kRecs;
    if (t >= (uint32_t)n_contacts) continue;
    const BodyContactRec& r = rec[t];
    if (!(r.d > 0.0)) continue;
    if (kRecs == 4 && which == 0) {
      a[0] += r.f[0]; a[1] += r.f[1]; a[2] += r.f[2];
    } else {
      const double w = r.b[which - (kRecs - 3)];
      a[0] += (-r.f[0]) * w; a[1] += (-r.f[1]) * w; a[2] += (-r.f[2]) * w;
    }
  }
  fext[3 * (size_t)node] = a[0]; fext[3 * (size_t)node + 1] = a[1]; fext[3 * (size_t)node + 2] = a[2];
}

// ---- host ----

// The force stage of S's contacts: forces, records, sort, scatter into fext_t (and, kRecs == 3, in place into fext_p), and the records
// back on the host.  law: null for the frictionless rule; else the friction call's, its side records into side_out.
template <int kRecs>
int contact_forces(hipStream_t s, PlanWorkspace& ws, FaceSearchWork& F, const SearchDev& S, double stiffness, double depth_cap, const FrictionLaw* law, const double* qvel_p,
                   const double* qvel_t, double* fext_p, double* fext_t, std::vector<BodyContactRec>& out, std::vector<ContactFrictionRec>* side_out) {
  const int n = S.n_contacts;
  const size_t n_rec = (size_t)kRecs * n;
  FB_TRY(F.r_key.reserve(n_rec)); FB_TRY(F.r_key_s.reserve(n_rec)); FB_TRY(F.r_val.reserve(n_rec)); FB_TRY(F.r_val_s.reserve(n_rec));
  if (law) {
    FB_TRY(F.fric.reserve((size_t)n));
    FB_TRY(launch_1d(k_contact_force<kRecs, true>, n, s, S, stiffness, depth_cap, *law, qvel_p, qvel_t, F.rec.p, F.fric.p, fext_p, F.r_key.p, F.r_val.p));
  } else {
    FB_TRY(launch_1d(k_contact_force<kRecs, false>, n, s, S, stiffness, depth_cap, FrictionLaw{0.0, 0.0, 0.0}, nullptr, nullptr, F.rec.p, nullptr, fext_p, F.r_key.p, F.r_val.p));
  }
  FB_TRY(sort_pairs(ws.temp, s, F.r_key.p, F.r_key_s.p, F.r_val.p, F.r_val_s.p, n_rec, (unsigned)bits_of((long long)S.n_nodes_t + 1)));
  FB_TRY(launch_1d(k_contact_segments<kRecs>, (long long)n_rec, s, (int)n_rec, F.r_key_s.p, F.r_val_s.p, n, S.n_nodes_t, F.rec.p, fext_t));
  out.resize((size_t)n);
  if (law && side_out) {
    side_out->resize((size_t)n);
    FB_HIP(hipMemcpyAsync(side_out->data(), F.fric.p, sizeof(ContactFrictionRec) * (size_t)n, hipMemcpyDeviceToHost, s));  // (the wait below covers it)
  }
  return F.rec.download(out.data(), (size_t)n, s);  // a host wait
}

// What the info structs sum over the records of one direction, in record order, onto the values S came with (the second direction of
// two bodies goes on where the first ended: the order of the additions is the rule's).  keep(i, r): false for a record the caller drops
// (its tested faces still count).  The sums are formed in a local and handed back by value: accumulated through pointers into the
// caller's info struct, the same loop measured slower on the host.
struct ContactSums {
  long long faces_tested = 0;
  int n_degenerate = 0;
  double max_depth = 0.0, on_points[3] = {0.0, 0.0, 0.0}, on_faces[3] = {0.0, 0.0, 0.0};
};
template <class Keep>
ContactSums contact_sums(const std::vector<BodyContactRec>& recs, double depth_cap, ContactSums S, Keep keep) {
  for (size_t i = 0; i < recs.size(); i++) {
    const BodyContactRec& r = recs[i];
    S.faces_tested += r.tested;
    if (!keep(i, r)) continue;
    if (!(r.d > 0.0)) { S.n_degenerate++; continue; }
    const double depth = depth_cap > 0.0 ? std::min(r.d, depth_cap) : r.d;
    S.max_depth = std::max(S.max_depth, depth);
    for (int k = 0; k < 3; k++) S.on_points[k] += r.f[k];
    for (int c = 0; c < 3; c++)
      for (int k = 0; k < 3; k++) S.on_faces[k] += (-r.f[k]) * r.b[c];
  }
  return S;
}

// what fb_fem_read_body_contact / fb_fem_read_self_contact hand back
void read_contacts(const std::vector<BodyContactRec>& v, int* node, int* element, int* face, double* closest_xyz, double* bary3, double* depth) {
  for (size_t i = 0; i < v.size(); i++) {
    const BodyContactRec& r = v[i];
    if (node) node[i] = r.node;
    if (element) element[i] = r.elem;
    if (face) face[i] = r.face;
    if (closest_xyz) memcpy(closest_xyz + 3 * i, r.c, sizeof(double) * 3);
    if (bary3) memcpy(bary3 + 3 * i, r.b, sizeof(double) * 3);
    if (depth) depth[i] = r.d;
  }
}

}  // namespace
}  // namespace fb
