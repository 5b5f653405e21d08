// Penalty contact of a rigid tool with the tissue (tool_contact.h), hand-written for gfx950.
//
// The rule is the header's (include/fembrain_hip.h, "Contact with a rigid tool"): every point -- a surface vertex, or any node -- that a
// sphere, capsule or oriented box of the tool holds is pushed out along that shape's normal, of several shapes the deepest, and the
// host sums what the tissue returns to the tool.  Two kernels, a selection between them, and two host waits (the count, the records):
//  - points: a thread per point, p = x0 + q against every shape.  The tool travels in the kernel arguments (fb_tool by value, 2.5 KB):
//    it is the same for every lane, so the loop over the shapes reads it through the scalar unit and no lane holds a copy.  The thread
//    writes a flag and a dense record (point, winning shape, depth, normal), and raises a word where a position -- with friction, a
//    velocity -- of a point is not finite.  Nothing is culled: sixteen shapes cost a point less than the position it loads;
//  - one rocPRIM select over the flags gives the contacts by ascending point; one host wait brings their number and the two words, and
//    a call that finds a word raised ends there, the force vector untouched;
//  - forces: a thread per contact, the header's step 4 -- under friction the tail of the law of contact_friction.hip.h written again
//    with the tool's velocity at the point in place of a face's -- added in place (the points are distinct nodes: no atomics, no sort),
//    and the compact records, which one copy brings back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "contact_friction.hip.h"
#include "device_prims.hip.h"
#include "fem_handle.h"
#include "launch.hip.h"

namespace fb {
namespace {

__device__ __forceinline__ double dot3(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// the sphere (c, r) against p: held, and then depth, normal and whether the point sits on c
__device__ __forceinline__ bool sphere_holds(const double* p, const double* c, double r, double& depth, double* n, bool& degenerate) {
  const double u[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const double l2 = dot3(u, u);
  if (!(l2 <= r * r)) return false;
  const double l = sqrt(l2);
  degenerate = l == 0.0;
  depth = degenerate ? r : r - l;
#pragma unroll
  for (int k = 0; k < 3; k++) n[k] = degenerate ? 0.0 : u[k] / l;
  return true;
}

__device__ __forceinline__ bool shape_holds(const fb_tool_shape& S, const double* p, double& depth, double* n, bool& degenerate) {
  if (S.kind == FB_TOOL_BOX) {
    const double u[3] = {p[0] - S.a[0], p[1] - S.a[1], p[2] - S.a[2]};
    double l[3];
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      l[i] = dot3(S.R + 3 * i, u);
      in = in && fabs(l[i]) <= S.size[i];
    }
    if (!in) return false;
    int axis = 0;
    double e = S.size[0] - fabs(l[0]);
#pragma unroll
    for (int i = 1; i < 3; i++) {
      const double ei = S.size[i] - fabs(l[i]);
      if (ei < e) { e = ei; axis = i; }
    }
    depth = e;
    degenerate = false;
#pragma unroll
    for (int k = 0; k < 3; k++) n[k] = l[axis] < 0.0 ? -S.R[3 * axis + k] : S.R[3 * axis + k];
    return true;
  }
  if (S.kind == FB_TOOL_CAPSULE) {
    const double d[3] = {S.b[0] - S.a[0], S.b[1] - S.a[1], S.b[2] - S.a[2]};
    const double dd = dot3(d, d);
    const double u[3] = {p[0] - S.a[0], p[1] - S.a[1], p[2] - S.a[2]};
    const double t = dd > 0.0 ? fmin(fmax(dot3(u, d) / dd, 0.0), 1.0) : 0.0;
    const double c[3] = {S.a[0] + t * d[0], S.a[1] + t * d[1], S.a[2] + t * d[2]};
    return sphere_holds(p, c, S.size[0], depth, n, degenerate);
  }
  return sphere_holds(p, S.a, S.size[0], depth, n, degenerate);
}

// A thread per point.  ids: the caller id of every point (null: the point's index); internal: its internal id (null: the caller id).
// qvel: null without friction.  bad[0] / bad[1]: a position / a velocity of a point is not finite (every writer stores the same value).
__global__ __launch_bounds__(kB) void k_tool_points(int n_points, int n_nodes, const int* __restrict__ ids, const int* __restrict__ internal, const double* __restrict__ x0,
                                                    const double* __restrict__ q, const double* __restrict__ qvel, const fb_tool T, ToolContactRec* __restrict__ dense,
                                                    unsigned char* __restrict__ flag, int* __restrict__ bad) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_points) return;
  const int node = ids ? ids[i] : i;
  const int nd = internal ? internal[i] : node;
  if ((unsigned)nd >= (unsigned)n_nodes) {  // (a vertex without a node: nothing holds it)
    flag[i] = 0;
    return;
  }
  double p[3];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    p[k] = x0[3 * (size_t)nd + k] + q[3 * (size_t)nd + k];
    finite = finite && fabs(p[k]) <= DBL_MAX;
  }
  if (!finite) bad[0] = 1;
  if (qvel) {
    bool vfinite = true;
#pragma unroll
    for (int k = 0; k < 3; k++) vfinite = vfinite && fabs(qvel[3 * (size_t)nd + k]) <= DBL_MAX;
    if (!vfinite) bad[1] = 1;
  }
  ToolContactRec r;
  r.depth = 0.0;
  r.shape = -1;
  r.degenerate = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) { r.p[k] = p[k]; r.n[k] = 0.0; r.f[k] = 0.0; }
  const int ns = min(max(T.n_shapes, 0), FB_TOOL_MAX_SHAPES);
  for (int s = 0; s < ns; s++) {
    double depth, n[3];
    bool degenerate;
    if (!shape_holds(T.shapes[s], p, depth, n, degenerate)) continue;
    if (r.shape >= 0 && !(depth > r.depth)) continue;  // (the deepest; of equal depths the first)
    r.shape = s;
    r.depth = depth;
    r.degenerate = degenerate ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 3; k++) r.n[k] = n[k];
  }
  r.node = node;
  r.nd = nd;
  flag[i] = r.shape >= 0 ? 1 : 0;
  if (r.shape >= 0) dense[i] = r;
}

// origin, velocity and angular velocity of the tool, as the force kernel takes them
struct ToolFrame {
  double origin[3], velocity[3], omega[3];
};

// A thread per contact: F, its addition to the point's node, the compact record.  Under friction side[t] holds N, |t|, t, -f.
template <bool kFriction>
__global__ __launch_bounds__(kB) void k_tool_force(int n_contacts, int n_points, int n_nodes, const int* __restrict__ hit, const ToolContactRec* __restrict__ dense, double stiffness,
                                                   double depth_cap, FrictionLaw L, ToolFrame T, const double* __restrict__ qvel, ToolContactRec* __restrict__ rec,
                                                   ContactFrictionRec* __restrict__ side, double* __restrict__ fext) {
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= n_contacts) return;
  const int i = hit[t];
  ToolContactRec r;
  memset(&r, 0, sizeof(r));
  r.node = -1; r.nd = -1; r.shape = -1; r.degenerate = 1;
  if ((unsigned)i < (unsigned)n_points) r = dense[i];
  ContactFrictionRec o = {0.0, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  const bool push = !r.degenerate && (unsigned)r.nd < (unsigned)n_nodes;
  if (push) {
    const double depth = depth_cap > 0.0 ? fmin(r.depth, depth_cap) : r.depth;
    const double sd = stiffness * depth;
    double F[3];
    if constexpr (kFriction) {
      const double a[3] = {r.p[0] - T.origin[0], r.p[1] - T.origin[1], r.p[2] - T.origin[2]};
      const double vt[3] = {T.velocity[0] + (T.omega[1] * a[2] - T.omega[2] * a[1]), T.velocity[1] + (T.omega[2] * a[0] - T.omega[0] * a[2]),
                            T.velocity[2] + (T.omega[0] * a[1] - T.omega[1] * a[0])};
      double w[3];
#pragma unroll
      for (int k = 0; k < 3; k++) w[k] = qvel[3 * (size_t)r.nd + k] - vt[k];
      // the law's lines vn ... F_k (contact_friction_law), with the shape's n and this sd
      const double vn = (w[0] * r.n[0] + w[1] * r.n[1]) + w[2] * r.n[2];
      double N = sd - L.damping * vn;
      if (!(N > 0.0)) N = 0.0;  // no adhesion
      double tv[3];
#pragma unroll
      for (int k = 0; k < 3; k++) tv[k] = w[k] - vn * r.n[k];
      const double s = sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2]);
      const double den = fmax(s, L.slip_speed);
      const double g = den > 0.0 ? (L.mu * N) / den : 0.0;
      o.N = N;
      o.s = s;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double f = g * tv[k];
        F[k] = N * r.n[k] - f;
        o.t[k] = tv[k];
        o.mf[k] = -f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) F[k] = sd * r.n[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      fext[3 * (size_t)r.nd + k] += F[k];
      r.f[k] = F[k];
    }
  }
  rec[t] = r;
  if constexpr (kFriction) side[t] = o;
}

// ---- host ----

bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// everything the header refuses before a launch
int check_tool(fb_fem_s* h, const fb_tool* tool, const fb_fem_tool_contact_params* p, const fb_fem_contact_friction_params* fr) {
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_tool_contact is for unsharded handles");
  if (!tool || !p) return fail(FB_EINVAL, "fb_fem_tool_contact: null tool or parameters");
  if (tool->n_shapes < 1 || tool->n_shapes > FB_TOOL_MAX_SHAPES) return fail(FB_EINVAL, "fb_fem_tool_contact: %d shapes (1 .. %d)", tool->n_shapes, FB_TOOL_MAX_SHAPES);
  if (tool->reserved != 0 || p->reserved != 0) return fail(FB_EINVAL, "fb_fem_tool_contact: reserved must be zero");
  if (p->points != FB_TOOL_SURFACE_VERTICES && p->points != FB_TOOL_ALL_NODES) return fail(FB_EINVAL, "fb_fem_tool_contact: points %d", p->points);
  FB_TRY(check_penalty("tool contact", p->stiffness, p->depth_cap));
  if (!finite3(tool->origin) || !finite3(tool->velocity) || !finite3(tool->omega)) return fail(FB_EINVAL, "fb_fem_tool_contact: origin, velocity or omega is not finite");
  for (int s = 0; s < tool->n_shapes; s++) {
    const fb_tool_shape& S = tool->shapes[s];
    if (S.kind != FB_TOOL_SPHERE && S.kind != FB_TOOL_CAPSULE && S.kind != FB_TOOL_BOX) return fail(FB_EINVAL, "fb_fem_tool_contact: shape %d of kind %d", s, S.kind);
    if (S.reserved != 0) return fail(FB_EINVAL, "fb_fem_tool_contact: shape %d: reserved must be zero", s);
    const int n_size = S.kind == FB_TOOL_BOX ? 3 : 1;
    for (int k = 0; k < n_size; k++)
      if (!std::isfinite(S.size[k]) || S.size[k] < 0.0) return fail(FB_EINVAL, "fb_fem_tool_contact: shape %d: radius or half extent %g", s, S.size[k]);
    if (!finite3(S.a) || (S.kind == FB_TOOL_CAPSULE && !finite3(S.b))) return fail(FB_EINVAL, "fb_fem_tool_contact: shape %d: a point is not finite", s);
    if (S.kind == FB_TOOL_BOX) {
      for (int i = 0; i < 3; i++)
        if (!finite3(S.R + 3 * i)) return fail(FB_EINVAL, "fb_fem_tool_contact: shape %d: R is not finite", s);
      for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++) {
          const double d = (S.R[3 * i] * S.R[3 * j] + S.R[3 * i + 1] * S.R[3 * j + 1]) + S.R[3 * i + 2] * S.R[3 * j + 2];
          if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-9)) return fail(FB_EINVAL, "fb_fem_tool_contact: shape %d: the rows of R are not orthonormal", s);
        }
    }
  }
  if (fr) FB_TRY(check_friction(fr, "fb_fem_tool_contact"));
  if (h->plan.n_global <= 0) return fail(FB_EINVAL, "fb_fem_tool_contact: %d nodes", h->plan.n_global);
  return FB_OK;
}

// one stage of fb_fem_time_tool_contact between two events (seconds null: not timing)
struct ToolStages {
  hipEvent_t* ev;
  hipStream_t s;
  double* seconds;
  int begin() {
    if (seconds) FB_HIP(hipEventRecord(ev[0], s));
    return FB_OK;
  }
  int end(int stage) {
    if (!seconds) return FB_OK;
    FB_HIP(hipEventRecord(ev[1], s));
    FB_HIP(hipEventSynchronize(ev[1]));
    float ms = 0;
    FB_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    seconds[stage] += ms * 1e-3;
    return FB_OK;
  }
};

// The header's step 5 on the host, in record order.  side: empty for a frictionless call.
void tool_sums(const std::vector<ToolContactRec>& recs, const std::vector<ContactFrictionRec>& side, const fb_tool& tool, const fb_fem_tool_contact_params& prm,
               const fb_fem_contact_friction_params* fr, fb_fem_tool_contact_info& I) {
  for (size_t i = 0; i < recs.size(); i++) {
    const ToolContactRec& r = recs[i];
    I.n_contacts++;
    if ((unsigned)r.shape < (unsigned)FB_TOOL_MAX_SHAPES) I.contacts_by_shape[r.shape]++;
    if (r.degenerate) { I.n_degenerate++; continue; }
    const double depth = prm.depth_cap > 0.0 ? std::min(r.depth, prm.depth_cap) : r.depth;
    I.max_depth = std::max(I.max_depth, depth);
    const double a[3] = {r.p[0] - tool.origin[0], r.p[1] - tool.origin[1], r.p[2] - tool.origin[2]};
    const double m[3] = {-r.f[0], -r.f[1], -r.f[2]};
    for (int k = 0; k < 3; k++) { I.force_on_body[k] += r.f[k]; I.force_on_tool[k] += m[k]; }
    I.torque_on_tool[0] += a[1] * m[2] - a[2] * m[1];
    I.torque_on_tool[1] += a[2] * m[0] - a[0] * m[2];
    I.torque_on_tool[2] += a[0] * m[1] - a[1] * m[0];
    if (fr && i < side.size()) {
      const ContactFrictionRec& o = side[i];
      if (o.N == 0.0) I.n_separating++;
      else if (o.s < fr->slip_speed) I.n_sticking++;
      else I.n_sliding++;
      I.max_slip_speed = std::max(I.max_slip_speed, o.s);
      I.max_normal_force = std::max(I.max_normal_force, o.N);
      if (fr->slip_speed > 0.0) I.max_stick_rate = std::max(I.max_stick_rate, fr->mu * o.N / fr->slip_speed);
    }
  }
}

// add: into the external force vector, the records kept for fb_fem_read_tool_contact; else into scratch, nothing kept (seconds: the stages)
int tool_contact(fb_fem_s* h, const fb_tool& tool, const fb_fem_tool_contact_params& prm, const fb_fem_contact_friction_params* fr, bool add, double* seconds,
                 fb_fem_tool_contact_info* out) {
  ToolContactWork& W = h->toolc;
  PlanWorkspace& ws = h->plan_ws;
  hipStream_t s = h->stream;
  fb_fem_tool_contact_info I;
  memset(&I, 0, sizeof(I));
  const int n_nodes = h->plan.n_global;
  int n_points = n_nodes;
  const int *ids = nullptr, *internal = h->ren.active ? h->ren.d_new_of_old.p : nullptr;
  if (prm.points == FB_TOOL_SURFACE_VERTICES) {
    FB_TRY(surface_current(h));  // the surface belongs to the current mesh
    n_points = h->surf.n_vertices;
    ids = h->surf.vertex_ids.p;
    internal = h->surf.vnode.p;
  }
  I.n_points = n_points;
  if (seconds)  // (only the timing call has stages to time)
    for (auto& e : W.ev_t)
      if (!e) FB_HIP(hipEventCreate(&e));
  ToolStages tm = {W.ev_t, s, seconds};
  std::vector<ToolContactRec> recs;
  std::vector<ContactFrictionRec> side;
  int got[3] = {0, 0, 0};

  if (n_points > 0) {
    // ---- points against shapes ----
    FB_TRY(tm.begin());
    FB_TRY(W.dense.reserve((size_t)n_points)); FB_TRY(W.flag.reserve((size_t)n_points)); FB_TRY(W.hit.reserve((size_t)n_points)); FB_TRY(W.counts.reserve(3));
    FB_HIP(hipMemsetAsync(W.counts.p, 0, sizeof(int) * 3, s));
    FB_TRY(launch_1d(k_tool_points, n_points, s, n_points, n_nodes, ids, internal, h->x0.p, h->q.p, fr ? h->qvel.p : nullptr, tool, W.dense.p, W.flag.p, W.counts.p + 1));
    FB_TRY(tm.end(0));

    // ---- the contacts by ascending point; their number and the two words ----
    FB_TRY(tm.begin());
    FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.hit.p, W.counts.p, (size_t)n_points));
    FB_TRY(W.counts.download(got, 3, s));  // a host wait
    FB_TRY(tm.end(1));
    if (got[1]) return fail(FB_EINVAL, "fb_fem_tool_contact: a position of a point is not finite");
    if (got[2]) return fail(FB_EINVAL, "fb_fem_tool_contact: a velocity of a point is not finite");
    if (got[0] < 0 || got[0] > n_points) return fail(FB_EDEVICE, "tool contact: %d contacts of %d points", got[0], n_points);
  }
  const int n_found = got[0];

  if (n_found > 0) {
    // ---- forces, and the records back ----
    double* fext = h->fext.p;
    if (!add) {  // (outside the stage: the adding call has no such fill)
      FB_TRY(W.scratch.reserve((size_t)3 * n_nodes));
      FB_TRY(W.scratch.zero(s));
      fext = W.scratch.p;
    }
    FB_TRY(tm.begin());
    FB_TRY(W.rec.reserve((size_t)n_found));
    ToolFrame frame;
    memcpy(frame.origin, tool.origin, sizeof(frame.origin)); memcpy(frame.velocity, tool.velocity, sizeof(frame.velocity)); memcpy(frame.omega, tool.omega, sizeof(frame.omega));
    recs.resize((size_t)n_found);
    if (fr) {
      const FrictionLaw law = {fr->mu, fr->slip_speed, fr->damping};
      FB_TRY(W.fric.reserve((size_t)n_found));
      FB_TRY(launch_1d(k_tool_force<true>, n_found, s, n_found, n_points, n_nodes, W.hit.p, W.dense.p, prm.stiffness, prm.depth_cap, law, frame, h->qvel.p, W.rec.p, W.fric.p, fext));
      side.resize((size_t)n_found);
      FB_HIP(hipMemcpyAsync(side.data(), W.fric.p, sizeof(ContactFrictionRec) * (size_t)n_found, hipMemcpyDeviceToHost, s));  // (the wait below covers it)
    } else {
      FB_TRY(launch_1d(k_tool_force<false>, n_found, s, n_found, n_points, n_nodes, W.hit.p, W.dense.p, prm.stiffness, prm.depth_cap, FrictionLaw{0.0, 0.0, 0.0}, frame, nullptr, W.rec.p,
                       nullptr, fext));
    }
    FB_TRY(W.rec.download(recs.data(), (size_t)n_found, s));  // a host wait
    FB_TRY(tm.end(2));
  }

  tool_sums(recs, side, tool, prm, fr, I);
  if (add) {
    W.host.swap(recs);
    W.fric_host.swap(side);
  }
  if (out) *out = I;
  return FB_OK;
}

}  // namespace
}  // namespace fb

// ---- the C ABI ----

int fb_fem_tool_contact(fb_fem_t h, const fb_tool* tool, const fb_fem_tool_contact_params* p, const fb_fem_contact_friction_params* fr, fb_fem_tool_contact_info* out) {
  CHECK_HANDLE(h);
  FB_TRY(check_tool(h, tool, p, fr));
  return tool_contact(h, *tool, *p, fr, true, nullptr, out);
}

int fb_fem_num_tool_contacts(fb_fem_t h) {
  CHECK_HANDLE(h);
  return (int)h->toolc.host.size();
}

int fb_fem_read_tool_contact(fb_fem_t h, int* node, int* shape, double* depth, double* normal3, double* force3, double* normal_force, double* slip3, double* friction3) {
  CHECK_HANDLE(h);
  const std::vector<ToolContactRec>& v = h->toolc.host;
  const std::vector<ContactFrictionRec>& f = h->toolc.fric_host;
  for (size_t i = 0; i < v.size(); i++) {
    const ToolContactRec& r = v[i];
    const bool fric = i < f.size();
    if (node) node[i] = r.node;
    if (shape) shape[i] = r.shape;
    if (depth) depth[i] = r.depth;
    if (normal_force) normal_force[i] = fric ? f[i].N : 0.0;
    for (int k = 0; k < 3; k++) {
      if (normal3) normal3[3 * i + k] = r.n[k];
      if (force3) force3[3 * i + k] = r.f[k];
      if (slip3) slip3[3 * i + k] = fric ? f[i].t[k] : 0.0;
      if (friction3) friction3[3 * i + k] = fric ? f[i].mf[k] : 0.0;
    }
  }
  return FB_OK;
}

int fb_fem_time_tool_contact(fb_fem_t h, const fb_tool* tool, const fb_fem_tool_contact_params* p, const fb_fem_contact_friction_params* fr, int reps, double seconds[3]) {
  CHECK_HANDLE(h);
  FB_TRY(check_tool(h, tool, p, fr));
  if (reps < 1 || !seconds) return fail(FB_EINVAL, "fb_fem_time_tool_contact: reps must be positive and seconds not null");
  FB_TRY(tool_contact(h, *tool, *p, fr, false, nullptr, nullptr));  // warm: the buffers exist, the surface is current
  double sum[3] = {0, 0, 0};
  for (int r = 0; r < reps; r++) FB_TRY(tool_contact(h, *tool, *p, fr, false, sum, nullptr));
  for (int k = 0; k < 3; k++) seconds[k] = sum[k] / reps;
  return FB_OK;
}
