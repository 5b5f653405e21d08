// Constrained DOFs that move: fb_fem_set_constrained_motion / fb_fem_read_constrained_motion / fb_fem_read_reactions / fb_fem_motion_info_get /
// fb_fem_time_motion, and the grasp on top of them (fb_fem_grasp / fb_fem_grasp_move / fb_fem_release).  The rule is "Constrained motion"
// in include/fembrain_hip.h; the reference has only the flag of IAvatar::grip() (IScalpel.cpp:42-44, AvatarRing.cpp:177).
//
// The stored matrix has the columns of the constrained DOFs zeroed, so what the free rows need of them -- Keff_fc dv_c -- is formed from
// the elements: every element with a node that has a DOF in the set ("listed") multiplies its s_k K_e + s_m M_e, in the closed form the
// assembly sums (k0_apply over the rotated gradients of the step record, the symmetric part of kcorr under warp = 2, rho/20 V (1 + delta_ij)),
// with the 12-vector that holds dv_c at the moved DOFs.  The 4 x 3 results go to scratch, record 4p + k for corner k of listed element p,
// and a thread per touched node adds its records in record order (a table sorted stably by node, built once per set and mesh
// generation): no floating-point atomics, two calls give the same bits.  The reaction pass runs the same two kernels with the full dv
// and the velocities and keeps the rows of the set.
//
// A node's run is walked by ONE thread in a loop, however long it is (a hub of a tet mesh reaches hundreds of records): the touched
// nodes are a few thousand at most, the records 12 doubles each, and the per-step cost is the element kernel's.  A wavefront per long
// run would add a second kernel and a second summation order for no measured gain.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <iterator>
#include <vector>

#include "device_prims.hip.h"
#include "fem_handle.h"
#include "launch.hip.h"
#include "motion.h"
#include "tet_math.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

// ---- the table ----

// the set's caller ids -> internal DOFs, and the set's entry at each of them
__global__ __launch_bounds__(kB) void k_motion_map(int n, const int* __restrict__ dofs_caller, const int* __restrict__ new_of_old, int n_nodes, int* __restrict__ dof,
                                                   int* __restrict__ dof_slot) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  const int c = dofs_caller[i], node = c / 3;
  if ((unsigned)node >= (unsigned)n_nodes) { dof[i] = -1; return; }  // (checked on the host; never out of the arrays)
  const int in = new_of_old ? new_of_old[node] : node;
  if ((unsigned)in >= (unsigned)n_nodes) { dof[i] = -1; return; }
  const int d = 3 * in + (c - 3 * node);
  dof[i] = d;
  dof_slot[d] = i;
}

// element e is listed: one of its nodes has a DOF in the set
__global__ __launch_bounds__(kB) void k_motion_flag(int nt, const int4* __restrict__ tets, int n_nodes, const int* __restrict__ dof_slot, unsigned char* __restrict__ flag) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= nt) return;
  const int4 t = tets[e];
  const int id[4] = {t.x, t.y, t.z, t.w};
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if ((unsigned)id[k] >= (unsigned)n_nodes) continue;
#pragma unroll
    for (int a = 0; a < 3; a++) any = any || dof_slot[3 * (size_t)id[k] + a] >= 0;
  }
  flag[e] = any ? 1 : 0;
}

// record r = 4p + k, corner k of listed element p: its node as the sort key, and the set's entries at its three DOFs
__global__ __launch_bounds__(kB) void k_motion_corners(int n_rec, const int* __restrict__ listed, const int4* __restrict__ tets, int n_nodes,
                                                       const int* __restrict__ dof_slot, uint32_t* __restrict__ key, uint32_t* __restrict__ val, int* __restrict__ esel) {
  const int r = blockIdx.x * kB + threadIdx.x;
  if (r >= n_rec) return;
  const int4 t = tets[listed[r >> 2]];
  const int k = r & 3;
  const int node = k == 0 ? t.x : k == 1 ? t.y : k == 2 ? t.z : t.w;
  const bool ok = (unsigned)node < (unsigned)n_nodes;
  key[r] = ok ? (uint32_t)node : (uint32_t)n_nodes;  // (no such node: sorted behind every node, and skipped)
  val[r] = (uint32_t)r;
#pragma unroll
  for (int a = 0; a < 3; a++) esel[3 * (size_t)r + a] = ok ? dof_slot[3 * (size_t)node + a] : -1;
}

// sorted record i opens a node's run; the longest run
__global__ __launch_bounds__(kB) void k_motion_heads(int n_rec, const uint32_t* __restrict__ key_s, int n_nodes, unsigned char* __restrict__ flag, int* __restrict__ longest) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_rec) return;
  const uint32_t node = key_s[i];
  const bool head = node < (uint32_t)n_nodes && (i == 0 || key_s[i - 1] != node);
  flag[i] = head ? 1 : 0;
  if (!head) return;
  int len = 1;
  while (i + len < n_rec && key_s[i + len] == node) len++;
  atomicMax(longest, len);
}

// ---- the step ----

// v* = (u - q) / h and dv_c = v* - qvel at the set's DOFs.  A target or a state that is not finite writes nothing but the error word.
__global__ __launch_bounds__(kB) void k_motion_dv(int n, const int* __restrict__ dof, const double* __restrict__ target, const double* __restrict__ q,
                                                  const double* __restrict__ qvel, double h, double* __restrict__ vstar, double* __restrict__ dvc, int* __restrict__ err) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  const int d = dof[i];
  if (d < 0) { atomicOr(err, 2); vstar[i] = 0.0; dvc[i] = 0.0; return; }
  const double u = target[i];
  const double vs = (u - q[d]) / h, dv = vs - qvel[d];
  if (!isfinite(u) || !isfinite(vs) || !isfinite(dv)) { atomicOr(err, 1); vstar[i] = 0.0; dvc[i] = 0.0; return; }
  vstar[i] = vs;
  dvc[i] = dv;
}

struct MotionParams {
  double a_k, a_m;           // on dv:   the correction s_k, s_m; the reactions s_k / h, s_m / h
  double b_k, b_m;           // on qvel: the reactions g_k, g_m
  double lambda, mu, rho20;  // the handle's material (no element map)
  const double* mtab;        // the material table where the handle has a map (lambda | mu | rho/20), else null
  // the reactions only: rest records, rest positions and displacements, from which the rotated gradients are formed again in fp64
  const double *rest, *x0, *q;
  int linear;
};

// A thread per listed element p: y[4p + k] = (a_k K_e + a_m M_e) v_e (+ (b_k K_e + b_m M_e) qvel_e + f_e: REACT), K_e and M_e as the
// assembly forms them from the element's step record.  v_e: dv_c at the moved DOFs; elsewhere 0 (the correction) or x (REACT: the solve's
// dv, which is 0 on the constrained rows).
// The correction must be the columns of the STORED matrix, so it takes the rotated gradients and the volume from the step record, in
// the handle's storage type.  The reactions are an output, with nothing to be consistent with but the rule, and they are small
// differences of large terms (the free neighbours move with the held nodes): with fp32 records their error measured 2.4e-7 of the
// largest reaction on the 4^3 cube of the tests.  REACT therefore forms c_k = R b_k again in fp64 from the rest record and the positions,
// as k_tet_warp forms them before it rounds (the same polar_rotation), and reads the fp64 volume.
template <typename MT, bool REACT>
__global__ __launch_bounds__(kB) void k_motion_elements(int n_listed, const int* __restrict__ listed, const int* __restrict__ esel, const int4* __restrict__ tets,
                                                        int n_nodes, const MT* __restrict__ rec, const MT* __restrict__ kcorr, const double* __restrict__ fe,
                                                        MotionParams P, const double* __restrict__ dvc, const double* __restrict__ x,
                                                        const double* __restrict__ qvel, double* __restrict__ y) {
  const int p = blockIdx.x * kB + threadIdx.x;
  if (p >= n_listed) return;
  const int e = listed[p];
  const int4 t = tets[e];
  const int id[4] = {t.x, t.y, t.z, t.w};
  const MT* rc = rec + 16 * (size_t)e;
  double c[4][3];
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int a = 0; a < 3; a++) c[k][a] = (double)rc[4 * k + a];
  double V = (double)rc[3];  // (quarter 0 keeps V; quarter 1 carries the material id where the handle has a map)
  if (REACT && (unsigned)id[0] < (unsigned)n_nodes && (unsigned)id[1] < (unsigned)n_nodes && (unsigned)id[2] < (unsigned)n_nodes && (unsigned)id[3] < (unsigned)n_nodes) {
    const double* r = P.rest + 16 * (size_t)e;
    double b[4][3], X[4][3];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int d = 0; d < 3; d++) {
        b[k][d] = r[3 * k + d];
        X[k][d] = P.x0[3 * (size_t)id[k] + d] + P.q[3 * (size_t)id[k] + d];
      }
    V = r[12];
    double F[9], R[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) F[3 * i + j] = X[0][i] * b[0][j] + X[1][i] * b[1][j] + X[2][i] * b[2][j] + X[3][i] * b[3][j];
    if (P.linear) {
#pragma unroll
      for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else {
      const double det = polar_rotation(F, R, 1e-6);
      if (det < 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = -R[i];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int a = 0; a < 3; a++) c[k][a] = R[3 * a] * b[k][0] + R[3 * a + 1] * b[k][1] + R[3 * a + 2] * b[k][2];
  }
  double lambda = P.lambda, mu = P.mu, rho20 = P.rho20;
  if (P.mtab) {
    const int mid = rec_mat_id(rc[7]);
    lambda = P.mtab[mid]; mu = P.mtab[kMaxMaterials + mid]; rho20 = P.mtab[2 * kMaxMaterials + mid];
  }
  double vk[12], vm[12];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const bool ok = (unsigned)id[k] < (unsigned)n_nodes;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const int j = 3 * k + a, sel = esel[12 * (size_t)p + j];
      double v = 0.0, w = 0.0;
      if (sel >= 0) v = dvc[sel];
      else if (REACT && ok) v = x[3 * (size_t)id[k] + a];
      if (REACT && ok) w = qvel[3 * (size_t)id[k] + a];
      vk[j] = REACT ? P.a_k * v + P.b_k * w : P.a_k * v;
      vm[j] = REACT ? P.a_m * v + P.b_m * w : P.a_m * v;
    }
  }
  double out[12];
  k0_apply(c, V, lambda, mu, vk, out);
  if (kcorr) {  // warp = 2: the symmetric part of the rotation-derivative terms, as add_contribution takes it
    const MT* C = kcorr + 144 * (size_t)e;
    for (int r = 0; r < 12; r++) {
      double s = 0.0;
      for (int col = 0; col < 12; col++) s += 0.5 * ((double)C[12 * r + col] + (double)C[12 * col + r]) * vk[col];
      out[r] += s;
    }
  }
  const double mv = rho20 * V;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double all = (vm[a] + vm[3 + a]) + (vm[6 + a] + vm[9 + a]);
#pragma unroll
    for (int k = 0; k < 4; k++) out[3 * k + a] += mv * (all + vm[3 * k + a]);  // rho/20 V (1 + delta_ij)
  }
  if (REACT) {
    const double* f = fe + 12 * (size_t)e;
#pragma unroll
    for (int j = 0; j < 12; j++) out[j] += f[j];
  }
  double* yo = y + 12 * (size_t)p;
#pragma unroll
  for (int j = 0; j < 12; j++) yo[j] = out[j];
}

// A thread per touched node: its records in record order.  The correction is subtracted from the right-hand side on the node's FREE
// DOFs; REACT keeps the rows of the set: react[entry] = the sum - fext.
template <bool REACT>
__global__ __launch_bounds__(kB) void k_motion_gather(int n_touched, const int* __restrict__ heads, int n_rec, const uint32_t* __restrict__ key_s,
                                                      const uint32_t* __restrict__ val_s, const int* __restrict__ esel, const double* __restrict__ y,
                                                      const uint8_t* __restrict__ dofmask, const double* __restrict__ fext, double* __restrict__ out) {
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= n_touched) return;
  const int i0 = heads[t];
  if ((unsigned)i0 >= (unsigned)n_rec) return;
  const uint32_t node = key_s[i0];
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = i0; i < n_rec && key_s[i] == node; i++) {
    const uint32_t r = val_s[i];
    if (r >= (uint32_t)n_rec) continue;
    s[0] += y[3 * (size_t)r]; s[1] += y[3 * (size_t)r + 1]; s[2] += y[3 * (size_t)r + 2];
  }
  const uint32_t r0 = val_s[i0];
  if (r0 >= (uint32_t)n_rec) return;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const size_t d = 3 * (size_t)node + a;
    if (REACT) {
      const int sel = esel[3 * (size_t)r0 + a];  // (every record of the node holds the same three entries)
      if (sel >= 0) out[sel] = s[a] - fext[d];
    } else if (dofmask[d]) {
      out[d] -= s[a];
    }
  }
}

// Before the gather: an entry on a node that no element uses (what FB_DETACH_REMOVE leaves) has an empty row in the rule, lambda = -fext;
// every other entry is written by the gather
__global__ __launch_bounds__(kB) void k_motion_react_init(int n, const int* __restrict__ dof, const double* __restrict__ fext, double* __restrict__ react) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n + 3) return;
  const int d = i < n ? dof[i] : -1;
  react[i] = d >= 0 ? -fext[d] : 0.0;
}

// one workgroup: the reactions summed by axis in one fixed tree (thread t takes the entries t, t + 256, ... in that order)
__global__ __launch_bounds__(kB) void k_motion_sum3(int n, const int* __restrict__ dof, const double* __restrict__ react, double* __restrict__ sum3) {
  for (int a = 0; a < 3; a++) {
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += kB)
      if (dof[i] >= 0 && dof[i] % 3 == a) v += react[i];
    const double s = wg_sum(v);
    if (threadIdx.x == 0) sum3[a] = s;
  }
}

// q_c = u_c (the target's bits) and qvel_c = v*_c; nothing where k_motion_dv refused
__global__ __launch_bounds__(kB) void k_motion_apply(int n, const int* __restrict__ dof, const double* __restrict__ target, const double* __restrict__ vstar,
                                                     const int* __restrict__ err, double* __restrict__ q, double* __restrict__ qvel) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n || *err) return;
  const int d = dof[i];
  if (d < 0) return;
  q[d] = target[i];
  qvel[d] = vstar[i];
}

// FB_CUT_BAKE is about to add q to the rest positions and zero it: a target is a displacement from the rest shape, so u_c -= q_c keeps
// the world-space target x0_c + u_c where it is.  From the caller's ids, as k_motion_map: the table may be stale here.
__global__ __launch_bounds__(kB) void k_motion_rebase(int n, const int* __restrict__ dofs_caller, const int* __restrict__ new_of_old, int n_nodes,
                                                      const double* __restrict__ q, double* __restrict__ target) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  const int c = dofs_caller[i], node = c / 3;
  if ((unsigned)node >= (unsigned)n_nodes) return;
  const int in = new_of_old ? new_of_old[node] : node;
  if ((unsigned)in >= (unsigned)n_nodes) return;
  target[i] -= q[3 * (size_t)in + (c - 3 * node)];
}

// ---- the grasp ----

// the grasped nodes' world positions, and their displacement as the targets of their DOFs
__global__ __launch_bounds__(kB) void k_grasp_take(int n_nodes_g, const int* __restrict__ nodes, const int* __restrict__ new_of_old, int n_nodes,
                                                   const double* __restrict__ x0, const double* __restrict__ q, const int* __restrict__ slot,
                                                   double* __restrict__ pos, double* __restrict__ target) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_nodes_g) return;
  const int c = nodes[j];
  const int in = (unsigned)c < (unsigned)n_nodes ? (new_of_old ? new_of_old[c] : c) : -1;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const bool ok = (unsigned)in < (unsigned)n_nodes;
    const double u = ok ? q[3 * (size_t)in + a] : 0.0;
    pos[3 * (size_t)j + a] = ok ? x0[3 * (size_t)in + a] + u : 0.0;
    const int s = slot[3 * (size_t)j + a];
    if (s >= 0) target[s] = u;
  }
}

struct GraspMotion { double v[15]; };  // R (row-major) | t | pivot, a kernel argument

// targets = R (p_grab - pivot) + pivot + t - x0
__global__ __launch_bounds__(kB) void k_grasp_move(int n_nodes_g, const int* __restrict__ nodes, const int* __restrict__ new_of_old, int n_nodes,
                                                   const double* __restrict__ x0, const double* __restrict__ pos, const int* __restrict__ slot, GraspMotion M,
                                                   double* __restrict__ target) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_nodes_g) return;
  const int c = nodes[j];
  const int in = (unsigned)c < (unsigned)n_nodes ? (new_of_old ? new_of_old[c] : c) : -1;
  if ((unsigned)in >= (unsigned)n_nodes) return;
  const double* R = M.v;
  const double* tr = M.v + 9;
  const double* pv = M.v + 12;
  const double d[3] = {pos[3 * (size_t)j] - pv[0], pos[3 * (size_t)j + 1] - pv[1], pos[3 * (size_t)j + 2] - pv[2]};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int s = slot[3 * (size_t)j + a];
    if (s < 0) continue;
    const double w = ((R[3 * a] * d[0] + R[3 * a + 1] * d[1]) + R[3 * a + 2] * d[2]) + pv[a] + tr[a];
    target[s] = w - x0[3 * (size_t)in + a];
  }
}

// ---- host ----

int check_motion_handle(const fb_fem_s* h, const char* who) {
  if (h->plan.n_ranks > 1 || (h->comm && h->comm->n_ranks > 1)) return fail(FB_EINVAL, "%s is for unsharded handles", who);
  if (h->prm.integrator == FB_INTEGRATOR_NEWMARK) return fail(FB_EINVAL, "%s is not built for FB_INTEGRATOR_NEWMARK", who);
  return FB_OK;
}

// the set's arrays for n entries
int reserve_set(MotionWork& W, size_t n) {
  const size_t m = std::max<size_t>(n, 1);
  FB_TRY(W.target.reserve(m)); FB_TRY(W.vstar.reserve(m)); FB_TRY(W.dvc.reserve(m)); FB_TRY(W.react.reserve(m + 3)); FB_TRY(W.err.reserve(1));
  FB_TRY(W.dofs_dev.reserve(m)); FB_TRY(W.dof.reserve(m));
  return FB_OK;
}

// the set replaced by (dofs, targets) -- both on the host, validated
int install_set(fb_fem_s* h, const std::vector<int>& dofs, const std::vector<double>& targets) {
  MotionWork& W = h->motion;
  hipStream_t s = h->stream;
  const size_t n = dofs.size();
  if (n && dofs == W.dofs) {  // new targets for the same DOFs: the table, the grasp's entries and the last step's reactions stay
    FB_HIP(hipMemcpyAsync(W.target.p, targets.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
    FB_HIP(hipStreamSynchronize(s));
    return FB_OK;
  }
  if (n) {
    FB_TRY(reserve_set(W, n));
    FB_HIP(hipMemcpyAsync(W.target.p, targets.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
    FB_HIP(hipMemsetAsync(W.react.p, 0, sizeof(double) * (n + 3), s));
    FB_HIP(hipMemsetAsync(W.err.p, 0, sizeof(int), s));
    FB_HIP(hipStreamSynchronize(s));
  }
  W.dofs = dofs;
  W.table_valid = false;
  W.react_valid = false;
  W.grasp_slots_valid = false;
  return FB_OK;
}

// The entries whose DOF is still in the constrained list stay, in order, with their targets; the others go.
int filter_set(fb_fem_s* h) {
  MotionWork& W = h->motion;
  if (W.dofs.empty()) return FB_OK;
  const std::vector<int>& fixed = h->fixed_caller;  // ascending (check_fixed_dofs)
  std::vector<int> keep;
  keep.reserve(W.dofs.size());
  for (size_t i = 0; i < W.dofs.size(); i++)
    if (std::binary_search(fixed.begin(), fixed.end(), W.dofs[i])) keep.push_back((int)i);
  if (keep.size() == W.dofs.size()) return FB_OK;
  std::vector<double> u(W.dofs.size()), u2(keep.size());
  FB_TRY(W.target.download(u.data(), u.size(), h->stream));
  std::vector<int> d2(keep.size());
  for (size_t k = 0; k < keep.size(); k++) { d2[k] = W.dofs[(size_t)keep[k]]; u2[k] = u[(size_t)keep[k]]; }
  return install_set(h, d2, u2);
}

// The table of the current (set, mesh generation).  count: table_builds goes up (fb_fem_time_motion's repetitions do not count)
int build_table(fb_fem_s* h, bool count) {
  MotionWork& W = h->motion;
  PlanWorkspace& ws = h->plan_ws;
  hipStream_t s = h->stream;
  FB_TRY(filter_set(h));
  const int n = (int)W.dofs.size(), n_nodes = h->plan.n_global, nt = h->plan.n_tets;
  W.n_listed = W.n_touched = W.longest_run = 0;
  if (n == 0) { W.table_valid = true; return FB_OK; }
  FB_TRY(reserve_set(W, (size_t)n));
  FB_TRY(W.dof_slot.reserve((size_t)3 * n_nodes));
  FB_TRY(W.flag.reserve((size_t)std::max(nt, 1)));
  FB_TRY(W.listed.reserve((size_t)std::max(nt, 1)));
  FB_TRY(W.counts.reserve(3));
  FB_HIP(hipMemcpyAsync(W.dofs_dev.p, W.dofs.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
  FB_HIP(hipMemsetAsync(W.dof_slot.p, 0xff, sizeof(int) * 3 * (size_t)n_nodes, s));
  FB_HIP(hipMemsetAsync(W.counts.p, 0, sizeof(int) * 3, s));
  FB_TRY(launch_1d(k_motion_map, n, s, n, W.dofs_dev.p, h->ren.active ? h->ren.d_new_of_old.p : nullptr, n_nodes, W.dof.p, W.dof_slot.p));
  FB_TRY(launch_1d(k_motion_flag, nt, s, nt, h->tets.p, n_nodes, W.dof_slot.p, W.flag.p));
  FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.listed.p, W.counts.p, (size_t)nt));
  int n_listed = 0;
  FB_TRY(W.counts.download(&n_listed, 1, s));  // a host wait
  if (n_listed < 0 || n_listed > nt) return fail(FB_EDEVICE, "constrained motion: %d listed elements of %d", n_listed, nt);
  W.n_listed = n_listed;
  if (n_listed > 0) {
    if (n_listed >= (1 << 28)) return fail(FB_EINVAL, "constrained motion: %d listed elements", n_listed);
    const size_t n_rec = (size_t)4 * n_listed;
    FB_TRY(W.esel.reserve(3 * n_rec)); FB_TRY(W.y.reserve(3 * n_rec));
    FB_TRY(W.key.reserve(n_rec)); FB_TRY(W.key_s.reserve(n_rec)); FB_TRY(W.val.reserve(n_rec)); FB_TRY(W.val_s.reserve(n_rec));
    FB_TRY(W.heads.reserve(n_rec));
    FB_TRY(W.flag.reserve(std::max<size_t>(n_rec, (size_t)nt)));  // (reserve keeps the flags' buffer or grows it: the flags are spent)
    FB_TRY(launch_1d(k_motion_corners, (long long)n_rec, s, (int)n_rec, W.listed.p, h->tets.p, n_nodes, W.dof_slot.p, W.key.p, W.val.p, W.esel.p));
    FB_TRY(sort_pairs(ws.temp, s, W.key.p, W.key_s.p, W.val.p, W.val_s.p, n_rec, (unsigned)bits_of((long long)n_nodes + 1)));
    FB_TRY(launch_1d(k_motion_heads, (long long)n_rec, s, (int)n_rec, W.key_s.p, n_nodes, W.flag.p, W.counts.p + 2));
    FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.heads.p, W.counts.p + 1, n_rec));
    int c[3] = {0, 0, 0};
    FB_TRY(W.counts.download(c, 3, s));  // a host wait
    if (c[1] < 0 || (size_t)c[1] > n_rec) return fail(FB_EDEVICE, "constrained motion: %d touched nodes of %zu records", c[1], n_rec);
    W.n_touched = c[1];
    W.longest_run = c[2];
  }
  W.table_valid = true;
  if (count) W.table_builds++;
  return FB_OK;
}

MotionParams element_params(const fb_fem_s* h) {
  MotionParams P;
  P.lambda = h->lambda; P.mu = h->mu; P.rho20 = h->prm.rho / 20.0;
  P.mtab = has_material_map(h) ? h->mat_tab.p : nullptr;
  P.a_k = P.a_m = P.b_k = P.b_m = 0.0;
  P.rest = h->rest.p; P.x0 = h->x0.p; P.q = h->q.p; P.linear = h->prm.linear != 0 ? 1 : 0;
  return P;
}

template <bool REACT>
int launch_elements(fb_fem_s* h, const MotionParams& P) {
  MotionWork& W = h->motion;
  if (h->f64)
    return launch_1d(k_motion_elements<double, REACT>, W.n_listed, h->stream, W.n_listed, W.listed.p, W.esel.p, h->tets.p, h->plan.n_global, (const double*)h->rec.p,
                     (const double*)h->kcorr.p, h->fe.p, P, W.dvc.p, h->x.p, h->qvel.p, W.y.p);
  return launch_1d(k_motion_elements<float, REACT>, W.n_listed, h->stream, W.n_listed, W.listed.p, W.esel.p, h->tets.p, h->plan.n_global, (const float*)h->rec.p,
                   (const float*)h->kcorr.p, h->fe.p, P, W.dvc.p, h->x.p, h->qvel.p, W.y.p);
}

// v*, dv_c, and the correction subtracted from `rhs` (the step: h->rhs)
int correct_rhs(fb_fem_s* h, double* rhs) {
  MotionWork& W = h->motion;
  hipStream_t s = h->stream;
  const int n = (int)W.dofs.size();
  const double hh = h->prm.timestep;
  FB_HIP(hipMemsetAsync(W.err.p, 0, sizeof(int), s));
  FB_TRY(launch_1d(k_motion_dv, n, s, n, W.dof.p, W.target.p, h->q.p, h->qvel.p, hh, W.vstar.p, W.dvc.p, W.err.p));
  if (W.n_listed == 0) return FB_OK;
  MotionParams P = element_params(h);
  P.a_k = hh * (hh + h->prm.damping_stiffness); P.a_m = 1.0 + hh * h->prm.damping_mass;  // s_k, s_m of assemble_system
  FB_TRY(launch_elements<false>(h, P));
  const int n_rec = 4 * W.n_listed;
  return launch_1d(k_motion_gather<false>, W.n_touched, s, W.n_touched, W.heads.p, n_rec, W.key_s.p, W.val_s.p, W.esel.p, W.y.p, h->dofmask.p, h->fext.p, rhs);
}

// lambda of the set into react[0 .. n), its sum by axis behind it
int reactions(fb_fem_s* h, double* react) {
  MotionWork& W = h->motion;
  hipStream_t s = h->stream;
  const int n = (int)W.dofs.size();
  const double hh = h->prm.timestep, cM = h->prm.damping_mass, cK = h->prm.damping_stiffness;
  FB_TRY(launch_1d(k_motion_react_init, n + 3, s, n, W.dof.p, h->fext.p, react));
  if (W.n_listed > 0) {
    MotionParams P = element_params(h);
    P.a_k = hh * (hh + cK) / hh; P.a_m = (1.0 + hh * cM) / hh;  // (1/h) Keff
    P.b_k = hh + cK; P.b_m = cM;                               // g_k, g_m of assemble_system
    FB_TRY(launch_elements<true>(h, P));
    const int n_rec = 4 * W.n_listed;
    FB_TRY(launch_1d(k_motion_gather<true>, W.n_touched, s, W.n_touched, W.heads.p, n_rec, W.key_s.p, W.val_s.p, W.esel.p, W.y.p, h->dofmask.p, h->fext.p, react));
  }
  return launch_grid(k_motion_sum3, dim3(1), s, n, W.dof.p, react, react + n);
}

// the grasp's entries in the current set
int grasp_slots(fb_fem_s* h) {
  MotionWork& W = h->motion;
  if (W.grasp_slots_valid) return FB_OK;
  const size_t ng = W.grasp_nodes.size();
  std::vector<int> slot(3 * ng, -1);
  for (size_t j = 0; j < ng; j++)
    for (int a = 0; a < 3; a++) {
      const int d = 3 * W.grasp_nodes[j] + a;
      const auto it = std::lower_bound(W.dofs.begin(), W.dofs.end(), d);
      if (it != W.dofs.end() && *it == d) slot[3 * j + a] = (int)(it - W.dofs.begin());
    }
  FB_TRY(W.grasp_slot.reserve(std::max<size_t>(3 * ng, 1)));
  if (ng) {
    FB_HIP(hipMemcpyAsync(W.grasp_slot.p, slot.data(), sizeof(int) * 3 * ng, hipMemcpyHostToDevice, h->stream));
    FB_HIP(hipStreamSynchronize(h->stream));
  }
  W.grasp_slots_valid = true;
  return FB_OK;
}

}  // namespace

// ---- what the step and the life cycle ask ----

int motion_correct_rhs(fb_fem_s* h) {
  if (!h->motion.table_valid) FB_TRY(build_table(h, true));
  if (h->motion.dofs.empty()) return FB_OK;  // (the filter may have emptied the set)
  return correct_rhs(h, h->rhs.p);
}

int motion_reactions(fb_fem_s* h) {
  MotionWork& W = h->motion;
  if (W.dofs.empty() || !W.table_valid) return FB_OK;
  FB_TRY(reactions(h, W.react.p));
  W.react_valid = true;
  return FB_OK;
}

int motion_apply(fb_fem_s* h) {
  MotionWork& W = h->motion;
  if (W.dofs.empty() || !W.table_valid) return FB_OK;
  const int n = (int)W.dofs.size();
  FB_TRY(launch_1d(k_motion_apply, n, h->stream, n, W.dof.p, W.target.p, W.vstar.p, W.err.p, h->q.p, h->qvel.p));
  int err = 0;
  FB_TRY(W.err.download(&err, 1, h->stream));  // (the step waits for its stream anyway)
  if (err) return fail(FB_EINVAL, "constrained motion: a target or the state at a moved DOF is not finite; the moved DOFs were left as the step wrote them");
  return FB_OK;
}

void motion_mesh_changed(MotionWork& W) { W.table_valid = false; W.grasp_slots_valid = false; }

int motion_rest_absorbs_q(fb_fem_s* h) {
  MotionWork& W = h->motion;
  FB_TRY(filter_set(h));
  const int n = (int)W.dofs.size();
  if (n == 0) return FB_OK;
  hipStream_t s = h->stream;
  FB_TRY(reserve_set(W, (size_t)n));
  FB_HIP(hipMemcpyAsync(W.dofs_dev.p, W.dofs.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
  return launch_1d(k_motion_rebase, n, s, n, W.dofs_dev.p, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->plan.n_global, h->q.p, W.target.p);
}

void motion_clear(MotionWork& W) {
  W.dofs.clear();
  W.grasp_nodes.clear();
  W.grasp_added.clear();
  W.grasp_set_added.clear();
  W.table_valid = false;
  W.react_valid = false;
  W.grasp_slots_valid = false;
  W.n_listed = W.n_touched = W.longest_run = 0;
}

int motion_constraints_changed(fb_fem_s* h) {
  if (h->motion.dofs.empty()) return FB_OK;
  h->motion.table_valid = false;
  return filter_set(h);
}

}  // namespace fb

// ---- the C ABI ----

int fb_fem_set_constrained_motion(fb_fem_t h, int n, const int* dofs, const double* displacements) {
  CHECK_HANDLE(h);
  FB_TRY(check_motion_handle(h, "fb_fem_set_constrained_motion"));
  if (n < 0 || (n > 0 && (!dofs || !displacements))) return fail(FB_EINVAL, "fb_fem_set_constrained_motion: null array with a count, or a negative count");
  const std::vector<int>& fixed = h->fixed_caller;
  for (int i = 0; i < n; i++) {
    if (i && dofs[i] <= dofs[i - 1]) return fail(FB_EINVAL, "fb_fem_set_constrained_motion: dofs[%d] = %d: ids must ascend", i, dofs[i]);
    if (!std::binary_search(fixed.begin(), fixed.end(), dofs[i])) return fail(FB_EINVAL, "fb_fem_set_constrained_motion: DOF %d is not constrained", dofs[i]);
    if (!std::isfinite(displacements[i])) return fail(FB_EINVAL, "fb_fem_set_constrained_motion: the target of DOF %d is not finite", dofs[i]);
  }
  return install_set(h, std::vector<int>(dofs, dofs + n), std::vector<double>(displacements, displacements + n));
}

int fb_fem_num_constrained_motion(fb_fem_t h) {
  if (!h || h->poisoned) return -1;
  if (filter_set(h) != FB_OK) return -1;
  return (int)h->motion.dofs.size();
}

int fb_fem_read_constrained_motion(fb_fem_t h, int* dofs, double* displacements) {
  CHECK_HANDLE(h);
  FB_TRY(filter_set(h));
  const MotionWork& W = h->motion;
  if (dofs && !W.dofs.empty()) memcpy(dofs, W.dofs.data(), sizeof(int) * W.dofs.size());
  if (displacements) FB_TRY(W.target.download(displacements, W.dofs.size(), h->stream));
  return FB_OK;
}

int fb_fem_read_reactions(fb_fem_t h, double* forces, double* sum3) {
  CHECK_HANDLE(h);
  FB_TRY(filter_set(h));
  const MotionWork& W = h->motion;
  const size_t n = W.dofs.size();
  if (!W.react_valid || n == 0) {
    if (forces) std::fill(forces, forces + n, 0.0);
    if (sum3) sum3[0] = sum3[1] = sum3[2] = 0.0;
    return FB_OK;
  }
  if (forces) FB_TRY(W.react.download(forces, n, h->stream));
  if (sum3) FB_TRY(W.react.download(sum3, 3, h->stream, n));
  return FB_OK;
}

int fb_fem_motion_info_get(fb_fem_t h, fb_fem_motion_info* out) {
  CHECK_HANDLE(h);
  if (!out) return fail(FB_EINVAL, "fb_fem_motion_info_get: null output");
  FB_TRY(filter_set(h));
  const MotionWork& W = h->motion;
  memset(out, 0, sizeof(*out));
  out->n_dofs = (int)W.dofs.size();
  out->table_valid = W.table_valid ? 1 : 0;
  out->n_listed_elements = W.table_valid ? W.n_listed : 0;
  out->n_touched_nodes = W.table_valid ? W.n_touched : 0;
  out->longest_run = W.table_valid ? W.longest_run : 0;
  out->table_builds = W.table_builds;
  out->n_grasp_nodes = (int)W.grasp_nodes.size();
  return FB_OK;
}

int fb_fem_time_motion(fb_fem_t h, int reps, double seconds[4]) {
  CHECK_HANDLE(h);
  FB_TRY(check_motion_handle(h, "fb_fem_time_motion"));
  if (reps < 1 || !seconds) return fail(FB_EINVAL, "fb_fem_time_motion: reps must be positive and seconds not null");
  MotionWork& W = h->motion;
  FB_TRY(filter_set(h));
  if (W.dofs.empty()) return fail(FB_EINVAL, "fb_fem_time_motion: the handle has no motion set");
  hipStream_t s = h->stream;
  for (auto& e : W.ev_t)
    if (!e) FB_HIP(hipEventCreate(&e));
  FB_TRY(assemble_system(h));  // the step records and element forces of the current state
  if (!W.table_valid) FB_TRY(build_table(h, true));
  const size_t n = W.dofs.size();
  FB_TRY(W.react_t.reserve(n + 3));
  // what the stages write goes to solver scratch: r for the right-hand side, tmp and Ad for q and qvel -- the state, the step's
  // right-hand side and the reactions of the last step stay what they are
  const int nn = (int)n;
  auto stage = [&](int k) -> int {
    switch (k) {
      case 0: return build_table(h, false);
      case 1: return correct_rhs(h, h->r.p);
      case 2: return reactions(h, W.react_t.p);
      default: return launch_1d(k_motion_apply, nn, s, nn, W.dof.p, W.target.p, W.vstar.p, W.err.p, h->tmp.p, h->Ad.p);
    }
  };
  for (int k = 0; k < 4; k++) {
    FB_TRY(stage(k));  // warm
    seconds[k] = 0.0;
  }
  for (int r = 0; r < reps; r++)
    for (int k = 0; k < 4; k++) {
      FB_HIP(hipEventRecord(W.ev_t[0], s));
      FB_TRY(stage(k));
      FB_HIP(hipEventRecord(W.ev_t[1], s));
      FB_HIP(hipEventSynchronize(W.ev_t[1]));
      float ms = 0;
      FB_HIP(hipEventElapsedTime(&ms, W.ev_t[0], W.ev_t[1]));
      seconds[k] += ms * 1e-3 / reps;
    }
  h->system_valid = false;
  return FB_OK;
}

int fb_fem_grasp(fb_fem_t h, int n_nodes, const int* node_ids, fb_fem_motion_info* info) {
  CHECK_HANDLE(h);
  FB_TRY(check_motion_handle(h, "fb_fem_grasp"));
  MotionWork& W = h->motion;
  if (n_nodes < 1 || !node_ids) return fail(FB_EINVAL, "fb_fem_grasp: no nodes");
  if (!W.grasp_nodes.empty()) return fail(FB_EINVAL, "fb_fem_grasp: the handle holds a grasp already (fb_fem_release first)");
  for (int j = 0; j < n_nodes; j++) {
    if (node_ids[j] < 0 || node_ids[j] >= h->plan.n_global) return fail(FB_EINVAL, "fb_fem_grasp: node %d outside [0,%d)", node_ids[j], h->plan.n_global);
    if (j && node_ids[j] <= node_ids[j - 1]) return fail(FB_EINVAL, "fb_fem_grasp: node_ids[%d] = %d: ids must ascend", j, node_ids[j]);
  }
  FB_TRY(filter_set(h));
  // the constrained list with the nodes' DOFs merged in; what was not in it before is what fb_fem_release takes out again
  const std::vector<int> fixed = h->fixed_caller;
  std::vector<int> mine((size_t)3 * n_nodes), merged, added;
  for (int j = 0; j < n_nodes; j++)
    for (int a = 0; a < 3; a++) mine[3 * (size_t)j + a] = 3 * node_ids[j] + a;
  std::set_union(fixed.begin(), fixed.end(), mine.begin(), mine.end(), std::back_inserter(merged));
  std::set_difference(mine.begin(), mine.end(), fixed.begin(), fixed.end(), std::back_inserter(added));
  std::vector<int> set_added;
  std::set_difference(mine.begin(), mine.end(), W.dofs.begin(), W.dofs.end(), std::back_inserter(set_added));
  // the set with them merged in; entries it had keep their targets, the new ones get the current q below
  std::vector<double> u_old(W.dofs.size());
  FB_TRY(W.target.download(u_old.data(), u_old.size(), h->stream));
  std::vector<int> set2;
  std::set_union(W.dofs.begin(), W.dofs.end(), mine.begin(), mine.end(), std::back_inserter(set2));
  std::vector<double> u2(set2.size(), 0.0);
  for (size_t i = 0; i < W.dofs.size(); i++) u2[(size_t)(std::lower_bound(set2.begin(), set2.end(), W.dofs[i]) - set2.begin())] = u_old[i];
  const std::vector<int> set_old = W.dofs;
  FB_TRY(fb_fem_set_constrained_dofs(h, (int)merged.size(), merged.data()));
  FB_TRY(install_set(h, set2, u2));
  W.grasp_nodes.assign(node_ids, node_ids + n_nodes);
  W.grasp_added = added;
  W.grasp_set_added = set_added;
  hipStream_t s = h->stream;
  FB_TRY(W.grasp_nodes_dev.reserve((size_t)n_nodes));
  FB_TRY(W.grasp_pos.reserve((size_t)3 * n_nodes));
  FB_HIP(hipMemcpyAsync(W.grasp_nodes_dev.p, node_ids, sizeof(int) * (size_t)n_nodes, hipMemcpyHostToDevice, s));
  FB_TRY(grasp_slots(h));
  FB_TRY(launch_1d(k_grasp_take, n_nodes, s, n_nodes, W.grasp_nodes_dev.p, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->plan.n_global, h->x0.p, h->q.p,
                   W.grasp_slot.p, W.grasp_pos.p, W.target.p));
  // an entry the set held before the grasp keeps its target: k_grasp_take wrote the current q over it (rare, and a few doubles)
  for (size_t i = 0; i < set_old.size(); i++)
    if (std::binary_search(mine.begin(), mine.end(), set_old[i])) {
      const size_t at = (size_t)(std::lower_bound(set2.begin(), set2.end(), set_old[i]) - set2.begin());
      FB_HIP(hipMemcpyAsync(W.target.p + at, &u_old[i], sizeof(double), hipMemcpyHostToDevice, s));
    }
  FB_HIP(hipStreamSynchronize(s));
  if (info) return fb_fem_motion_info_get(h, info);
  return FB_OK;
}

int fb_fem_grasp_move(fb_fem_t h, const double R[9], const double t[3], const double pivot[3]) {
  CHECK_HANDLE(h);
  FB_TRY(check_motion_handle(h, "fb_fem_grasp_move"));
  MotionWork& W = h->motion;
  if (W.grasp_nodes.empty()) return fail(FB_EINVAL, "fb_fem_grasp_move: the handle holds no grasp");
  if (!R || !t || !pivot) return fail(FB_EINVAL, "fb_fem_grasp_move: null argument");
  GraspMotion M;
  memcpy(M.v, R, sizeof(double) * 9); memcpy(M.v + 9, t, sizeof(double) * 3); memcpy(M.v + 12, pivot, sizeof(double) * 3);
  for (double v : M.v)
    if (!std::isfinite(v)) return fail(FB_EINVAL, "fb_fem_grasp_move: the motion is not finite");
  FB_TRY(filter_set(h));
  FB_TRY(grasp_slots(h));
  const int ng = (int)W.grasp_nodes.size();
  return launch_1d(k_grasp_move, ng, h->stream, ng, W.grasp_nodes_dev.p, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->plan.n_global, h->x0.p, W.grasp_pos.p,
                   W.grasp_slot.p, M, W.target.p);
}

int fb_fem_release(fb_fem_t h) {
  CHECK_HANDLE(h);
  MotionWork& W = h->motion;
  if (W.grasp_nodes.empty()) return FB_OK;
  FB_TRY(filter_set(h));
  std::vector<int> added = W.grasp_added, fixed2;
  // the entries the grasp put into the set go, the others keep their targets
  if (!W.grasp_set_added.empty() && !W.dofs.empty()) {
    std::vector<double> u(W.dofs.size()), u2;
    FB_TRY(W.target.download(u.data(), u.size(), h->stream));
    std::vector<int> d2;
    for (size_t i = 0; i < W.dofs.size(); i++)
      if (!std::binary_search(W.grasp_set_added.begin(), W.grasp_set_added.end(), W.dofs[i])) { d2.push_back(W.dofs[i]); u2.push_back(u[i]); }
    FB_TRY(install_set(h, d2, u2));
  }
  W.grasp_nodes.clear();
  W.grasp_added.clear();
  W.grasp_set_added.clear();
  W.grasp_slots_valid = false;
  const std::vector<int> fixed = h->fixed_caller;
  std::set_difference(fixed.begin(), fixed.end(), added.begin(), added.end(), std::back_inserter(fixed2));
  // (fb_fem_set_constrained_dofs drops the freed DOFs from the set; q and qvel are not touched)
  return fb_fem_set_constrained_dofs(h, (int)fixed2.size(), fixed2.data());
}
