// Element stress and strain on the device (stress.h), hand-written for gfx950.
//
// k_tet_stress: a thread per element forms F and the assembly's rotation exactly as k_tet_warp does (same expressions, same
// polar_rotation, the unit is built with -ffp-contract=off), H through the displacement gradient (below: the assembly's node-by-node sum
// is good to the force's 1e-9, not to a strain of 1e-13 on a flat element), and from H the strain, the stress of the element's own
// material, von Mises, the energy density and J.  Per element it reads 16 B of ids, 104 B of its rest record and the four node gathers, and writes 24 B
// (120 B more with TENSORS).  MAT and TENSORS are template parameters: a uniform handle that wants colours only neither reads a
// table nor writes tensors.  Every index is the thread's own id, checked against the count, or a node id of the handle's element list,
// checked against n_nodes; a material id is masked into the full-size table.
//
// Summary: largest (von Mises, element), smallest (J, element), the inverted count and the sum of V psi leave the workgroup as
// partials (shuffles, LDS) and a second, single-workgroup launch folds them in a fixed order -- no floating-point atomics, the same bits
// from call to call.
//
// Surface: a thread per surface vertex walks the faces of its vertex in ascending face order (SurfaceWork's corner lists).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "fem_handle.h"
#include "launch.hip.h"
#include "stress.h"
#include "tet_math.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

// what a thread (element or strided partials) carries into the workgroup's fold
struct Fold {
  double vm; int vm_e;   // largest von Mises, of equal ones the lowest element
  double J; int J_e;     // smallest J, likewise
  int inverted;
  double energy;
};

// Over the workgroup; valid in thread 0.  The wavefront-level pieces of workgroup.hip.h with ONE exchange through LDS and one barrier for
// the six values (four wg_* calls would bring eight), so it is called once in a kernel.  The sum is wg_sum's tree.
__device__ __forceinline__ void fold_reduce(Fold& f) {
  for (int o = 32; o >= 1; o >>= 1) {  // (the three butterflies step by step together: their exchanges overlap)
    wf_best_step<int, Highest>(f.vm, f.vm_e, o);
    wf_best_step<int, Lowest>(f.J, f.J_e, o);
    f.inverted += __shfl_xor(f.inverted, o);
  }
  f.energy = wf_sum(f.energy);
  __shared__ double s_vm[kWaves], s_J[kWaves], s_en[kWaves];
  __shared__ int s_vme[kWaves], s_Je[kWaves], s_inv[kWaves];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_vm[w] = f.vm; s_vme[w] = f.vm_e; s_J[w] = f.J; s_Je[w] = f.J_e; s_inv[w] = f.inverted; s_en[w] = f.energy; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; k++) {
      if (Highest()(s_vm[k], s_vme[k], f.vm, f.vm_e)) { f.vm = s_vm[k]; f.vm_e = s_vme[k]; }
      if (Lowest()(s_J[k], s_Je[k], f.J, f.J_e)) { f.J = s_J[k]; f.J_e = s_Je[k]; }
      f.inverted += s_inv[k];
    }
    static_assert(kWaves == 4, "the sum's tree is written for four wavefronts");
    f.energy = (s_en[0] + s_en[1]) + (s_en[2] + s_en[3]);
  }
}

// T <- R T R^T (T symmetric, row-major)
__device__ __forceinline__ void to_world(const double* R, double* T) {
  double A[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) A[3 * i + j] = R[3 * i] * T[j] + R[3 * i + 1] * T[3 + j] + R[3 * i + 2] * T[6 + j];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = i; j < 3; j++) T[3 * i + j] = T[3 * j + i] = A[3 * i] * R[3 * j] + A[3 * i + 1] * R[3 * j + 1] + A[3 * i + 2] * R[3 * j + 2];
}

__device__ __forceinline__ void store6(double* __restrict__ dst, const double* T) {  // xx yy zz xy yz zx: 48 bytes, 16-byte aligned
  double2* d = reinterpret_cast<double2*>(dst);
  d[0] = make_double2(T[0], T[4]);
  d[1] = make_double2(T[8], T[1]);
  d[2] = make_double2(T[5], T[6]);
}

template <bool MAT, bool TENSORS>
__global__ __launch_bounds__(kB) void k_tet_stress(StressArgs a, double* __restrict__ vm_out, double* __restrict__ psi_out, double* __restrict__ J_out,
                                                       double* __restrict__ sig_out, double* __restrict__ eps_out, double* __restrict__ part_d, int* __restrict__ part_i) {
  const int e = blockIdx.x * kB + threadIdx.x;
  Fold f;
  f.vm = -INFINITY; f.vm_e = INT_MAX; f.J = INFINITY; f.J_e = INT_MAX; f.inverted = 0; f.energy = 0.0;
  if (e < a.n_tets) {
    const int4 t = a.tets[e];
    const int id[4] = {t.x, t.y, t.z, t.w};
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) ok = ok && (unsigned)id[k] < (unsigned)a.n_nodes;
    double lambda = a.lambda, mu = a.mu;
    if (MAT) {  // the element's own Lame parameters (any byte indexes inside the full-size table)
      const int mid = a.mat_ids[e] & (kMaxMaterials - 1);
      lambda = a.mtab[mid];
      mu = a.mtab[kMaxMaterials + mid];
    }
    double b[4][3], U[4][3], P[4][3];
    const double2* r2 = reinterpret_cast<const double2*>(a.rest + 16 * (size_t)e);  // 13 of the record's 16 doubles
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double2 v = r2[k];
      b[(2 * k) / 3][(2 * k) % 3] = v.x;
      b[(2 * k + 1) / 3][(2 * k + 1) % 3] = v.y;
    }
    const double V = a.rest[16 * (size_t)e + 12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const size_t n = ok ? 3 * (size_t)id[k] : 0;
#pragma unroll
      for (int d = 0; d < 3; d++) {
        U[k][d] = a.q[n + d];
        P[k][d] = a.x0[n + d] + U[k][d];
      }
    }
    double F[9], R[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) F[3 * i + j] = P[0][i] * b[0][j] + P[1][i] * b[1][j] + P[2][i] * b[2][j] + P[3][i] * b[3][j];
    if (a.linear) {
#pragma unroll
      for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else {
      const double det = polar_rotation(F, R, 1e-6);
      if (det < 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = -R[i];
      }
    }
    // H = sum_j (R^T P_j - X_j) b_j^T = (R^T - I) + R^T D with the displacement gradient D = sum_j q_j b_j^T (sum_j X_j b_j^T = I):
    // summed node by node as written, a flat element (|b| of thousands) would multiply the rounding of x0 + q into the strain
    double D[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, H[9];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int d = 0; d < 3; d++) D[3 * c + d] += U[j][c] * b[j][d];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int d = 0; d < 3; d++) H[3 * c + d] = (R[3 * d + c] - (c == d ? 1.0 : 0.0)) + (R[c] * D[d] + R[3 + c] * D[3 + d] + R[6 + c] * D[6 + d]);
    const double tr = H[0] + H[4] + H[8];
    double S[9], E[9];  // lambda tr I + mu (H + H^T) | (H + H^T) / 2
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const double hs = H[3 * c + d] + H[3 * d + c];
        S[3 * c + d] = mu * hs + (c == d ? lambda * tr : 0.0);
        E[3 * c + d] = 0.5 * hs;
      }
    const double d0 = S[0] - S[4], d1 = S[4] - S[8], d2 = S[8] - S[0];
    double vm = sqrt(0.5 * (d0 * d0 + d1 * d1 + d2 * d2) + 3.0 * (S[1] * S[1] + S[5] * S[5] + S[6] * S[6]));
    double psi = 0.5 * (S[0] * E[0] + S[4] * E[4] + S[8] * E[8] + 2.0 * (S[1] * E[1] + S[5] * E[5] + S[6] * E[6]));
    double J = F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) + F[2] * (F[3] * F[7] - F[4] * F[6]);
    if (!ok) {  // (an element list with a node id out of range: validated on the way in, never met)
      vm = psi = J = 0.0;
#pragma unroll
      for (int i = 0; i < 9; i++) S[i] = E[i] = 0.0;
    }
    vm_out[e] = vm;
    psi_out[e] = psi;
    J_out[e] = J;
    if (TENSORS) {
      if (a.world) { to_world(R, S); to_world(R, E); }
      store6(sig_out + 6 * (size_t)e, S);
      store6(eps_out + 6 * (size_t)e, E);
    }
    f.vm = vm; f.vm_e = e; f.J = J; f.J_e = e; f.inverted = J < 0 ? 1 : 0; f.energy = V * psi;
  }
  fold_reduce(f);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x, k = blockIdx.x;
    part_d[k] = f.vm; part_d[nb + k] = f.J; part_d[2 * nb + k] = f.energy;
    part_i[k] = f.vm_e; part_i[nb + k] = f.J_e; part_i[2 * nb + k] = f.inverted;
  }
}

// one workgroup: thread t folds the partials t, t + 256, ... in that order, then the same fold
__global__ __launch_bounds__(kB) void k_stress_final(int n_part, const double* __restrict__ part_d, const int* __restrict__ part_i, int n_tets, int flags,
                                                         fb_fem_stress_info* __restrict__ out) {
  Fold f;
  f.vm = -INFINITY; f.vm_e = INT_MAX; f.J = INFINITY; f.J_e = INT_MAX; f.inverted = 0; f.energy = 0.0;
  const size_t nb = (size_t)n_part;
  for (int k = threadIdx.x; k < n_part; k += kB) {  // (one loop for the six arrays, not a fold_* each: their loads go out together)
    if (Highest()(part_d[k], part_i[k], f.vm, f.vm_e)) { f.vm = part_d[k]; f.vm_e = part_i[k]; }
    if (Lowest()(part_d[nb + k], part_i[nb + k], f.J, f.J_e)) { f.J = part_d[nb + k]; f.J_e = part_i[nb + k]; }
    f.inverted += part_i[2 * nb + k];
    f.energy += part_d[2 * nb + k];
  }
  fold_reduce(f);
  if (threadIdx.x == 0) {
    fb_fem_stress_info r;
    r.n_elements = n_tets; r.flags = flags;
    r.max_von_mises = f.vm; r.max_element = f.vm_e;
    r.min_J = f.J; r.min_J_element = f.J_e;
    r.n_inverted = f.inverted;
    r.energy = f.energy;
    *out = r;
  }
}

// A thread per surface vertex: the fp64 sum of its faces' elements in ascending face order, divided by the face count
__global__ __launch_bounds__(kB) void k_surface_stress(int n_vertices, int n_faces, int n_tets, const int* __restrict__ inc_off, const uint32_t* __restrict__ inc,
                                                           const int* __restrict__ face_tets, const double* __restrict__ vm, float* __restrict__ out) {
  const int v = blockIdx.x * kB + threadIdx.x;
  if (v >= n_vertices) return;
  double sum = 0.0;
  int cnt = 0;
  for (int j = inc_off[v]; j < inc_off[v + 1]; j++) {
    if (j < 0 || j >= 3 * n_faces) break;
    const unsigned face = inc[j] / 3u;
    if (face >= (unsigned)n_faces) continue;
    const int t = face_tets[face];
    if ((unsigned)t >= (unsigned)n_tets) continue;
    sum += vm[t];
    cnt++;
  }
  out[v] = cnt ? (float)(sum / (double)cnt) : 0.0f;
}

using StressKernel = void (*)(StressArgs, double*, double*, double*, double*, double*, double*, int*);
// [MAT][TENSORS]
const StressKernel kStressKernels[2][2] = {{k_tet_stress<false, false>, k_tet_stress<false, true>}, {k_tet_stress<true, false>, k_tet_stress<true, true>}};

}  // namespace

int stress_elements(hipStream_t s, StressWork& S, const StressArgs& a, bool tensors, fb_fem_stress_info* out) {
  S.valid = false;
  const int nt = a.n_tets, nblk = blocks_for(nt);
  const int flags = (a.world ? FB_STRESS_WORLD : 0) | (tensors ? FB_STRESS_TENSORS : 0);
  const size_t ne = (size_t)std::max(nt, 1);
  FB_TRY(S.vm.reserve(ne)); FB_TRY(S.psi.reserve(ne)); FB_TRY(S.J.reserve(ne));
  if (tensors) { FB_TRY(S.sig.reserve(6 * ne)); FB_TRY(S.eps.reserve(6 * ne)); }
  FB_TRY(S.part_d.reserve((size_t)3 * nblk)); FB_TRY(S.part_i.reserve((size_t)3 * nblk)); FB_TRY(S.out.reserve(1));
  if (nt > 0) {
    FB_TRY(launch_1d(kStressKernels[a.mat_ids ? 1 : 0][tensors ? 1 : 0], nt, s, a, S.vm.p, S.psi.p, S.J.p, tensors ? S.sig.p : nullptr, tensors ? S.eps.p : nullptr, S.part_d.p,
                     S.part_i.p));
    FB_TRY(launch_grid(k_stress_final, dim3(1), s, nblk, S.part_d.p, S.part_i.p, nt, flags, S.out.p));
    if (out) FB_TRY(S.out.download(out, 1, s));
  } else if (out) {
    out->n_elements = 0; out->flags = flags;
    out->max_von_mises = 0.0; out->max_element = -1; out->min_J = 0.0; out->min_J_element = -1; out->n_inverted = 0; out->energy = 0.0;
  }
  S.n_elements = nt;
  S.flags = flags;
  S.valid = true;
  return FB_OK;
}

int stress_surface(hipStream_t s, StressWork& S, int n_vertices, int n_faces, const int* inc_off, const uint32_t* inc, const int* face_tets) {
  if (n_vertices <= 0) return FB_OK;
  FB_TRY(S.surf_vm.reserve((size_t)n_vertices));
  return launch_1d(k_surface_stress, n_vertices, s, n_vertices, n_faces, S.n_elements, inc_off, inc, face_tets, S.vm.p, S.surf_vm.p);
}

}  // namespace fb

// ---- the C ABI ----

int fb::stress_current(const fb_fem_s* h, const char* who) {
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "%s is for unsharded handles", who);
  if (!h->stress.valid || h->stress.n_elements != h->plan.n_tets)
    return fail(FB_EINVAL, "%s: no fb_fem_stress of the current mesh (none yet, or the mesh has changed since)", who);
  return FB_OK;
}

namespace {

int run_stress(fb_fem_s* h, int flags, fb_fem_stress_info* out) {
  StressArgs a;
  a.n_tets = h->plan.n_tets; a.n_nodes = h->plan.n_global;
  a.tets = h->tets.p; a.x0 = h->x0.p; a.q = h->q.p; a.rest = h->rest.p;
  a.lambda = h->lambda; a.mu = h->mu;
  a.mat_ids = h->mat_ids.p; a.mtab = h->mat_ids.p ? h->mat_tab.p : nullptr;
  a.linear = h->prm.linear != 0 ? 1 : 0;
  a.world = (flags & FB_STRESS_WORLD) ? 1 : 0;
  SlackScope slack(handle_slack_now(h));
  return stress_elements(h->stream, h->stress, a, (flags & FB_STRESS_TENSORS) != 0, out);
}

int run_surface_stress(fb_fem_s* h, float* von_mises) {
  FB_TRY(surface_current(h));  // (builds it where it is stale)
  const SurfaceWork& F = h->surf;
  if (F.n_vertices <= 0) return FB_OK;
  SlackScope slack(handle_slack_now(h));
  FB_TRY(stress_surface(h->stream, h->stress, F.n_vertices, F.n_faces, F.inc_off.p, F.inc.p, F.face_tets.p));
  if (von_mises) FB_TRY(h->stress.surf_vm.download(von_mises, (size_t)F.n_vertices, h->stream));
  return FB_OK;
}

}  // namespace

int fb_fem_stress(fb_fem_t h, int flags, fb_fem_stress_info* out) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_stress is for unsharded handles");
  if (flags & ~(FB_STRESS_WORLD | FB_STRESS_TENSORS)) return fail(FB_EINVAL, "fb_fem_stress: unknown flag bits 0x%x", flags & ~(FB_STRESS_WORLD | FB_STRESS_TENSORS));
  fb_fem_stress_info info;
  FB_TRY(run_stress(h, flags, &info));
  if (out) *out = info;
  return FB_OK;
}

int fb_fem_read_stress(fb_fem_t h, int first, int count, double* von_mises, double* energy_density, double* J, double* stress6, double* strain6) {
  CHECK_HANDLE(h);
  FB_TRY(stress_current(h, "fb_fem_read_stress"));
  const StressWork& S = h->stress;
  if (first < 0 || count < 0 || first > S.n_elements || count > S.n_elements - first)
    return fail(FB_EINVAL, "fb_fem_read_stress: elements [%d, %d + %d) outside [0, %d)", first, first, count, S.n_elements);
  if ((stress6 || strain6) && !(S.flags & FB_STRESS_TENSORS)) return fail(FB_EINVAL, "fb_fem_read_stress: the last fb_fem_stress did not keep tensors (FB_STRESS_TENSORS)");
  if (count == 0) return FB_OK;
  hipStream_t s = h->stream;
  const size_t n = (size_t)count, o = (size_t)first;
  if (von_mises) FB_HIP(hipMemcpyAsync(von_mises, S.vm.p + o, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  if (energy_density) FB_HIP(hipMemcpyAsync(energy_density, S.psi.p + o, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  if (J) FB_HIP(hipMemcpyAsync(J, S.J.p + o, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  if (stress6) FB_HIP(hipMemcpyAsync(stress6, S.sig.p + 6 * o, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, s));
  if (strain6) FB_HIP(hipMemcpyAsync(strain6, S.eps.p + 6 * o, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  return FB_OK;
}

int fb_fem_surface_stress(fb_fem_t h, float* von_mises) {
  CHECK_HANDLE(h);
  FB_TRY(stress_current(h, "fb_fem_surface_stress"));
  return run_surface_stress(h, von_mises);
}

int fb_fem_time_stress(fb_fem_t h, int reps, int flags, double* seconds_elements, double* seconds_surface) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_time_stress is for unsharded handles");
  if (reps < 1) return fail(FB_EINVAL, "reps must be positive");
  if (flags & ~(FB_STRESS_WORLD | FB_STRESS_TENSORS)) return fail(FB_EINVAL, "fb_fem_time_stress: unknown flag bits 0x%x", flags & ~(FB_STRESS_WORLD | FB_STRESS_TENSORS));
  fb_fem_stress_info info;
  FB_TRY(run_stress(h, flags, &info));  // warm: the buffers exist
  FB_TRY(surface_current(h));
  std::vector<float> host((size_t)std::max(h->surf.n_vertices, 1));
  FB_TRY(run_surface_stress(h, host.data()));
  if (seconds_elements) FB_TRY(timed_median(h, reps, [&] { return run_stress(h, flags, &info); }, seconds_elements));
  if (seconds_surface) FB_TRY(timed_median(h, reps, [&] { return run_surface_stress(h, host.data()); }, seconds_surface));
  return FB_OK;
}
