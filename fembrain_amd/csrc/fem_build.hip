// The handle's life cycle (include/fembrain_hip.h): building a plan, creating and destroying a handle, the three kinds of re-sync (full, sharded,
// delta) and fb_fem_cut on top of the delta.  Each step is written once, below; what it needs of fem.hip is declared under "fem.hip" in fem_handle.h.
#include <cfloat>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "fem_handle.h"

using namespace fb;

namespace {

// one wavefront per slice: does any of its columns lie in the halo?
__global__ __launch_bounds__(kBlock) void k_slice_halo(int n_slices, int n_owned, const int* __restrict__ slice_off, const int* __restrict__ colidx,
                                                       unsigned char* __restrict__ out) {
  const int s = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= n_slices) return;
  bool any = false;
  for (int k = slice_off[s]; k < slice_off[s + 1]; k++) any = any || colidx[(size_t)k * 64 + lane] >= n_owned;
  const unsigned long long b = __ballot(any);
  if (lane == 0) out[s] = b != 0ULL ? 1 : 0;
}

constexpr int kFreshOrderPercent = 2;
int fresh_order_percent() {
  const char* e = getenv("FEMBRAIN_FRESH_ORDER_PERCENT");
  return e ? std::max(0, atoi(e)) : kFreshOrderPercent;
}

// ---- each step of a build, once ----

// FEMBRAIN_TIMING (development aid): where a (re)build spends its time, one "[fembrain] <prefix>: <what> at <ms> ms" per lap.  The variable is
// read when a timer is made, once per build: nothing is cached per process (HostKnobs)
struct LapTimer {
  static bool enabled() { return getenv("FEMBRAIN_TIMING") != nullptr; }
  const char* prefix;
  const bool on = enabled();
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit LapTimer(const char* p) : prefix(p) {}
  void operator()(const char* what) const {
    if (on) fprintf(stderr, "[fembrain] %s: %s at %.2f ms\n", prefix, what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

// A new mesh generation begins: the captured graph goes (the buffers it refers to are about to be replaced) and every per-generation flag
// of the handle (fem_handle.h, "per mesh generation") is reset.  keep: what fb_fem_resync_delta carries over on purpose
enum { kKeepOrder = 1, kKeepCsr = 2 };
void begin_mesh_generation(fb_fem_s* h, int keep = 0) {
  drop_graph(h);
  h->surf.valid = h->stress.valid = h->parts.valid = false;  // (fb_fem_surface; fb_fem_read_stress / fb_fem_surface_stress; fb_fem_parts)
  motion_mesh_changed(h->motion);  // (fb_fem_set_constrained_motion: the element table is built again, the set filtered by the new constrained list)
  embed_mesh_changed(h->embed, keep != 0 || h->map_from_delta);  // (fb_fem_embed: a change in place, or its full rebuild, is followed by resync_delta)
  contact_mesh_changed(h->contact, keep != 0 || h->map_from_delta);  // (fb_fem_contact_move: the same two keep the session, a full re-sync clears it)
  if (!(keep & kKeepCsr)) h->csr_ready = false;
  if (!(keep & kKeepOrder)) h->ren.clear();
  h->l2c.clear();
  h->order_sum = 0;
  h->span_stale = h->x0_ready = h->masks_ready = h->caller_pattern = false;
}

// A re-sync replaces the plan and the buffers in place; if it fails half way (a node id out of range after a bad subdivision, a flat
// element, no memory) the handle holds pieces of two meshes and must not step: it stays poisoned unless the re-sync commits
struct ResyncScope {
  fb_fem_s* h;
  explicit ResyncScope(fb_fem_s* handle) : h(handle) { h->poisoned = true; h->system_valid = false; }
  void commit() { h->poisoned = false; }
};

// the host's part of an unsharded plan: one rank, the identity numbering, no halo
FemPlan unsharded_plan(int n_nodes, int n_tets, int n_fixed) {
  FemPlan P;
  P.n_global = n_nodes; P.n_ranks = 1; P.rank = 0;
  P.splits = {0, n_nodes};
  P.node_lo = 0; P.node_hi = n_nodes;
  P.n_owned = P.n_local = n_nodes; P.n_halo = 0;
  P.local2global.resize(n_nodes);
  for (int l = 0; l < n_nodes; l++) P.local2global[l] = l;
  P.halo_off.assign(2, 0);
  P.send_off.assign(2, 0);
  P.n_tets = n_tets;
  P.n_fixed_owned = n_fixed;
  return P;
}

// the device plan builder's outputs wired to the handle's buffers (a shard adds halo_base, an unsharded handle ucnt_keep)
DevicePlan handle_plan_outputs(fb_fem_s* h) {
  DevicePlan D;
  D.slice_off = &h->slice_off; D.colidx = &h->colidx; D.slot_coff = &h->slot_coff; D.slot_ccnt = &h->slot_ccnt; D.contrib = &h->contrib;
  D.bptr = &h->d_bptr; D.bcol = &h->d_bcol; D.blk_slot = &h->d_blk_slot; D.coldelta = &h->coldelta;
  return D;
}

// the counts and slice offsets of a device-built plan, and whether the SpMV reads its 16-bit column words (c16_form: 1 column - row, 2 the halo form)
void adopt_device_plan(fb_fem_s* h, const DevicePlan& D, int c16_form) {
  FemPlan& P = h->plan;
  P.n_blocks = D.n_blocks; P.n_slices = D.n_slices; P.n_slots = D.n_slots; P.n_crows = D.n_crows;
  h->c16 = (D.deltas_fit16 && read_host_knobs().spmv_c16) ? c16_form : 0;
  P.slice_off = D.slice_off_host;
}

// the plan builder's temporaries are kept for the next re-sync only while they are small change (0.8 GB at 1M tets)
void release_large_plan_ws(fb_fem_s* h) {
  if (h->plan_ws.bytes() > ((size_t)2 << 30)) h->plan_ws.release();
}

// rc of a device builder that refused element first_bad_tet: say which node, as the host builder does
int bad_tet_error(int rc, int first_bad_tet, const int* tets, int n_nodes) {
  if (rc != FB_OK && first_bad_tet >= 0 && tets)
    for (int k = 0; k < 4; k++) {
      const int id = tets[4 * (size_t)first_bad_tet + k];
      if (id < 0 || id >= n_nodes) return fail(FB_EINVAL, "tet %d references node %d outside [0,%d)", first_bad_tet, id, n_nodes);
    }
  return rc;
}

// a constrained DOF list in the caller's ids: inside [0, n_dofs_total) and strictly ascending
int check_fixed_dofs(int n, const int* dofs, long long n_dofs_total) {
  for (int i = 0; i < n; i++) {
    if (dofs[i] < 0 || dofs[i] >= n_dofs_total) return fail(FB_EINVAL, "constrained DOF %d out of range [0,%lld)", dofs[i], n_dofs_total);
    if (i && dofs[i] <= dofs[i - 1]) return fail(FB_EINVAL, "constrained DOFs must be strictly ascending (index %d)", i);
  }
  return FB_OK;
}

// ... of a renumbered shard, in internal ids, ascending again (the list was checked)
std::vector<int> fixed_to_internal(const fb_fem_s* h, int n, const int* dofs) {
  std::vector<int> mapped((size_t)n);
  for (int i = 0; i < n; i++) mapped[i] = 3 * h->ren.new_of_old[dofs[i] / 3] + dofs[i] % 3;
  std::sort(mapped.begin(), mapped.end());
  return mapped;
}

// Collective: the ranks agree on a rank-local outcome before anything collective follows it, so that none waits in an all-gather for a
// rank that has left.  A rank that failed keeps its own code and message; the others report the first rank that failed,
// with fmt (rank, code); the communicator's error if the all-gather itself fails.
int agree_on_outcome(fb_comm_s* comm, hipStream_t stream, int rc_mine, const char* fmt) {
  const std::string why_mine = rc_mine == FB_OK ? std::string() : last_error();
  std::vector<int> rcs((size_t)comm->n_ranks, 0);
  FB_TRY(comm_allgather_bytes(comm, &rc_mine, rcs.data(), sizeof(int), stream));  // (host-staged or on the null stream if ours could not be made)
  if (rc_mine != FB_OK) { last_error() = why_mine; return rc_mine; }
  for (int q = 0; q < comm->n_ranks; q++)
    if (rcs[q] != FB_OK) return fail(rcs[q], fmt, q, rcs[q]);
  return FB_OK;
}

// The plan of an unsharded handle, built on the device (plan_device.hip).  The host keeps the scalars, the slice offsets,
// the identity numbering and the constraint mask; the pattern arrays stay on the device until an inspection entry point
// asks for them (ensure_host_pattern).
// tets: host node ids, or -- d_tets non-null -- ids already on this device (the polygonizer's own output: in range by construction)
int build_plan_on_device(fb_fem_s* h, int n_nodes, int n_tets, const int* tets, int n_fixed, const int* fixed, const double* xyz, const uint4* d_tets = nullptr,
                         const float* d_xyz = nullptr, const double* d_xyz64 = nullptr) {
  if (n_nodes <= 0 || n_tets <= 0 || (!tets && !d_tets)) return fail(FB_EINVAL, "empty mesh (%d nodes, %d tets)", n_nodes, n_tets);
  if ((long long)n_tets >= (1LL << 28)) return fail(FB_EINVAL, "too many tets for the packed contribution word");

  const LapTimer lap("device plan");
  h->plan = unsharded_plan(n_nodes, n_tets, n_fixed);
  if (d_tets) {
    FB_TRY(h->tets.alloc((size_t)n_tets));
    FB_HIP(hipMemcpyAsync(h->tets.p, d_tets, sizeof(int4) * (size_t)n_tets, hipMemcpyDeviceToDevice, h->stream));
  } else {
    FB_TRY(h->tets.upload((const int4*)tets, (size_t)n_tets, h->stream));
  }
  lap("elements uploaded");
  {
    // the internal node order (renumber.h): decided from the widest element, built from the rest positions
    bool want = false;
    FB_TRY(renumber_decide(h->stream, renumber_mode(h), n_nodes, n_tets, h->tets.p, h->plan_ws, h->ren, &want));
    if (want) {
      FB_TRY(h->xyz_in.reserve((size_t)3 * n_nodes));
      if (d_xyz64) {
        FB_HIP(hipMemcpyAsync(h->xyz_in.p, d_xyz64, sizeof(double) * 3 * (size_t)n_nodes, hipMemcpyDeviceToDevice, h->stream));
      } else if (d_xyz) {
        FB_TRY(widen_positions(h->stream, 3LL * n_nodes, d_xyz, h->xyz_in.p));
      } else {
        FB_HIP(hipMemcpyAsync(h->xyz_in.p, xyz, sizeof(double) * 3 * (size_t)n_nodes, hipMemcpyHostToDevice, h->stream));
      }
      FB_TRY(renumber_build(h->stream, renumber_mode(h), n_nodes, n_tets, h->tets.p, h->xyz_in.p, h->plan_ws, h->ren));
      if (h->ren.active) {
        FB_TRY(relabel_tets(h->stream, n_tets, h->tets.p, n_nodes, h->ren.d_new_of_old.p));
        FB_TRY(h->x0.alloc((size_t)3 * n_nodes));
        FB_TRY(gather_nodes(h->stream, n_nodes, 3, h->xyz_in.p, h->ren.d_old_of_new.p, h->x0.p));
        h->x0_ready = true;  // (P.local2global -- internal id -> the caller's -- is fetched when an inspection entry point asks: ensure_host_order)
        h->ren_nodes_at_build = n_nodes;
      }
    }
    if (lap.on)
      fprintf(stderr, "[fembrain] node order: widest element %d -> %d (%s%s)\n", h->ren.span_before, h->ren.span_after, h->ren.active ? "renumbered" : "caller's order kept",
              h->ren.active && h->ren.sigma ? ", rows sorted by element count inside windows" : "");
  }
  lap("node order");
  // constraint masks on the device, in the internal order (host: 0.23 ms of loops and two uploads at 1M tets)
  FB_TRY(device_constraint_masks(h->stream, n_nodes, n_fixed, fixed, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->fixed_stage, h->dofmask, h->nodemask));
  h->masks_ready = true;
  lap("constraints");
  DevicePlan D = handle_plan_outputs(h);
  D.ucnt_keep = &h->d_ucnt;
  // (the widest element was measured for the node order: FB_RENUMBER_OFF skips that pass and leaves the sort its 64-bit keys)
  const int span = renumber_mode(h) == FB_RENUMBER_OFF ? -1 : (h->ren.active ? h->ren.span_after : h->ren.span_before);
  const int rc = build_plan_device(h->stream, n_nodes, n_tets, h->tets.p, D, h->plan_ws, nullptr, span);
  release_large_plan_ws(h);
  FB_TRY(bad_tet_error(rc, D.first_bad_tet, tets, n_nodes));
  adopt_device_plan(h, D, 1);
  h->csr_ready = true;
  return FB_OK;
}

// global node ids of a rank's elements -> local ids: owned nodes first, then the halo in ascending global order
__global__ void __launch_bounds__(kBlock) k_tets_to_local(int n_tets, int4* __restrict__ tets, int node_lo, int n_owned, const int* __restrict__ halo, int n_halo) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_tets) return;
  int4 t = tets[e];
  int* v = &t.x;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int g = v[i];
    if (g >= node_lo && g < node_lo + n_owned) { v[i] = g - node_lo; continue; }
    int lo = 0, hi = n_halo;  // lower bound; g is in the list by construction
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (halo[mid] < g) lo = mid + 1; else hi = mid;
    }
    v[i] = n_owned + lo;
  }
  tets[e] = t;
}

// One rank's share of a sharded system: partition, local numbering, halo and send lists on the host (build_fem_partition: one
// pass over the element list), then pattern / SELL-64 / contribution lists of the owned rows on the device -- the part that
// took 68-75 ms per rank at 1M tets on the host.
int build_shard_plan_on_device(fb_fem_s* h, int n_nodes, int n_tets, const int* tets, int n_fixed, const int* fixed, int n_ranks, int rank,
                               const int* splits, const double* xyz) {
  FemPlan& P = h->plan;
  const LapTimer lap("shard plan");
  // the partition (elements with an owned node, halo, send lists, local numbering) is computed on the device from the uploaded
  // list, be it the rank's own elements or the whole mesh; on the host only for more than 64 ranks or FEMBRAIN_PARTITION_DEVICE=0
  const bool on_device = n_ranks <= 64 && !(getenv("FEMBRAIN_PARTITION_DEVICE") && atoi(getenv("FEMBRAIN_PARTITION_DEVICE")) == 0);
  DevBuf<int> d_halo;
  if (on_device) {
    FB_TRY(begin_fem_partition(P, n_nodes, n_tets, n_ranks, rank, splits));
    FB_TRY(h->tets.upload((const int4*)tets, (size_t)n_tets, h->stream));
    if (renumber_mode(h) == FB_RENUMBER_ON) {
      // Opt-in on a sharded handle (include/fembrain_hip.h, "Node numbering"): every rank derives the SAME internal order from the whole
      // mesh, relabels its copy of the element list, and the ranks then own contiguous ranges of THAT order -- slabs of the body with
      // two neighbours each, whatever the caller's numbering.  Everything below works on internal ids; l2c maps back at the ABI.
      bool want = false;
      FB_TRY(renumber_decide(h->stream, FB_RENUMBER_ON, n_nodes, n_tets, h->tets.p, h->plan_ws, h->ren, &want));
      if (want) {
        FB_TRY(h->xyz_in.reserve((size_t)3 * n_nodes));
        FB_HIP(hipMemcpyAsync(h->xyz_in.p, xyz, sizeof(double) * 3 * (size_t)n_nodes, hipMemcpyHostToDevice, h->stream));
        FB_TRY(renumber_build(h->stream, FB_RENUMBER_ON, n_nodes, n_tets, h->tets.p, h->xyz_in.p, h->plan_ws, h->ren));
      }
      if (h->ren.active) {
        FB_TRY(relabel_tets(h->stream, n_tets, h->tets.p, n_nodes, h->ren.d_new_of_old.p));
        FB_TRY(h->ren.host_maps(h->stream));
        h->order_sum = 0;
        for (int l = 0; l < n_nodes; l++) h->order_sum += (unsigned long long)(l + 1) * (unsigned long long)(h->ren.old_of_new[l] + 7);
      }
      lap("node order");
    }
    DevicePartition dp;
    const int rc = device_partition(h->stream, n_tets, h->tets, n_nodes, n_ranks, rank, P.splits, dp, h->plan_ws);
    FB_TRY(bad_tet_error(rc, dp.first_bad_tet, tets, n_nodes));
    P.n_tets = dp.n_kept;
    P.tet_global = dp.tet_global;
    P.n_owned_corners = dp.owned_corners;
    set_partition_halo(P, dp.halo);
    P.send_off = dp.send_off;
    P.send_local = dp.send_local;
  } else {
    FB_TRY(build_fem_partition(P, n_nodes, n_tets, tets, n_ranks, rank, splits, false));
  }
  lap(on_device ? "partition (device)" : "partition (host)");
  if (h->ren.active) {
    // caller ids of the local nodes, and the constrained DOFs in internal ids (ascending again)
    h->l2c.resize((size_t)P.n_local);
    for (int l = 0; l < P.n_local; l++) h->l2c[l] = h->ren.old_of_new[P.local2global[l]];
    FB_TRY(check_fixed_dofs(n_fixed, fixed, 3LL * n_nodes));
    FB_TRY(plan_set_constraints(P, n_fixed, fixed_to_internal(h, n_fixed, fixed).data()));
  } else {
    FB_TRY(plan_set_constraints(P, n_fixed, fixed));
  }
  lap("constraints");
  if (P.n_halo > 0) FB_TRY(d_halo.upload(P.local2global.data() + P.n_owned, (size_t)P.n_halo, h->stream));
  if (on_device) {
    // numbered locally already
  } else if (P.tets.empty()) {  // host partition of the caller's own list: local numbering on the device
    FB_TRY(h->tets.upload((const int4*)tets, (size_t)P.n_tets, h->stream));
    hipLaunchKernelGGL(k_tets_to_local, dim3(ceil_div(P.n_tets, kBlock)), dim3(kBlock), 0, h->stream, P.n_tets, h->tets.p, P.node_lo, P.n_owned, d_halo.p, P.n_halo);
    FB_HIP(hipGetLastError());
  } else {
    FB_TRY(h->tets.upload((const int4*)P.tets.data(), (size_t)P.n_tets, h->stream));
  }
  lap("element upload");
  PlanShard sh;
  sh.n_rows = P.n_owned; sh.node_lo = P.node_lo; sh.n_global = P.n_global; sh.d_halo = d_halo.p; sh.n_halo = P.n_halo;
  sh.n_pairs = 4 * P.n_owned_corners + P.n_owned;
  DevicePlan D = handle_plan_outputs(h);
  D.halo_base = &h->halo_base;
  const int rc = build_plan_device(h->stream, P.n_local, P.n_tets, h->tets.p, D, h->plan_ws, &sh);
  release_large_plan_ws(h);
  FB_TRY(rc);
  adopt_device_plan(h, D, 2);  // the halo form
  return FB_OK;
}

// rest state of a device-built plan; the kernel reports the first flat element (see build)
int rest_state_checked(fb_fem_s* h) {
  const int none = 0x7fffffff;
  FB_TRY(h->flat_flag.alloc(1));
  FB_HIP(hipMemcpyAsync(h->flat_flag.p, &none, sizeof(int), hipMemcpyHostToDevice, h->stream));
  FB_TRY(launch_rest(h, h->flat_flag.p));
  int first = none;
  FB_TRY(h->flat_flag.download(&first, 1, h->stream));
  if (first != none)
    return fail(FB_EINVAL, "element %d has zero (or non-finite) rest volume", h->plan.tet_global.empty() ? first : h->plan.tet_global[first]);
  return FB_OK;
}

int build(fb_fem_s* h, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed, const int* fixed, int n_ranks,
          int rank, const int* splits, const DeviceTetMesh* dm = nullptr) {
  begin_mesh_generation(h);
  SlackScope slack(handle_slack(h, n_nodes, n_tets));
  if (n_ranks == 1 && fixed != h->fixed_caller.data()) h->fixed_caller.assign(fixed, fixed + n_fixed);
  if (h->prm.matrix_precision == FB_MATRIX_AUTO) h->f64 = auto_matrix_f64(h, n_nodes, n_ranks);
  h->last_resync_path = FB_RESYNC_FULL;
  const LapTimer lap("build");
  const bool want_device = !(getenv("FEMBRAIN_PLAN_DEVICE") && atoi(getenv("FEMBRAIN_PLAN_DEVICE")) == 0);
  h->device_plan = (want_device || dm) && (n_ranks == 1 || !dm);
  h->host_pattern = !h->device_plan;
  if (h->device_plan) {
    const int rc = n_ranks > 1 ? build_shard_plan_on_device(h, n_nodes, n_tets, tets, n_fixed, fixed, n_ranks, rank, splits, xyz)
                               : build_plan_on_device(h, n_nodes, n_tets, tets, n_fixed, fixed, xyz, dm ? dm->tets : nullptr, dm ? dm->xyz : nullptr, dm ? dm->xyz64 : nullptr);
    if (dm && rc != FB_OK) return rc;
    if (rc == FB_ENOMEM) {  // no room for the sort's temporaries: the host builder needs none on the device
      (void)hipGetLastError();
      h->device_plan = false;
      h->host_pattern = true;
      begin_mesh_generation(h);  // (the host builder works in the caller's order, and puts positions and masks in place itself)
    } else if (rc != FB_OK) {
      return rc;
    }
    lap("device plan");
  }
  if (!h->device_plan) {
    h->c16 = 0;
    FB_TRY(build_fem_plan(h->plan, n_nodes, n_tets, tets, n_fixed, fixed, n_ranks, rank, splits));
    lap("host plan");
  }
  // A flat element makes inverse4x4 (corotationalLinearFEM.cpp:529-572) divide by zero; the reference then carries
  // inf/NaN into the step silently.  Refuse it here instead (checked on this rank's elements, rest geometry; a handle
  // whose plan was built on the device lets the rest-state kernel look, below).
  for (int e = 0; e < (h->device_plan ? 0 : h->plan.n_tets); e++) {
    const double* p[4];
    for (int k = 0; k < 4; k++)
      p[k] = xyz + 3 * (size_t)(h->device_plan ? tets[4 * (size_t)e + k] : h->plan.local2global[h->plan.tets[4 * (size_t)e + k]]);
    double a[3], b[3], c[3];
    for (int k = 0; k < 3; k++) { a[k] = p[1][k] - p[0][k]; b[k] = p[2][k] - p[0][k]; c[k] = p[3][k] - p[0][k]; }
    const double det = a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    if (!(det != 0.0) || !std::isfinite(det))
      return fail(FB_EINVAL, "element %d has zero (or non-finite) rest volume", h->plan.tet_global.empty() ? e : h->plan.tet_global[e]);
  }
  lap("volume check");
  if (has_material_map(h) && !h->map_from_delta) {  // a new mesh: every element is material 0 again, the table stays (a delta re-sync swaps its own map in afterwards)
    FB_TRY(h->mat_ids.alloc((size_t)std::max(1, n_tets)));
    FB_TRY(h->mat_ids.zero(h->stream));
    h->mat_hi = 0;
  }
  FB_TRY(upload_plan(h, xyz, dm ? dm->xyz : nullptr, dm ? dm->xyz64 : nullptr));
  lap("upload");
  if (h->device_plan) {
    FB_TRY(rest_state_checked(h));
  } else {
    FB_TRY(launch_rest(h));
    FB_HIP(hipStreamSynchronize(h->stream));
  }
  lap("rest state");
  return FB_OK;
}


// Collective, BEFORE the rank-local build: FB_RENUMBER_AUTO on a sharded handle ("the same contiguous-range rule after an
// RCM / space-filling-curve renumbering").  Equal ranges of the caller's ids are slabs of the body only while the caller numbers plane
// by plane; after cuts (nodes appended at the end: VolMesh.cpp:1086-1091) or on a TetGen mesh every rank is a neighbour of every other
// and half the mesh is halo (profiles/r04_numbering_probe_after.json: 7 neighbours and 128k halo nodes per rank at 8 ranks, against 2 and
// 6k).  Every rank counts the ranks its own elements couple it to under the caller's numbering and sums a checksum of the element list
// it was handed; the ranks all-gather (neighbours, sizes, checksum, mode) and switch the internal order on -- all of them or none --
// when some rank would have more than two neighbours (or, from 8,192 nodes, most of its elements reaching into another rank) AND every
// rank holds the same whole mesh (the internal order is derived from all
// nodes and all elements; a rank that was handed its own elements only keeps the caller's numbering, as before).  One pass over the
// element list on the host (2 ms per million tets) and one all-gather of 40 bytes.
struct ShardOrderVote { int neighbours, n_nodes, n_tets, mode; unsigned long long sum; int splits_sum, own_elements, boundary_elements, pad; };
int vote_shard_order(fb_fem_s* h, int n_nodes, int n_tets, const int* tets, int n_ranks, int rank, const int* splits) {
  h->shard_auto_on = false;
  h->shard_vote_neighbours = 0;
  if (!h->comm || n_ranks < 2) return FB_OK;
  ShardOrderVote mine;
  memset(&mine, 0, sizeof mine);
  int mode = h->prm.renumber > 0 ? FB_RENUMBER_ON : (h->prm.renumber < 0 ? FB_RENUMBER_OFF : FB_RENUMBER_AUTO);
  if (const char* e = getenv("FEMBRAIN_RENUMBER")) mode = atoi(e) != 0 ? FB_RENUMBER_ON : FB_RENUMBER_OFF;
  mine.mode = mode; mine.n_nodes = n_nodes; mine.n_tets = n_tets; mine.neighbours = -1;
  if (mode == FB_RENUMBER_AUTO && tets && n_tets > 0 && n_nodes > 0 && n_ranks <= 64) {
    // (bad ranges, bad ids: the build refuses them with its own message; this rank then votes "unknown")
    shard_neighbour_count(n_nodes, n_tets, tets, n_ranks, rank, splits, &mine.neighbours, &mine.sum, &mine.splits_sum, &mine.own_elements, &mine.boundary_elements);
  }
  std::vector<ShardOrderVote> all((size_t)n_ranks);
  FB_TRY(comm_allgather_bytes(h->comm, &mine, all.data(), sizeof mine, h->stream));
  bool same = true, any_wide = false;
  int most = 0;
  for (int q = 0; q < n_ranks; q++) {
    same = same && all[q].mode == FB_RENUMBER_AUTO && all[q].neighbours >= 0 && all[q].n_nodes == all[0].n_nodes && all[q].n_tets == all[0].n_tets &&
           all[q].sum == all[0].sum && all[q].splits_sum == all[0].splits_sum;
    // more than two neighbour ranks; or (meshes of a size AUTO renumbers at all) most of a rank's elements reach into another rank -- the
    // two-rank form of the same disorder, where "every rank a neighbour" still means one
    any_wide = any_wide || all[q].neighbours > 2 || (n_nodes >= kRenumberMinNodes && 2LL * all[q].boundary_elements > all[q].own_elements);
    most = std::max(most, all[q].neighbours);
  }
  h->shard_vote_neighbours = most;
  h->shard_auto_on = same && any_wide;
  if (LapTimer::enabled())
    fprintf(stderr, "[fembrain] rank %d: node-order vote: %d neighbour ranks here, %d at most, same mesh on every rank: %s -> %s\n", rank, mine.neighbours, most, same ? "yes" : "no",
            h->shard_auto_on ? "internal slab order" : "caller's numbering");
  return FB_OK;
}

// collective: a renumbered sharded handle works only if every rank derived the same internal order (from the same whole mesh)
int agree_on_node_order(fb_fem_s* h) {
  if (!h->comm || h->comm->n_ranks < 2) return FB_OK;
  const int R = h->comm->n_ranks;
  std::vector<unsigned long long> sums((size_t)R);
  FB_TRY(comm_allgather_bytes(h->comm, &h->order_sum, sums.data(), sizeof(unsigned long long), h->stream));
  for (int q = 0; q < R; q++)
    if (sums[q] != sums[0])
      return fail(FB_EINVAL, "the ranks derived different node orders (FB_RENUMBER_ON on a sharded handle needs the WHOLE mesh -- all nodes, all elements -- on every rank, and the same setting)");
  return FB_OK;
}

// collective: every rank of the communicator creates its handle at the same point of its program
int attach_p2p(fb_fem_s* h) {
  const FemPlan& P = h->plan;
  FB_TRY(p2p_attach(h->comm, P.n_local - P.n_owned, P.halo_off.data(), h->stream, &h->p2p));
  if (!h->p2p) return FB_OK;
  h->xch_mode = FB_XCH_P2P_FUSED;
  if (const char* e = getenv("FEMBRAIN_XCH_MODE")) {  // 2 / 3 / 4: how much of the exchange rides inside the PCG kernels
    const int m = atoi(e);
    if (m >= FB_XCH_COLLECTIVE && m <= FB_XCH_P2P_FUSED) h->xch_mode = m;
  }
  FB_TRY(h->send_off_dev.upload(P.send_off, h->stream));
  FB_TRY(h->halo_off_dev.upload(P.halo_off, h->stream));
  // slices with a halo column are done after the halo wait
  if (h->device_plan) {
    FB_TRY(h->slice_halo.alloc((size_t)std::max(1, P.n_slices)));
    hipLaunchKernelGGL(k_slice_halo, dim3(ceil_div(std::max(1, P.n_slices), kWavesPerBlock)), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->slice_off.p,
                       h->colidx.p, h->slice_halo.p);
    FB_HIP(hipGetLastError());
  } else {
    std::vector<unsigned char> sh((size_t)std::max(1, P.n_slices), 0);
    for (int sl = 0; sl < P.n_slices; sl++)
      for (size_t k = (size_t)P.slice_off[sl] * kSliceRows; k < (size_t)P.slice_off[sl + 1] * kSliceRows && !sh[sl]; k++) sh[sl] = P.colidx[k] >= P.n_owned;
    FB_TRY(h->slice_halo.upload(sh, h->stream));
  }
  if (P.send_local.empty()) FB_TRY(h->send_local.alloc(1));
  return FB_OK;
}

int prewarm_delta(fb_fem_s* h, int n_fixed, const int* fixed);

int create_common(fb_fem_t* out, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed, const int* fixed,
                  const fb_fem_params* params, int n_ranks, int rank, const int* splits, fb_comm_t comm, const DeviceTetMesh* dm = nullptr) {
  if (!out || (!dm && (!xyz || !tets)) || !params) return fail(FB_EINVAL, "null argument");
  if (dm && dm->device != params->device) return fail(FB_EINVAL, "the polygonizer lives on device %d, the FEM handle is asked for device %d", dm->device, params->device);
  if (n_fixed < 0 || (n_fixed > 0 && !fixed)) return fail(FB_EINVAL, "bad constrained DOF list");
  if (params->integrator != FB_INTEGRATOR_VOLUME_CONSERVING && params->integrator != FB_INTEGRATOR_NEWMARK) return fail(FB_EINVAL, "unknown integrator %d", params->integrator);
  if (!(params->timestep > 0) || !(params->E > 0) || !(params->rho > 0) || !(params->nu > -1.0 && params->nu < 0.5) ||
      !std::isfinite(params->timestep) || !std::isfinite(params->E) || !std::isfinite(params->rho) ||
      !std::isfinite(params->damping_mass) || !std::isfinite(params->damping_stiffness))
    return fail(FB_EINVAL, "bad material / timestep / damping parameters");
  if (params->pcg_variant != FB_PCG_MERGED && params->pcg_variant != FB_PCG_REFERENCE && params->pcg_variant != FB_PCG_PERSISTENT &&
      params->pcg_variant != FB_PCG_BLOCK_JACOBI)
    return fail(FB_EINVAL, "unknown pcg_variant %d", params->pcg_variant);
  if (n_ranks > 1 && !comm) return fail(FB_EINVAL, "sharded handle needs a communicator");
  if (comm && (comm->n_ranks != n_ranks || comm->rank != rank)) return fail(FB_EINVAL, "communicator rank/size does not match the handle");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FB_EDEVICE, "no HIP device visible");
  if (params->device < 0 || params->device >= ndev) return fail(FB_EINVAL, "device %d out of range (%d visible)", params->device, ndev);
  FB_HIP(hipSetDevice(params->device));
  fb_fem_s* h = new fb_fem_s;
  h->prm = *params;
  h->comm = comm;  // a one-rank communicator with a live RCCL handle still runs the collectives (plumbing test)
  if (params->matrix_precision != FB_MATRIX_F32 && params->matrix_precision != FB_MATRIX_F64 && params->matrix_precision != FB_MATRIX_AUTO) {
    delete h;
    return fail(FB_EINVAL, "unknown matrix_precision %d", params->matrix_precision);
  }
  h->f64 = params->matrix_precision == FB_MATRIX_F64;  // (FB_MATRIX_AUTO: build() decides by size, at every re-sync again)
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, params->device) == hipSuccess) h->n_cu_device = prop.multiProcessorCount;
  }
  h->lambda = (params->nu * params->E) / ((1 + params->nu) * (1 - 2 * params->nu));
  h->mu = params->E / (2 * (1 + params->nu));
  h->mat_E.assign(1, params->E); h->mat_nu.assign(1, params->nu); h->mat_rho.assign(1, params->rho);  // the one-entry table of the params
  int rc = FB_OK;
  do {
   // collective, before anything rank-local can fail: the node order of a sharded handle under FB_RENUMBER_AUTO
   if (comm && comm->n_ranks > 1 && (rc = vote_shard_order(h, n_nodes, n_tets, tets, n_ranks, rank, splits)) != FB_OK) break;
   // rank-local set-up; a failure here (stream, events, pinned memory, the build) must still reach the agreement below -- the other ranks
   // are on their way into that all-gather
   do {
    // FEMBRAIN_CU_MASK=first:count -- the handle's stream runs on `count` CUs from bit `first` of the CU mask only (development and test
    // aid: two processes on one GPU, each with a persistent kernel on its own half of the CUs); the persistent grid follows
    if (const char* cm = getenv("FEMBRAIN_CU_MASK")) {
      int first = 0, count = 0;
      if (sscanf(cm, "%d:%d", &first, &count) != 2 || first < 0 || count < 8 || first + count > 512) { rc = fail(FB_EINVAL, "FEMBRAIN_CU_MASK=first:count"); break; }
      uint32_t mask[16];
      memset(mask, 0, sizeof mask);
      for (int b = first; b < first + count; b++) mask[b >> 5] |= 1u << (b & 31);
      if (hipExtStreamCreateWithCUMask(&h->stream, 16, mask) != hipSuccess) { rc = fail(FB_EDEVICE, "hipExtStreamCreateWithCUMask failed"); break; }
      h->cu_limit = count;
    } else
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(FB_EDEVICE, "hipStreamCreate failed"); break; }
    for (auto& e : h->ev) if (hipEventCreate(&e) != hipSuccess) rc = fail(FB_EDEVICE, "hipEventCreate failed");
    for (auto& e : h->ev_batch) if (hipEventCreate(&e) != hipSuccess) rc = fail(FB_EDEVICE, "hipEventCreate failed");
    for (auto& e : h->ev_p) if (hipEventCreate(&e) != hipSuccess) rc = fail(FB_EDEVICE, "hipEventCreate failed");
    if (rc != FB_OK) break;
    if (hipHostMalloc((void**)&h->st_host, 2 * sizeof(CGState), hipHostMallocDefault) != hipSuccess) { rc = fail(FB_ENOMEM, "hipHostMalloc failed"); break; }
    if (const char* e = getenv("FEMBRAIN_GRAPH")) h->use_graph = atoi(e) != 0;
    rc = build(h, n_nodes, xyz, n_tets, tets, n_fixed, fixed, n_ranks, rank, splits, dm);
    // a mesh that will be cut: the workspace of fb_fem_resync_delta now, not inside the first cut
    if (rc == FB_OK && h->prm.expect_cuts && n_ranks == 1 && h->device_plan) rc = prewarm_delta(h, n_fixed, fixed);
   } while (0);
    if (comm && comm->n_ranks > 1) {  // creation is collective: the ranks agree on the outcome so far before the collective attach
      rc = agree_on_outcome(comm, h->stream, rc, "handle creation failed on rank %d (code %d)");
      if (rc == FB_OK) rc = agree_on_node_order(h);
    }
    if (rc == FB_OK && comm && comm->n_ranks > 1) rc = attach_p2p(h);
    if (rc == FB_OK && comm && comm->n_ranks > 1) rc = attach_pipe_shard(h);
  } while (0);
  if (rc != FB_OK) {
    std::string keep = last_error();
    fb_fem_destroy(h);
    last_error() = keep;
    return rc;
  }
  *out = h;
  return FB_OK;
}

}  // namespace

extern "C" {

int fb_fem_create(fb_fem_t* out, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs,
                  const int* fixed_dofs, const fb_fem_params* params) {
  return create_common(out, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, params, 1, 0, nullptr, nullptr);
}

int fb_fem_create_from_poly(fb_fem_t* out, fb_poly_t poly, int n_fixed_dofs, const int* fixed_dofs, const fb_fem_params* params) {
  DeviceTetMesh dm;
  FB_TRY(poly_device_tetmesh(poly, &dm));
  if (dm.n_tets < 1) return fail(FB_EINVAL, "the polygonizer holds no tets");
  return create_common(out, dm.n_vertices, nullptr, dm.n_tets, nullptr, n_fixed_dofs, fixed_dofs, params, 1, 0, nullptr, nullptr, &dm);
}

int fb_fem_create_sharded(fb_fem_t* out, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs,
                          const int* fixed_dofs, const fb_fem_params* params, int n_ranks, int rank, const int* node_splits,
                          fb_comm_t comm) {
  return create_common(out, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, params, n_ranks, rank, node_splits, comm);
}

int fb_fem_destroy(fb_fem_t h) {
  if (!h) return FB_OK;
  (void)hipSetDevice(h->prm.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (auto& e : h->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : h->ev_batch) if (e) (void)hipEventDestroy(e);
  for (auto& e : h->ev_p) if (e) (void)hipEventDestroy(e);
  if (h->st_host) (void)hipHostFree(h->st_host);
  if (h->p2p) p2p_detach(h->p2p);
  release_shard_persist(h);
  drop_graph(h);
  DevBuf<double>* vecs[] = {&h->q, &h->qvel, &h->fext, &h->fint, &h->rhs, &h->x, &h->r, &h->d, &h->Ad, &h->invdiag, &h->tmp};
  for (auto* v : vecs) v->release();
  hipStream_t s = h->stream;
  if (h->side) { (void)hipStreamSynchronize(h->side); (void)hipStreamDestroy(h->side); }
  for (auto& e : h->ev_side) if (e) (void)hipEventDestroy(e);
  delete h;  // frees the remaining device buffers
  if (s) (void)hipStreamDestroy(s);
  return FB_OK;
}

// collective re-sync of a sharded handle; node_splits NULL keeps the handle's ranges when the node count is unchanged, else equal ranges
static int resync_sharded(fb_fem_t h, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs, const int* fixed_dofs,
                          const int* node_splits) {
  // every rank re-syncs at the same point of its program; the peer-to-peer inboxes are sized by the halo and are attached again
  ResyncScope scope(h);
  const int n_ranks = h->plan.n_ranks, rank = h->plan.rank;
  const std::vector<int> kept = h->plan.splits;
  if (!node_splits && n_nodes == h->plan.n_global) node_splits = kept.data();
  // build() is rank-local (a bad node id or a flat element after a cut, no memory ...); what follows is collective.  The ranks
  // agree on the outcome first: if any of them failed, none enters the collective attach -- all stay poisoned and return an
  // error, instead of the healthy ones waiting in an all-gather for a rank that has left.
  FB_TRY(vote_shard_order(h, n_nodes, n_tets, tets, n_ranks, rank, node_splits));  // (collective; before the rank-local build)
  const int rc_mine = build(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, n_ranks, rank, node_splits);
  if (h->comm && h->comm->n_ranks > 1)
    FB_TRY(agree_on_outcome(h->comm, h->stream, rc_mine, "re-sync failed on rank %d (code %d); this rank's handle is unusable until a re-sync succeeds on every rank"));
  else
    FB_TRY(rc_mine);
  FB_TRY(agree_on_node_order(h));
  const int mode = h->xch_mode;
  if (h->p2p) { p2p_detach(h->p2p); h->p2p = nullptr; }
  if (h->comm && h->comm->n_ranks > 1) FB_TRY(attach_p2p(h));
  if (h->comm && h->comm->n_ranks > 1) FB_TRY(attach_pipe_shard(h));
  if (h->p2p && mode >= FB_XCH_P2P) h->xch_mode = mode;   // the form chosen before the re-sync stays
  else if (mode == FB_XCH_COLLECTIVE) h->xch_mode = FB_XCH_COLLECTIVE;
  scope.commit();
  return FB_OK;
}

int fb_fem_resync_sharded(fb_fem_t h, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs, const int* fixed_dofs,
                          const int* node_splits) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  FB_HIP(hipSetDevice(h->prm.device));
  if (!xyz || !tets) return fail(FB_EINVAL, "null mesh");
  FB_HIP(hipStreamSynchronize(h->stream));
  if (h->plan.n_ranks == 1) {
    if (node_splits && (node_splits[0] != 0 || node_splits[1] != n_nodes)) return fail(FB_EINVAL, "node splits must cover [0,%d)", n_nodes);
    return fb_fem_resync(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs);
  }
  return resync_sharded(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, node_splits);
}

int fb_fem_resync(fb_fem_t h, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs, const int* fixed_dofs) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  FB_HIP(hipSetDevice(h->prm.device));
  if (!xyz || !tets) return fail(FB_EINVAL, "null mesh");
  FB_HIP(hipStreamSynchronize(h->stream));
  if (h->plan.n_ranks > 1) return resync_sharded(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, nullptr);
  ResyncScope scope(h);
  motion_clear(h->motion);  // (a state reset: the moved DOFs and the grasp go with the state)
  FB_TRY(build(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, 1, 0, nullptr));
  scope.commit();
  return FB_OK;
}

// ---- fb_fem_resync_delta (delta.h) ----
namespace {
// The full builder from the device copy of the new mesh in the caller's numbering (no sorted list to update, or the new mesh is to
// get a new node order): what fb_fem_resync does, without the host hop.
int resync_delta_rebuild(fb_fem_s* h, int n_old, int n_new, int n_fixed, const int* fixed) {
  hipStream_t s = h->stream;
  MeshDelta& D = h->delta;
  const int nt_old = D.n_tets_old, nt_new = D.n_tets_new();
  // the old element list and the rest positions in the caller's numbering
  FB_TRY(h->tets_caller.alloc((size_t)nt_old));
  FB_HIP(hipMemcpyAsync(h->tets_caller.p, h->tets.p, sizeof(int4) * (size_t)nt_old, hipMemcpyDeviceToDevice, s));
  if (h->ren.active) FB_TRY(relabel_tets(s, nt_old, h->tets_caller.p, n_old, h->ren.d_old_of_new.p));
  FB_TRY(h->tets_next.alloc((size_t)nt_new));
  FB_TRY(delta_tets(s, D, h->tets_caller.p, nullptr, h->tets_next.p));
  FB_TRY(h->x0_next.alloc((size_t)3 * n_new));
  if (h->ren.active) FB_TRY(scatter_nodes(s, n_old, 3, h->x0.p, h->ren.d_old_of_new.p, h->x0_next.p));
  else FB_HIP(hipMemcpyAsync(h->x0_next.p, h->x0.p, sizeof(double) * 3 * (size_t)n_old, hipMemcpyDeviceToDevice, s));
  if (D.n_new_nodes) FB_HIP(hipMemcpyAsync(h->x0_next.p + 3 * (size_t)n_old, D.new_xyz.p, sizeof(double) * 3 * (size_t)D.n_new_nodes, hipMemcpyDeviceToDevice, s));
  DeviceTetMesh dm;
  dm.device = h->prm.device; dm.n_vertices = n_new; dm.n_tets = nt_new; dm.xyz = nullptr;
  dm.tets = reinterpret_cast<const uint4*>(h->tets_next.p); dm.xyz64 = h->x0_next.p;
  FB_TRY(build(h, n_new, nullptr, nt_new, nullptr, n_fixed, fixed, 1, 0, nullptr, &dm));
  h->last_resync_path = FB_RESYNC_DELTA_REBUILT;
  return FB_OK;
}

// device_src: removed / added / new_xyz are device arrays (fb_fem_cut; no element changed in place)
// force_rebuild: the full builder whatever there is to merge into (refresh_node_order)
int resync_delta_apply(fb_fem_s* h, int n_removed, const int* removed, int n_changed, const int* changed_ids, const int* changed_nodes, int n_added, const int* added,
                       int n_new_nodes, const double* new_xyz, int n_fixed, const int* fixed, bool device_src, bool force_rebuild) {
  const LapTimer lap("delta re-sync");
  hipStream_t s = h->stream;
  MeshDelta& D = h->delta;
  PlanWorkspace& W = h->plan_ws;
  const int n_old = h->plan.n_global, nt_old = h->plan.n_tets, n_new = n_old + n_new_nodes;
  SlackScope slack(handle_slack(h, n_new, nt_old - n_removed + n_added));
  // (the node order stays for the merged path to extend; csr_ready says below whether there is a plan to merge into)
  begin_mesh_generation(h, kKeepOrder | kKeepCsr);
  if (fixed != h->fixed_caller.data()) h->fixed_caller.assign(fixed, fixed + n_fixed);
  if (device_src)
    FB_TRY(delta_upload_device(s, nt_old, n_removed, removed, n_added, reinterpret_cast<const int4*>(added), n_new_nodes, new_xyz, D, W));
  else
    FB_TRY(delta_upload(s, nt_old, n_removed, removed, n_changed, changed_ids, changed_nodes, n_added, added, n_new_nodes, new_xyz, D, W));
  const int nt_new = D.n_tets_new();
  if (has_material_map(h)) {
    // the element map through the change, on the device: kept and changed elements keep their material in order, the pieces of a cut
    // inherit their parent's (k_cut_pieces' cut_tets / piece_off), other added elements get 0.  Swapped in when the re-sync is complete.
    FB_TRY(h->mat_ids_next.alloc((size_t)std::max(1, nt_new)));
    // (device_src with nothing added: a part's elements taken out, remove_elements_device -- no cut stands behind it)
    if (device_src && n_added) FB_TRY(delta_element_bytes(s, D, h->mat_ids.p, h->mat_ids_next.p, h->cut.n_cut, h->cut.cut_tets.p, h->cut.piece_off.p, h->cut.pcount.p));
    else FB_TRY(delta_element_bytes(s, D, h->mat_ids.p, h->mat_ids_next.p));
  }
  lap("change uploaded");
  const char* env = getenv("FEMBRAIN_RESYNC_DELTA");
  bool merge = h->csr_ready && !force_rebuild && !(env && !strcmp(env, "rebuild"));
  // A renumbered handle keeps the order it has while nodes are added -- new nodes are merged in, old ones stay where they are although
  // the cut has changed how many elements sit on them, so rows of unlike length come to share a slice and the matrix pads.  Measured at
  // 1.1M tets (tools/probe_resync_delta.py): 9 % more nodes merged in, 42.5 us per PCG iteration against 30.6 in a fresh order -- 26 ms per
  // step -- where the full builder from the device copy of the mesh costs 2.9 ms once.  So once kFreshOrderPercent more nodes have come
  // than the order was built for, the change gets a fresh order (FEMBRAIN_FRESH_ORDER_PERCENT overrides: the tests keep the merged
  // path busy with larger changes)
  if (merge && h->ren.active && (long long)n_new * 100 > (long long)h->ren_nodes_at_build * (100 + fresh_order_percent())) merge = false;
  // FB_MATRIX_AUTO is decided again at every re-sync: a mesh that has grown across the size rule gets its values in the other width,
  // which the full builder allocates
  if (merge && h->prm.matrix_precision == FB_MATRIX_AUTO && auto_matrix_f64(h, n_new, 1) != h->f64) merge = false;
  const int mode = renumber_mode(h);
  int span = -1;
  double mean = 0.0;
  if (merge && !h->ren.active && mode != FB_RENUMBER_OFF) {
    // A handle in the caller's order: would the full builder try a new node order for the new mesh (renumber_decide)?  Then it is to
    // decide.  The widest element of the new list: the kept elements are no wider than before, so the new ones settle it unless
    // the old widest element was removed -- measured over the whole new list, as the builder would.
    FB_TRY(h->tets_next.alloc((size_t)nt_new));
    FB_TRY(delta_tets(s, D, h->tets.p, nullptr, h->tets_next.p));
    FB_TRY(tet_span_device(s, nt_new, h->tets_next.p, n_new, nullptr, W, &span, &mean));
    if (mode == FB_RENUMBER_ON || (n_new >= kRenumberMinNodes && span > renumber_span_limit(n_new))) merge = false;
  }
  if (!merge) {
    h->map_from_delta = true;  // (the full builder leaves the map alone: the old one is still being read by the kernels queued above)
    const int rc = resync_delta_rebuild(h, n_old, n_new, n_fixed, fixed);
    h->map_from_delta = false;
    // (also where the builder failed half way: the handle is poisoned then and launches nothing until a re-sync succeeds, but the map's
    // length follows the element count the plan may already have)
    if (has_material_map(h)) h->mat_ids.swap(h->mat_ids_next);
    return rc;
  }

  // ---- the node order ----
  if (h->ren.active) {
    if (n_new_nodes) {
      FB_TRY(delta_node_order(s, D, n_old, h->ren.geom, h->ren.d_keys.p, h->ren.d_old_of_new.p, h->map_next_a, h->map_next_b, W, h->ren.sigma ? h->ren.n_windows : 0,
                              h->ren.sigma ? h->ren.d_win_keys.p : nullptr));
      h->ren.d_old_of_new.swap(h->map_next_a);
      h->ren.d_new_of_old.swap(h->map_next_b);
      h->ren.d_keys.swap(D.node_keys);
      h->ren.n = n_new;
      h->ren.old_of_new.clear();
      h->ren.new_of_old.clear();
    }
    FB_TRY(delta_relabel_nodes(s, D, n_new, h->ren.d_new_of_old.p));
    FB_TRY(h->tets_next.alloc((size_t)nt_new));
    FB_TRY(delta_tets(s, D, h->tets.p, D.mapped ? D.imap.p : nullptr, h->tets_next.p));
    h->span_stale = true;  // (the widest element under the merged order is measured when fb_fem_renumbering asks: a pass and a wait saved here)
  } else {
    h->ren.clear();
    if (mode != FB_RENUMBER_OFF) { h->ren.span_before = h->ren.span_after = span; h->ren.mean_before = h->ren.mean_after = mean; }
    else {
      FB_TRY(h->tets_next.alloc((size_t)nt_new));
      FB_TRY(delta_tets(s, D, h->tets.p, nullptr, h->tets_next.p));
    }
  }
  h->tets.swap(h->tets_next);
  FB_TRY(h->x0_next.alloc((size_t)3 * n_new));
  FB_TRY(delta_positions(s, D, n_old, h->x0.p, h->x0_next.p));
  h->x0.swap(h->x0_next);
  h->x0_ready = true;
  h->last_resync_path = FB_RESYNC_DELTA_MERGED;
  lap("node order and elements");
  FB_TRY(device_constraint_masks(s, n_new, n_fixed, fixed, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->fixed_stage, h->dofmask, h->nodemask));
  h->masks_ready = true;
  // ---- the plan, from the plan (delta.hip) ----
  OldPlanArrays old_plan = {h->d_bptr.p, h->d_bcol.p, h->d_ucnt.p, h->slice_off.p, h->slot_coff.p, h->contrib.p, n_old, h->plan.n_blocks};
  h->plan = unsharded_plan(n_new, nt_new, n_fixed);
  DevicePlan Dp;
  // (built next to the arrays it is built from; colidx, the list heights and the 16-bit column words are read by no stage of it)
  Dp.slice_off = &D.slice_off2; Dp.colidx = &h->colidx; Dp.slot_coff = &D.slot_coff2; Dp.slot_ccnt = &h->slot_ccnt; Dp.contrib = &D.contrib2;
  Dp.bptr = &D.bptr2; Dp.bcol = &D.bcol2; Dp.blk_slot = &D.blk_slot2; Dp.coldelta = &h->coldelta; Dp.ucnt_keep = &D.ucnt2;
  h->csr_ready = false;
  FB_TRY(delta_plan(s, D, old_plan, h->tets_next.p, h->tets.p, n_new, Dp, W));  // (tets_next: the old list, swapped out above)
  h->slice_off.swap(D.slice_off2); h->slot_coff.swap(D.slot_coff2); h->contrib.swap(D.contrib2);
  h->d_bptr.swap(D.bptr2); h->d_bcol.swap(D.bcol2); h->d_blk_slot.swap(D.blk_slot2); h->d_ucnt.swap(D.ucnt2);
  h->csr_ready = true;
  adopt_device_plan(h, Dp, 1);
  h->device_plan = true;
  h->host_pattern = false;
  lap("plan");
  if (has_material_map(h)) h->mat_ids.swap(h->mat_ids_next);
  FB_TRY(upload_plan(h, nullptr));
  lap("per-step arrays");
  FB_TRY(rest_state_checked(h));
  lap("rest state");
  return FB_OK;
}

// ... and every live embedding carried across it, in the same call: MeshDelta and CutWork are scratch the next change overwrites.
// (device_src with elements added: fb_fem_cut stands behind the change, as for the element map above)
int resync_delta(fb_fem_s* h, int n_removed, const int* removed, int n_changed, const int* changed_ids, const int* changed_nodes, int n_added, const int* added,
                 int n_new_nodes, const double* new_xyz, int n_fixed, const int* fixed, bool device_src = false, bool force_rebuild = false) {
  FB_TRY(resync_delta_apply(h, n_removed, removed, n_changed, changed_ids, changed_nodes, n_added, added, n_new_nodes, new_xyz, n_fixed, fixed, device_src, force_rebuild));
  if (!h->embed.n_live) return FB_OK;
  const CutWork* cut = device_src && n_added ? &h->cut : nullptr;
  EmbedMesh M;
  M.n_nodes = h->plan.n_global; M.n_tets = h->plan.n_tets; M.tets = h->tets.p; M.x0 = h->x0.p;
  M.caller_of = h->ren.active ? h->ren.d_old_of_new.p : nullptr;
  M.internal_of = h->ren.active ? h->ren.d_new_of_old.p : nullptr;
  for (Embedding& E : h->embed.slot)
    if (E.live) FB_TRY(embed_follow(h->stream, h->embed, E, M, h->delta, cut, cut && cut->mode == FB_CUT_BAKE));
  return FB_OK;
}

// fb_fem_params.expect_cuts: everything a fb_fem_resync_delta allocates -- the second set of plan arrays it builds into, the element and
// node maps, the sort's temporaries for a change of a twentieth of the elements -- is allocated at creation by running the empty change
int prewarm_delta(fb_fem_s* h, int n_fixed, const int* fixed) {
  MeshDelta& D = h->delta;
  FB_TRY(delta_reserve(h->stream, D, h->plan_ws, (long long)16 * (h->plan.n_tets / 20 + 64)));
  if (h->ren.active) {
    // ... and the node order's second stage on this mesh, into a scratch order: a cut mesh needs it (renumber.h) where the uncut one did
    // not, and the first launch of its kernels in a process costs milliseconds (7 of the 9.7 ms of a first cut, tools/probe_resync_delta.py)
    Renumbering scratch;
    FB_TRY(renumber_build(h->stream, FB_RENUMBER_ON, h->plan.n_global, h->plan.n_tets, h->tets.p, h->x0.p, h->plan_ws, scratch, true));
  }
  FB_TRY(resync_delta(h, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, n_fixed, fixed));
  h->last_resync_path = FB_RESYNC_FULL;
  return FB_OK;
}

// A delta re-sync that only takes elements out (n_removed ascending ids in a DEVICE list; none: the empty change) with q, qvel, (qaccel)
// and the external forces carried across it: a re-sync leaves the vectors zero, and the rebuilt path gives a renumbered handle a new
// order, so they go out in the caller's order before it and come back in the order it left.  force_rebuild: the full builder whatever
// there is to merge into.  The list is copied on the handle's stream by the re-sync's first step.  A failure inside the re-sync leaves
// the handle poisoned like any failed re-sync.
int resync_delta_carrying(fb_fem_s* h, int n_removed, const int* d_removed, bool force_rebuild) {
  hipStream_t s = h->stream;
  const int n = h->plan.n_global;
  const size_t len = (size_t)3 * n;
  DevBuf<double>* vec[4] = {&h->q, &h->qvel, &h->fext, &h->qacc};
  const int n_vec = h->prm.integrator == FB_INTEGRATOR_NEWMARK ? 4 : 3;
  FB_TRY(h->carry.reserve(len * n_vec));
  for (int v = 0; v < n_vec; v++) {
    double* dst = h->carry.p + len * v;
    if (h->ren.active) FB_TRY(gather_nodes(s, n, 3, vec[v]->p, h->ren.d_new_of_old.p, dst));
    else FB_HIP(hipMemcpyAsync(dst, vec[v]->p, sizeof(double) * len, hipMemcpyDeviceToDevice, s));
  }
  const std::vector<int> fixed = h->fixed_caller;
  FB_HIP(hipStreamSynchronize(s));
  ResyncScope scope(h);
  FB_TRY(resync_delta(h, n_removed, d_removed, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, (int)fixed.size(), fixed.data(), n_removed > 0, force_rebuild));
  for (int v = 0; v < n_vec; v++) {
    const double* src = h->carry.p + len * v;
    // (the builder may have decided against an order for the new mesh: FB_RENUMBER_AUTO)
    if (h->ren.active) FB_TRY(gather_nodes(s, n, 3, src, h->ren.d_old_of_new.p, vec[v]->p));
    else FB_HIP(hipMemcpyAsync(vec[v]->p, src, sizeof(double) * len, hipMemcpyDeviceToDevice, s));
  }
  FB_HIP(hipStreamSynchronize(s));
  scope.commit();
  return FB_OK;
}

}  // namespace

extern "C++" {
namespace fb {  // for parts.hip
// The rest positions of a renumbered handle have moved (fb_fem_split_parts): its node order was derived from the old ones, and so were the
// keys later cuts merge their new nodes by.  The handle is built again from its own mesh on the device -- the full builder of
// fb_fem_resync_delta with an empty change, which derives the order a new handle of the moved mesh would get -- and q, qvel, (qaccel) and
// the external forces are carried across in the caller's order, as FB_CUT_CARRY carries the state.  The labels of the parts hold the
// caller's ids and the element order, which do not change: they stay valid (PartsWork's arrays in the internal order are the build's own
// scratch, see parts.h).  Called for a handle with an active renumbering only -- which an unsharded handle has from build_plan_on_device
// alone, so its plan is device-built.  fb_fem_resync_path reports the rebuild (FB_RESYNC_DELTA_REBUILT).  A failure inside the rebuild
// leaves the handle poisoned like any failed re-sync.
int refresh_node_order(fb_fem_s* h) {
  if (!h->ren.active || !h->device_plan) return fail(FB_EINVAL, "refresh_node_order: the handle has no internal node order");
  const bool labels = h->parts.valid;
  FB_TRY(resync_delta_carrying(h, 0, nullptr, true));
  h->parts.valid = labels;
  return FB_OK;
}

// for detach.hip: the piece of fb_fem_detach_part.  dm's arrays belong to another handle of the same device; the new handle's own stream
// copies them, so whoever wrote them has been waited for, and creation ends with a wait for the new stream (the rest-state check).
int create_from_device_mesh(fb_fem_t* out, const DeviceTetMesh& dm, int n_fixed, const int* fixed, const fb_fem_params* params) {
  return create_common(out, dm.n_vertices, nullptr, dm.n_tets, nullptr, n_fixed, fixed, params, 1, 0, nullptr, nullptr, &dm);
}

// ... and the removal of its elements from the parent: fb_fem_resync_delta's device-fed removal (the order of the rest is kept, no node
// goes: the nodes only the removed elements used get identity rows).  A re-sync leaves the vectors zero, so q, qvel, (qaccel) and the
// external forces are carried across in the caller's order, as refresh_node_order carries them -- the change may take either path of the
// delta re-sync, and the rebuilt one gives a renumbered handle a new order.
int remove_elements_device(fb_fem_s* h, int n_removed, const int* d_removed) { return resync_delta_carrying(h, n_removed, d_removed, false); }
}  // namespace fb
}  // extern "C++"

int fb_fem_resync_delta(fb_fem_t h, int n_removed, const int* removed, int n_changed, const int* changed_ids, const int* changed_nodes, int n_added,
                        const int* added_tets, int n_new_nodes, const double* new_xyz, int n_fixed_dofs, const int* fixed_dofs) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  FB_HIP(hipSetDevice(h->prm.device));
  if (h->poisoned) return fail(FB_EINVAL, "the handle is unusable after a failed re-sync: a full fb_fem_resync first");
  if (h->plan.n_ranks > 1 || !h->device_plan) return fail(FB_EINVAL, "fb_fem_resync_delta is for unsharded handles whose plan was built on the device");
  if (n_removed < 0 || n_changed < 0 || n_added < 0 || n_new_nodes < 0 || n_fixed_dofs < 0) return fail(FB_EINVAL, "negative count");
  if ((n_removed && !removed) || (n_changed && (!changed_ids || !changed_nodes)) || (n_added && !added_tets) || (n_new_nodes && !new_xyz) || (n_fixed_dofs && !fixed_dofs))
    return fail(FB_EINVAL, "null array with a non-zero count");
  const int nt_old = h->plan.n_tets;
  const long long n_new = (long long)h->plan.n_global + n_new_nodes, nt_new = (long long)nt_old - n_removed + n_added;
  if (n_new >= (1LL << 31) - 2 || nt_new >= (1LL << 28)) return fail(FB_EINVAL, "mesh too large");
  if (nt_new < 1) return fail(FB_EINVAL, "the change leaves no element");
  for (int k = 0; k < n_removed; k++)
    if (removed[k] < 0 || removed[k] >= nt_old || (k && removed[k] <= removed[k - 1])) return fail(FB_EINVAL, "removed[%d] = %d: ids must ascend inside [0,%d)", k, removed[k], nt_old);
  for (int k = 0, r = 0; k < n_changed; k++) {
    if (changed_ids[k] < 0 || changed_ids[k] >= nt_old || (k && changed_ids[k] <= changed_ids[k - 1]))
      return fail(FB_EINVAL, "changed_ids[%d] = %d: ids must ascend inside [0,%d)", k, changed_ids[k], nt_old);
    while (r < n_removed && removed[r] < changed_ids[k]) r++;
    if (r < n_removed && removed[r] == changed_ids[k]) return fail(FB_EINVAL, "element %d is both removed and changed", changed_ids[k]);
  }
  for (long long k = 0; k < 4LL * n_changed; k++)
    if (changed_nodes[k] < 0 || changed_nodes[k] >= n_new) return fail(FB_EINVAL, "changed element %d references node %d outside [0,%lld)", changed_ids[k / 4], changed_nodes[k], n_new);
  for (long long k = 0; k < 4LL * n_added; k++)
    if (added_tets[k] < 0 || added_tets[k] >= n_new) return fail(FB_EINVAL, "added element %lld references node %d outside [0,%lld)", k / 4, added_tets[k], n_new);
  FB_TRY(check_fixed_dofs(n_fixed_dofs, fixed_dofs, 3 * n_new));
  FB_HIP(hipStreamSynchronize(h->stream));
  ResyncScope scope(h);
  FB_TRY(resync_delta(h, n_removed, removed, n_changed, changed_ids, changed_nodes, n_added, added_tets, n_new_nodes, new_xyz, n_fixed_dofs, fixed_dofs));
  scope.commit();
  return FB_OK;
}

// the constrained DOFs of a live handle: the same mesh, new masks
int fb_fem_set_constrained_dofs(fb_fem_t h, int n_fixed_dofs, const int* fixed_dofs) {
  CHECK_HANDLE(h);
  if (n_fixed_dofs < 0 || (n_fixed_dofs > 0 && !fixed_dofs)) return fail(FB_EINVAL, "bad constrained DOF list");
  if (h->device_plan && h->plan.n_ranks == 1) {
    FB_TRY(device_constraint_masks(h->stream, h->plan.n_global, n_fixed_dofs, fixed_dofs, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->fixed_stage, h->dofmask, h->nodemask));
    h->plan.n_fixed_owned = n_fixed_dofs;
    h->fixed_caller.assign(fixed_dofs, fixed_dofs + n_fixed_dofs);
  } else if (!h->l2c.empty()) {  // a renumbered shard: the list in internal ids, ascending again
    FB_TRY(check_fixed_dofs(n_fixed_dofs, fixed_dofs, 3LL * h->plan.n_global));
    FB_TRY(plan_set_constraints(h->plan, n_fixed_dofs, fixed_to_internal(h, n_fixed_dofs, fixed_dofs).data()));
    FB_TRY(upload_masks(h));
  } else {
    FB_TRY(plan_set_constraints(h->plan, n_fixed_dofs, fixed_dofs));
    FB_TRY(upload_masks(h));
    if (h->plan.n_ranks == 1) h->fixed_caller.assign(fixed_dofs, fixed_dofs + n_fixed_dofs);  // (fb_fem_read_constrained_dofs)
  }
  h->system_valid = false;
  return motion_constraints_changed(h);  // (moved DOFs that are no longer constrained leave the set; q and qvel stay)
}

int fb_fem_resync_path(fb_fem_t h) { return h ? h->last_resync_path : FB_RESYNC_FULL; }

// ---- fb_fem_cut (subdivide.h) ----
int fb_fem_cut(fb_fem_t h, int n_strip_points, const double* strip_xyz, int mode, int modify, fb_cut_result* out) {
  CHECK_HANDLE(h);
  if (out) memset(out, 0, sizeof(*out));
  if (h->plan.n_ranks > 1 || !h->device_plan) return fail(FB_EINVAL, "fb_fem_cut is for unsharded handles whose plan was built on the device");
  if (mode != FB_CUT_BAKE && mode != FB_CUT_CARRY) return fail(FB_EINVAL, "cut mode %d: FB_CUT_BAKE or FB_CUT_CARRY", mode);
  std::vector<double> quads;
  FB_TRY(cut_quads(n_strip_points, strip_xyz, quads));
  hipStream_t s = h->stream;
  CutWork& C = h->cut;
  C.valid = false;
  C.mode = mode;
  C.n_quads = (int)(quads.size() / 12);
  C.n_cut = C.n_a = C.n_b = C.n_unhandled = C.n_edges = C.n_added = 0;
  C.min_ratio = 0.0;
  C.min_volume = 0.0;
  C.unhandled_ids.clear();
  C.unhandled_codes.clear();
  bool delta = false;
  int status = FB_CUT_NOTHING;
  const int n_old = h->plan.n_global, nt_old = h->plan.n_tets;
  const int* caller_of = h->ren.active ? h->ren.d_old_of_new.p : nullptr;
  const int* internal_of = h->ren.active ? h->ren.d_new_of_old.p : nullptr;
  if (C.n_quads) {
    FB_TRY(C.quads.alloc(quads.size()));
    FB_HIP(hipMemcpyAsync(C.quads.p, quads.data(), sizeof(double) * quads.size(), hipMemcpyHostToDevice, s));
    FB_TRY(cut_classify(s, C, nt_old, h->tets.p, caller_of, h->x0.p, h->q.p, h->plan_ws));
    if (C.n_unhandled) {
      status = FB_CUT_UNHANDLED;
      FB_TRY(cut_read_unhandled(s, C, h->plan_ws));
    } else if (C.n_cut) {
      FB_TRY(cut_emit(s, C, n_old, h->tets.p, caller_of, internal_of, h->x0.p, h->q.p, h->plan_ws));
      delta = true;
      status = modify ? FB_CUT_DONE : FB_CUT_DRY;
      if ((long long)n_old + 2LL * C.n_edges >= (1LL << 31) - 2 || (long long)nt_old - C.n_cut + C.n_added >= (1LL << 28)) return fail(FB_EINVAL, "mesh too large after the cut");
      // a split point on a node (t = 0 or |edge|) would leave a flat piece, which the rest state refuses after the point of no return
      if (modify && !(C.min_ratio > 0.0)) return fail(FB_EINVAL, "the cut would leave a piece without volume (smallest piece / parent volume %g)", C.min_ratio);
      // ... and so would a piece the records cannot hold: every handle keeps the rest volumes as floats (volf, and the element records of fp32
      // storage, which FB_MATRIX_AUTO may choose at any later re-sync).  Below FLT_MIN a float loses bits and from 1.4e-45 down it is zero: the
      // piece then weighs and resists nothing, and a node that lies in such pieces only gets an empty row.  k_tet_rest itself is fp64 and would
      // accept the piece (its determinant is not zero), so this is checked here, before anything changes.
      if (modify && !((float)C.min_volume >= FLT_MIN))
        return fail(FB_EINVAL, "the cut would leave a piece of volume %g, which the fp32 element records cannot hold (below %g; smallest piece / parent volume %g)",
                    C.min_volume, (double)FLT_MIN, C.min_ratio);
    }
  }
  C.valid = true;
  C.n_nodes = n_old;
  if (out) {
    out->status = status;
    out->n_quads = C.n_quads;
    out->n_case_a = C.n_a; out->n_case_b = C.n_b; out->n_unhandled = C.n_unhandled;
    if (delta) {
      out->n_cut_edges = C.n_edges;
      out->n_removed = C.n_cut; out->n_added = C.n_added; out->n_new_nodes = 2 * C.n_edges;
      out->min_volume_ratio = C.min_ratio;
    }
  }
  if (status != FB_CUT_DONE) return FB_OK;
  // ---- the point of no return ----
  const int n_new = n_old + 2 * C.n_edges;
  const bool newmark = h->prm.integrator == FB_INTEGRATOR_NEWMARK;
  const int n_vec = newmark ? 3 : 2;
  const size_t len = (size_t)3 * n_new;
  ResyncScope scope(h);
  if (mode == FB_CUT_CARRY) {  // the state in the caller's order, new nodes interpolated
    FB_TRY(h->carry.reserve(len * n_vec));
    const DevBuf<double>* src[3] = {&h->q, &h->qvel, &h->qacc};
    for (int v = 0; v < n_vec; v++) {
      double* dst = h->carry.p + len * v;
      if (h->ren.active) FB_TRY(gather_nodes(s, n_old, 3, src[v]->p, h->ren.d_new_of_old.p, dst));
      else FB_HIP(hipMemcpyAsync(dst, src[v]->p, sizeof(double) * 3 * (size_t)n_old, hipMemcpyDeviceToDevice, s));
      FB_TRY(cut_interpolate(s, C, n_old, dst));
    }
  } else {
    if (motion_active(h)) FB_TRY(motion_rest_absorbs_q(h));  // (the targets are displacements from the rest shape that is about to move)
    FB_TRY(cut_bake(s, 3LL * n_old, h->x0.p, h->q.p));  // the deformed shape is the new rest shape (Deformable.cpp:144-147)
  }
  const std::vector<int> fixed = h->fixed_caller;
  FB_TRY(resync_delta(h, C.n_cut, C.cut_tets.p, 0, nullptr, nullptr, C.n_added, reinterpret_cast<const int*>(C.added.p), 2 * C.n_edges, C.new_xyz.p, (int)fixed.size(),
                      fixed.data(), true));
  if (mode == FB_CUT_CARRY) {
    DevBuf<double>* dst[3] = {&h->q, &h->qvel, &h->qacc};
    for (int v = 0; v < n_vec; v++) {
      const double* src = h->carry.p + len * v;
      if (h->ren.active) FB_TRY(gather_nodes(s, n_new, 3, src, h->ren.d_old_of_new.p, dst[v]->p));
      else FB_HIP(hipMemcpyAsync(dst[v]->p, src, sizeof(double) * len, hipMemcpyDeviceToDevice, s));
    }
  }
  FB_HIP(hipStreamSynchronize(s));
  scope.commit();
  return FB_OK;
}

int fb_fem_read_cut(fb_fem_t h, int* removed, int* added_tets, double* new_xyz, int* edge_nodes, double* edge_frac, int* unhandled_ids, int* unhandled_codes) {
  CHECK_HANDLE(h);
  const CutWork& C = h->cut;
  if (!C.valid) return fail(FB_EINVAL, "no fb_fem_cut has run on this handle");
  hipStream_t s = h->stream;
  const bool delta = C.n_cut > 0 && C.n_unhandled == 0;
  if (delta) {
    if (removed) FB_TRY(C.cut_tets.download(removed, (size_t)C.n_cut, s));
    if (added_tets) FB_TRY(C.added.download(reinterpret_cast<int4*>(added_tets), (size_t)C.n_added, s));
    if (new_xyz) FB_TRY(C.new_xyz.download(new_xyz, (size_t)6 * C.n_edges, s));
    if (edge_nodes || edge_frac) {
      std::vector<unsigned long long> keys((size_t)C.n_edges);
      std::vector<double> frac((size_t)C.n_edges);
      FB_TRY(C.ukeys.download(keys.data(), keys.size(), s));
      FB_TRY(C.frac.download(frac.data(), frac.size(), s));
      for (int k = 0; k < C.n_edges; k++)
        for (int c = 0; c < 2; c++) {
          if (edge_nodes) { edge_nodes[4 * k + 2 * c] = (int)(keys[k] >> 32); edge_nodes[4 * k + 2 * c + 1] = (int)(keys[k] & 0xffffffffu); }
          if (edge_frac) edge_frac[2 * k + c] = frac[k];
        }
    }
  }
  for (size_t k = 0; k < C.unhandled_ids.size(); k++) {
    if (unhandled_ids) unhandled_ids[k] = C.unhandled_ids[k];
    if (unhandled_codes) unhandled_codes[k] = C.unhandled_codes[k];
  }
  return FB_OK;
}

int fb_fem_read_mesh(fb_fem_t h, double* rest_xyz, int* tets) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_read_mesh is for unsharded handles");
  hipStream_t s = h->stream;
  const int n = h->plan.n_global, nt = h->plan.n_tets;
  if (rest_xyz) FB_TRY(download_owned(h, h->x0, rest_xyz));
  if (tets) {
    if (h->ren.active) {
      FB_TRY(h->tets_caller.alloc((size_t)nt));
      FB_HIP(hipMemcpyAsync(h->tets_caller.p, h->tets.p, sizeof(int4) * (size_t)nt, hipMemcpyDeviceToDevice, s));
      FB_TRY(relabel_tets(s, nt, h->tets_caller.p, n, h->ren.d_old_of_new.p));
      FB_TRY(h->tets_caller.download(reinterpret_cast<int4*>(tets), (size_t)nt, s));
    } else {
      FB_TRY(h->tets.download(reinterpret_cast<int4*>(tets), (size_t)nt, s));
    }
  }
  return FB_OK;
}

}  // extern "C"
