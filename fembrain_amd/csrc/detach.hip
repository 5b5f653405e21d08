// A part of the cut mesh detached into a handle of its own (detach.h), hand-written for gfx950.
//
// The piece is the mesh parts_extract leaves on the device (PartsWork::out_nodes / out_xyz / out_tets), handed to the device plan builder
// as resync_delta_rebuild hands it its own mesh; what it inherits is gathered between the two handles' node orders by the kernels below.
//
// Streams.  The piece has a stream of its own; the parent's extraction buffers, state vectors, DOF mask and element map are written on
// the PARENT's stream, and the next fb_fem_read_part overwrites the extraction buffers.  The ordering chosen is the plain one, two waits
// of the host:
//   1. everything that reads the parent alone -- the extraction, the DOF flags and their compaction, the downloads of the caller's
//      arrays -- runs on the parent's stream and ends with hipStreamSynchronize(parent stream) (the downloads wait; an explicit wait
//      follows them, because fb_fem_set_uniform_force and a step's last kernels are not waited for by every entry point);
//   2. only then does the piece's stream start: the builder's copies of out_tets / out_xyz, the state gather (parent vectors and maps ->
//      piece vectors), the byte gather (parent map -> piece map).  Nothing runs on the parent's stream meanwhile: the call owns the handle;
//   3. hipStreamSynchronize(piece stream) before the removal starts and before the call returns: every read of the parent's buffers is
//      complete when the parent's stream writes them again (the removal, a later fb_fem_read_part, a step).
// No event is needed: an event wait would only pay where the two streams could overlap, and the builder waits for the host anyway
// (the plan's counts, the rest-state check).
//
// The map chain of the state gather: piece internal id i -> the part's local id (the piece's old_of_new; i where the piece keeps the
// caller's order) -> the parent's caller id (out_nodes) -> the parent's internal id (the parent's new_of_old; the caller id where the
// parent keeps the caller's order).  The constrained DOFs take the last two links: local DOF 3 l + a is constrained exactly when the
// parent's DOF mask (internal order, 0 = constrained) says so for the node behind out_nodes[l]; the flags are compacted by one select
// over a counting iterator, which leaves them ascending in local ids, the order fb_fem_create asks for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "device_prims.hip.h"
#include "fem_handle.h"
#include "launch.hip.h"
#include "detach.h"

namespace fb {
namespace {

struct StateVecs { const double* src[4]; double* dst[4]; };

// A thread per node of the piece (its internal order): the node's three values of every carried vector from the parent's node behind it
__global__ __launch_bounds__(kB) void k_detach_gather_state(int n_nodes, const int* __restrict__ piece_local_of, const int* __restrict__ part_nodes,
                                                            const int* __restrict__ parent_internal_of, int n_vec, StateVecs V) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_nodes) return;
  const int l = piece_local_of ? piece_local_of[i] : i;
  const int c = part_nodes[l];
  const size_t from = 3 * (size_t)(parent_internal_of ? parent_internal_of[c] : c), to = 3 * (size_t)i;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    if (v >= n_vec) break;
    const double* __restrict__ s = V.src[v];
    double* __restrict__ d = V.dst[v];
#pragma unroll
    for (int a = 0; a < 3; a++) d[to + a] = s[from + a];
  }
}

// A thread per element of the part (rank j in ascending order): its byte of the parent's per-element array
__global__ __launch_bounds__(kB) void k_detach_gather_bytes(int n_el, const uint32_t* __restrict__ ids, const unsigned char* __restrict__ bytes, unsigned char* __restrict__ out) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j < n_el) out[j] = bytes[ids[j]];
}

// A thread per node of the part (local id l): a flag per DOF, set where the parent constrains it (dofmask: 0 = constrained)
__global__ __launch_bounds__(kB) void k_detach_flag_dofs(int n_nd, const int* __restrict__ part_nodes, const int* __restrict__ parent_internal_of,
                                                         const unsigned char* __restrict__ dofmask, unsigned char* __restrict__ flag) {
  const int l = blockIdx.x * kB + threadIdx.x;
  if (l >= n_nd) return;
  const int c = part_nodes[l];
  const size_t from = 3 * (size_t)(parent_internal_of ? parent_internal_of[c] : c);
#pragma unroll
  for (int a = 0; a < 3; a++) flag[3 * (size_t)l + a] = dofmask[from + a] ? 0 : 1;
}

}  // namespace

int detach_gather_state(hipStream_t s, const DetachMaps& M, int n_vec, const double* const src[4], double* const dst[4]) {
  StateVecs V;
  for (int v = 0; v < 4; v++) { V.src[v] = v < n_vec ? src[v] : nullptr; V.dst[v] = v < n_vec ? dst[v] : nullptr; }
  return launch_1d(k_detach_gather_state, M.n_nodes, s, M.n_nodes, M.piece_local_of, M.part_nodes, M.parent_internal_of, n_vec, V);
}

int detach_gather_bytes(hipStream_t s, int n_el, const uint32_t* element_ids, const unsigned char* bytes, unsigned char* out) {
  return launch_1d(k_detach_gather_bytes, n_el, s, n_el, element_ids, bytes, out);
}

int detach_fixed_dofs(hipStream_t s, DetachWork& D, int n_nd, const int* part_nodes, const int* parent_internal_of, const unsigned char* dofmask, PlanWorkspace& W,
                      std::vector<int>* out) {
  const size_t nd3 = (size_t)3 * n_nd;
  FB_TRY(D.dof_flag.reserve(nd3)); FB_TRY(D.dof_list.reserve(nd3)); FB_TRY(D.count.alloc(1));
  FB_TRY(launch_1d(k_detach_flag_dofs, n_nd, s, n_nd, part_nodes, parent_internal_of, dofmask, D.dof_flag.p));
  FB_TRY(select_flagged(W.temp, s, rocprim::counting_iterator<int>(0), D.dof_flag.p, D.dof_list.p, D.count.p, nd3));
  int nf = 0;
  FB_TRY(D.count.download(&nf, 1, s));
  if (nf < 0 || (size_t)nf > nd3) return fail(FB_EDEVICE, "detach: %d constrained DOFs of %zu", nf, nd3);
  out->resize((size_t)nf);
  return D.dof_list.download(out->data(), (size_t)nf, s);
}

}  // namespace fb

// ---- the C ABI ----

namespace {

// what the piece takes over once it exists; everything here runs on the PIECE's stream (step 2 of the ordering above)
int piece_inherit(fb_fem_s* h, fb_fem_s* p, int n_el, int first) {
  hipStream_t ps = p->stream;
  const bool newmark = h->prm.integrator == FB_INTEGRATOR_NEWMARK;
  p->nm_beta = h->nm_beta; p->nm_gamma = h->nm_gamma; p->nm_eps = h->nm_eps; p->nm_max_newton = h->nm_max_newton;
  DetachMaps M;
  M.n_nodes = p->plan.n_global;
  M.piece_local_of = p->ren.active ? p->ren.d_old_of_new.p : nullptr;
  M.part_nodes = h->parts.out_nodes.p;
  M.parent_internal_of = h->ren.active ? h->ren.d_new_of_old.p : nullptr;
  const double* src[4] = {h->q.p, h->qvel.p, h->fext.p, h->qacc.p};
  double* dst[4] = {p->q.p, p->qvel.p, p->fext.p, p->qacc.p};
  FB_TRY(detach_gather_state(ps, M, newmark ? 4 : 3, src, dst));
  if (has_material_map(h)) {
    SlackScope slack(handle_slack_now(p));  // the handle's slack rule, as for the element buffers
    DevBuf<unsigned char> ids;
    FB_TRY(ids.alloc((size_t)std::max(1, n_el)));
    FB_TRY(detach_gather_bytes(ps, n_el, h->parts.sorted.p + first, h->mat_ids.p, ids.p));
    FB_TRY(inherit_materials(p, h, &ids));
  } else {
    FB_TRY(inherit_materials(p, h, nullptr));
  }
  FB_HIP(hipStreamSynchronize(ps));  // step 3: every read of the parent's buffers is complete
  return FB_OK;
}

}  // namespace

extern "C" {

int fb_fem_detach_part(fb_fem_t h, int part, int flags, fb_fem_t* out, int* element_ids, int* node_ids, fb_fem_detach_info* info) {
  if (out) *out = nullptr;
  CHECK_HANDLE(h);
  if (!out) return fail(FB_EINVAL, "fb_fem_detach_part: null out");
  if (flags != FB_DETACH_KEEP && flags != FB_DETACH_REMOVE) return fail(FB_EINVAL, "fb_fem_detach_part: flags %d: FB_DETACH_KEEP or FB_DETACH_REMOVE", flags);
  if (h->plan.n_ranks > 1 || !h->device_plan) return fail(FB_EINVAL, "fb_fem_detach_part is for unsharded handles whose plan was built on the device");
  FB_TRY(fb_fem_parts(h, nullptr));  // (labels first when stale, as every call on the parts does)
  PartsWork& P = h->parts;
  if (part < 0 || part >= P.n_parts) return fail(FB_EINVAL, "fb_fem_detach_part: part %d outside [0, %d)", part, P.n_parts);
  const bool remove = flags == FB_DETACH_REMOVE;
  if (remove && P.n_parts < 2) return fail(FB_EINVAL, "fb_fem_detach_part: the handle has one part, and a handle cannot be left without elements");
  hipStream_t s = h->stream;
  // ---- step 1, on the parent's stream: the part as a mesh, its constrained DOFs, the caller's arrays ----
  int ne = 0, nd = 0, first = 0;
  std::vector<int> fixed;
  {
    SlackScope slack(handle_slack_now(h));
    FB_TRY(parts_extract(s, P, parts_mesh(h), part, &ne, &nd, &first, h->plan_ws));
    FB_TRY(detach_fixed_dofs(s, h->detach, nd, P.out_nodes.p, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->dofmask.p, h->plan_ws, &fixed));
  }
  if (element_ids) FB_TRY(P.sorted.download(reinterpret_cast<uint32_t*>(element_ids), (size_t)ne, s, (size_t)first));
  if (node_ids) FB_TRY(P.out_nodes.download(node_ids, (size_t)nd, s));
  FB_HIP(hipStreamSynchronize(s));
  // ---- step 2, on the piece's stream: the handle and what it inherits ----
  DeviceTetMesh dm;
  dm.device = h->prm.device; dm.n_vertices = nd; dm.n_tets = ne; dm.xyz = nullptr;
  dm.tets = reinterpret_cast<const uint4*>(P.out_tets.p); dm.xyz64 = P.out_xyz.p;
  const fb_fem_params prm = h->prm;  // (as the setters have left them: timestep, damping, CG; entry 0 of the material table)
  fb_fem_t piece = nullptr;
  FB_TRY(create_from_device_mesh(&piece, dm, (int)fixed.size(), fixed.data(), &prm));
  int rc = piece_inherit(h, piece, ne, first);
  // ---- the removal, on the parent's stream again ----
  // (the labels go stale with it, but the list of the part's elements stays where it is until the next labelling)
  if (rc == FB_OK && remove) rc = remove_elements_device(h, ne, reinterpret_cast<const int*>(P.sorted.p + first));
  if (rc != FB_OK) {
    const std::string keep = last_error();
    fb_fem_destroy(piece);
    last_error() = keep;
    return rc;
  }
  if (info) {
    info->part = part; info->n_elements = ne; info->n_nodes = nd;
    info->n_fixed_dofs = (int)fixed.size();
    info->n_materials = (int)piece->mat_E.size();
    info->parent_elements_left = h->plan.n_tets;
    info->parent_resync_path = remove ? h->last_resync_path : -1;
  }
  *out = piece;
  return FB_OK;
}

int fb_fem_num_constrained_dofs(fb_fem_t h) { return h && h->plan.n_ranks == 1 ? (int)h->fixed_caller.size() : -1; }

int fb_fem_read_constrained_dofs(fb_fem_t h, int* dofs) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_read_constrained_dofs is for unsharded handles");
  if (dofs && !h->fixed_caller.empty()) memcpy(dofs, h->fixed_caller.data(), sizeof(int) * h->fixed_caller.size());
  return FB_OK;
}

}  // extern "C"
