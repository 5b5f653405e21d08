// Penalty contact of a handle with itself (self_contact.h), hand-written for gfx950.
//
// The rule is the header's (include/fembrain_hip.h, "Contact of a body with itself"): every surface vertex that lies inside an element
// it may meet is pushed to the closest point of the boundary it may meet, and the face there is pushed back.  What a point may not meet
// is its exclusion: under FB_SELF_CONTACT_ANY the elements and faces that have the point's node among their own, under
// FB_SELF_CONTACT_OTHER_PARTS those of the point's part.  A point's key is its internal node or its part, an element answers with its
// four nodes or element_part, a face with its three nodes or the part of its element (face_part, filled once per call).
//  - positions: a thread per node, x0 + q and the box (k_contact_positions of face_search.hip.h); a position that is not finite opens
//    the box to infinity and the call ends there;
//  - containment, the other way round than body_contact.hip: the body's box is its own, so every surface vertex is a candidate and every
//    element would be binned.  The surface vertices -- two orders of magnitude fewer -- are binned instead, one sort over the cells of a
//    grid over the box, positions and keys stored in sorted order; a thread per element walks the cells its padded current box overlaps
//    (the cell functions of embed_grid.hip.h) and, for each point there that its box holds, that it may meet and whose four weights
//    (embed's bary) are >= 0, takes the point's slot with an integer atomicMin of its own id.  The lowest element wins whatever the
//    order: no floating-point atomic, the same bits from call to call.  An element over more than kEmbedWideCells cells goes to an
//    overflow list that wavefronts walk afterwards, lanes striding over the sorted points.  One compaction of the taken slots, one host
//    wait for their number;
//  - closest face: k_face_scan / k_face_ring of face_search.hip.h under a FaceExclusion, the excluded faces skipped ("The searches are
//    written over an exclusion" there); a contact for which the searches find no face has none left and is dropped;
//  - forces: contact_force.hip.h with four records per contact -- here a node can be pushed as a point and push back as a corner in one
//    call, so all four contributions of a contact are records (node, 4 contact + r), r = 0 the point's +F, r = 1..3 the corners' (-F) b_k;
//    sorted stably by node, and the thread at the head of a node's segment adds the whole segment, however long, in record order onto
//    the value the vector had.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "contact_force.hip.h"
#include "device_prims.hip.h"
#include "embed_grid.hip.h"
#include "face_search.hip.h"
#include "fem_handle.h"
#include "launch.hip.h"
#include "mesh_device.hip.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

// ---- the exclusion ----

// of an element: t its nodes, part its part
__device__ __forceinline__ bool element_excluded(int mode, int key, const int4& t, int part) {
  return mode == FB_SELF_CONTACT_OTHER_PARTS ? part == key : (t.x == key || t.y == key || t.z == key || t.w == key);
}

// ---- the grid of surface vertices and containment ----

// A thread per surface vertex: its cell, its key, its empty slot.  A vertex without a node sorts behind every cell.
__global__ __launch_bounds__(kB) void k_sc_point_keys(int nv, const int* __restrict__ vnode, const int* __restrict__ vertex_ids, int n_nodes, const double* __restrict__ cur, GridDev g,
                                                      int mode, const int* __restrict__ node_part_out, int* __restrict__ p_key, uint32_t* __restrict__ cells,
                                                      uint32_t* __restrict__ vals, int* __restrict__ slot) {
  const int v = blockIdx.x * kB + threadIdx.x;
  if (v >= nv) return;
  const int nd = vnode[v];
  uint32_t cell = (uint32_t)(g.dim[0] * g.dim[1] * g.dim[2]);
  int key = -1;
  if ((unsigned)nd < (unsigned)n_nodes) {
    const double* p = cur + 3 * (size_t)nd;
    cell = (uint32_t)((cell_clamped(g, 2, p[2]) * g.dim[1] + cell_clamped(g, 1, p[1])) * g.dim[0] + cell_clamped(g, 0, p[0]));
    if (mode == FB_SELF_CONTACT_OTHER_PARTS) {
      const int c = vertex_ids[v];
      key = (unsigned)c < (unsigned)n_nodes ? node_part_out[c] : -1;
    } else {
      key = nd;
    }
  }
  cells[v] = cell;
  vals[v] = (uint32_t)v;
  p_key[v] = key;
  slot[v] = INT_MAX;
}

// A thread per sorted entry: the point's coordinates, a plane each, and its key (a vertex without a node: no position, nothing holds it)
__global__ __launch_bounds__(kB) void k_sc_point_store(int nv, const uint32_t* __restrict__ p_v_s, const int* __restrict__ vnode, int n_nodes, const double* __restrict__ cur,
                                                       const int* __restrict__ p_key, double* __restrict__ xyz, int* __restrict__ key_s) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= nv) return;
  const uint32_t v = p_v_s[j];
  const int nd = v < (uint32_t)nv ? vnode[v] : -1;
  const bool ok = (unsigned)nd < (unsigned)n_nodes;
#pragma unroll
  for (int k = 0; k < 3; k++) xyz[(size_t)k * nv + j] = ok ? cur[3 * (size_t)nd + k] : NAN;
  key_s[j] = ok ? p_key[v] : -1;
}

// what the containment kernels know of the sorted points
struct PointsDev {
  int nv, mode;
  const int *cell_lo, *cell_hi;
  const double* xyz;
  const int* key_s;
  const uint32_t* v_s;
  int* slot;
};

// the sorted point j against element e (vertices v, padded box [a, b], nodes t, part)
__device__ __forceinline__ void test_point(const PointsDev& P, int j, int e, const int4& t, int part, const double (*v)[3], const double* a, const double* b) {
  const double p[3] = {P.xyz[j], P.xyz[(size_t)P.nv + j], P.xyz[2 * (size_t)P.nv + j]};
  if (!in_box(p, a, b)) return;  // (also a position that is not a number)
  if (element_excluded(P.mode, P.key_s[j], t, part)) return;
  double w[4];
  if (!bary(v, p, w)) return;
  const uint32_t vr = P.v_s[j];
  if (vr < (uint32_t)P.nv) atomicMin(P.slot + vr, e);
}

__device__ __forceinline__ void padded_box(const double (*v)[3], double pad, double* a, double* b) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    a[k] = fmin(fmin(v[0][k], v[1][k]), fmin(v[2][k], v[3][k])) - pad;
    b[k] = fmax(fmax(v[0][k], v[1][k]), fmax(v[2][k], v[3][k])) + pad;
  }
}

// A thread per element: the points of the cells its padded box overlaps; an element over more than kEmbedWideCells cells is flagged
__global__ __launch_bounds__(kB) void k_sc_contain(int n_tets, const int4* __restrict__ tets, const double* __restrict__ cur, const int* __restrict__ element_part, GridDev g, PointsDev P,
                                                   unsigned char* __restrict__ wide_flag) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  double v[4][3], a[3], b[3];
  load_tet(tets, cur, e, v);
  padded_box(v, g.pad, a, b);
  int c0[3], c1[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c0[k] = cell_clamped(g, k, a[k]);
    c1[k] = cell_clamped(g, k, b[k]);
    if (c1[k] < c0[k]) c1[k] = c0[k];
  }
  const long long n = (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  const bool wide = n > kEmbedWideCells;
  wide_flag[e] = wide ? 1 : 0;
  if (wide) return;
  const int4 t = tets[e];
  const int part = P.mode == FB_SELF_CONTACT_OTHER_PARTS ? element_part[e] : 0;
  for (int z = c0[2]; z <= c1[2]; z++)
    for (int y = c0[1]; y <= c1[1]; y++)
      for (int x = c0[0]; x <= c1[0]; x++) {
        const int c = (z * g.dim[1] + y) * g.dim[0] + x;
        const int j1 = min(P.cell_hi[c], P.nv);
        for (int j = max(P.cell_lo[c], 0); j < j1; j++) test_point(P, j, e, t, part, v, a, b);
      }
}

// Wavefronts over the overflow list (its length on the device: nobody waits for it), lanes striding over every sorted point
__global__ __launch_bounds__(kB) void k_sc_contain_wide(const int* __restrict__ n_wide, const int* __restrict__ wide, int n_tets, const int4* __restrict__ tets,
                                                        const double* __restrict__ cur, const int* __restrict__ element_part, double pad, PointsDev P) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = min(max(*n_wide, 0), n_tets), n_waves = gridDim.x * kWaves;
  for (int i = blockIdx.x * kWaves + wave; i < n; i += n_waves) {
    const int e = wide[i];
    if ((unsigned)e >= (unsigned)n_tets) continue;
    double v[4][3], a[3], b[3];
    load_tet(tets, cur, e, v);
    padded_box(v, pad, a, b);
    const int4 t = tets[e];
    const int part = P.mode == FB_SELF_CONTACT_OTHER_PARTS ? element_part[e] : 0;
    for (int j = lane; j < P.nv; j += 64) test_point(P, j, e, t, part, v, a, b);
  }
}

// A thread per surface vertex: its slot was taken
__global__ __launch_bounds__(kB) void k_sc_taken(int nv, const int* __restrict__ slot, unsigned char* __restrict__ flag) {
  const int v = blockIdx.x * kB + threadIdx.x;
  if (v < nv) flag[v] = slot[v] != INT_MAX ? 1 : 0;
}

__global__ __launch_bounds__(kB) void k_sc_iota(int n, int* __restrict__ out) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i < n) out[i] = i;
}

// A thread per boundary face: the part of its element
__global__ __launch_bounds__(kB) void k_sc_face_part(int nf, const int* __restrict__ face_tets, int n_tets, const int* __restrict__ element_part, int* __restrict__ face_part) {
  const int f = blockIdx.x * kB + threadIdx.x;
  if (f >= nf) return;
  const int e = face_tets[f];
  face_part[f] = (unsigned)e < (unsigned)n_tets ? element_part[e] : -1;
}

// ---- host ----

int check_self(fb_fem_s* h, const fb_fem_self_contact_params* p) {
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_self_contact is for unsharded handles");
  if (!p) return fail(FB_EINVAL, "null self contact parameters");
  FB_TRY(check_penalty("self contact", p->stiffness, p->depth_cap));
  if (p->mode != FB_SELF_CONTACT_ANY && p->mode != FB_SELF_CONTACT_OTHER_PARTS) return fail(FB_EINVAL, "self contact mode %d", p->mode);
  if (h->plan.n_global <= 0 || h->plan.n_global >= (1 << 28)) return fail(FB_EINVAL, "fb_fem_self_contact: %d nodes", h->plan.n_global);
  return FB_OK;
}

constexpr int kWideWorkgroups = 64;  // of k_sc_contain_wide: 256 wavefronts share the overflow list

// add: into the external force vector, the result kept for fb_fem_read_self_contact; else into scratch, nothing kept (seconds: the stages).
// fr: null for the frictionless call; else the friction call's parameters, fout its info.
int self_contact(fb_fem_s* h, const fb_fem_self_contact_params& prm, bool add, double* seconds, fb_fem_self_contact_info* out,
                 const fb_fem_contact_friction_params* fr = nullptr, fb_fem_contact_friction_info* fout = nullptr) {
  SelfContactWork& W = h->selfc;
  PlanWorkspace& ws = h->plan_ws;
  hipStream_t s = h->stream;
  const bool by_part = prm.mode == FB_SELF_CONTACT_OTHER_PARTS;
  fb_fem_self_contact_info I;
  memset(&I, 0, sizeof(I));
  // the surface and, where the mode asks for them, the labels belong to the current mesh
  FB_TRY(surface_current(h));
  if (by_part) {
    const int before = h->parts.n_builds;
    FB_TRY(parts_current(h));
    I.n_parts_builds = h->parts.n_builds - before;
  }
  FB_TRY(stage_events(W.fs));
  const SurfaceWork& SF = h->surf;
  const int n_nodes = h->plan.n_global, n_tets = h->plan.n_tets, nv = SF.n_vertices, nf = SF.n_faces;
  I.n_points = nv;
  Stages tm;
  tm.ev = W.fs.ev_t; tm.s = s; tm.seconds = seconds;

  // ---- positions and box ----
  FB_TRY(tm.begin());
  const int nb = blocks_for(n_nodes);
  const size_t n_box = fr ? 7 : 6;  // (the friction call: behind the box the flag of a velocity that is not finite, read in the same wait)
  FB_TRY(W.cur.reserve((size_t)3 * n_nodes)); FB_TRY(W.box_part.reserve((size_t)6 * nb)); FB_TRY(W.boxes.reserve(n_box));
  FB_TRY(launch_1d(k_contact_positions, n_nodes, s, n_nodes, h->x0.p, h->q.p, W.cur.p, W.box_part.p));
  FB_TRY(launch_grid(k_box_final<double>, dim3(1), s, nb, W.box_part.p, W.boxes.p));
  if (fr) {
    FB_HIP(hipMemsetAsync(W.boxes.p + 6, 0, sizeof(double), s));
    FB_TRY(launch_1d(k_cf_finite, 3LL * n_nodes, s, 3LL * n_nodes, h->qvel.p, W.boxes.p + 6));
  }
  double box[7];
  box[6] = 0.0;
  FB_TRY(W.boxes.download(box, n_box, s));  // a host wait
  FB_TRY(tm.end(0));
  for (int k = 0; k < 6; k++)
    if (!std::isfinite(box[k])) return fail(FB_EINVAL, "fb_fem_self_contact: a position of the body is not finite");
  if (box[6] != 0.0) return fail(FB_EINVAL, "fb_fem_self_contact_friction: a velocity of the body is not finite");
  const bool nothing = nv <= 0 || nf <= 0 || n_tets <= 0 || (by_part && h->parts.n_parts < 2);  // (one part has nothing to meet: no grid, no write)
  std::vector<BodyContactRec> recs;
  std::vector<ContactFrictionRec> side;
  int n_found = 0;
  double* fext = h->fext.p;
  if (!add) {
    FB_TRY(W.scratch.reserve((size_t)3 * n_nodes));
    FB_TRY(W.scratch.zero(s));
    fext = W.scratch.p;
  }
  double ext_max = 0.0;
  for (int k = 0; k < 3; k++) ext_max = std::max(ext_max, box[3 + k] - box[k]);
  if (!(ext_max > 0.0)) ext_max = 1.0;
  const double pad = std::ldexp(ext_max, -30);  // (embed_grid_build's padding: far above the rounding of a determinant test)

  if (!nothing) {
    // ---- the grid of surface vertices, containment ----
    FB_TRY(tm.begin());
    GridDev pg = make_grid(box, box + 3, pad, nv);
    const int n_cells = pg.dim[0] * pg.dim[1] * pg.dim[2];
    FB_TRY(W.p_key.reserve((size_t)nv)); FB_TRY(W.p_key_s.reserve((size_t)nv)); FB_TRY(W.slot.reserve((size_t)nv)); FB_TRY(W.hit.reserve((size_t)nv));
    FB_TRY(W.p_cell.reserve((size_t)nv)); FB_TRY(W.p_cell_s.reserve((size_t)nv)); FB_TRY(W.p_v.reserve((size_t)nv)); FB_TRY(W.p_v_s.reserve((size_t)nv));
    FB_TRY(W.p_xyz.reserve((size_t)3 * nv));
    FB_TRY(W.cell_lo.reserve((size_t)n_cells)); FB_TRY(W.cell_hi.reserve((size_t)n_cells));
    FB_TRY(W.flag.reserve((size_t)std::max(nv, n_tets))); FB_TRY(W.wide.reserve((size_t)n_tets)); FB_TRY(W.counts.reserve(2));
    if (W.ident_n < (size_t)nv) {  // (growth may move the buffer: filled from the start)
      FB_TRY(W.ident.reserve((size_t)nv));
      FB_TRY(launch_1d(k_sc_iota, nv, s, nv, W.ident.p));
      W.ident_n = (size_t)nv;
    }
    const int* part_of_element = by_part ? h->parts.element_part.p : nullptr;
    FB_TRY(launch_1d(k_sc_point_keys, nv, s, nv, SF.vnode.p, SF.vertex_ids.p, n_nodes, W.cur.p, pg, prm.mode, by_part ? h->parts.node_part_out.p : nullptr, W.p_key.p,
                     W.p_cell.p, W.p_v.p, W.slot.p));
    FB_TRY(sort_pairs(ws.temp, s, W.p_cell.p, W.p_cell_s.p, W.p_v.p, W.p_v_s.p, (size_t)nv, (unsigned)bits_of((long long)n_cells + 1)));
    FB_HIP(hipMemsetAsync(W.cell_lo.p, 0, sizeof(int) * (size_t)n_cells, s));
    FB_HIP(hipMemsetAsync(W.cell_hi.p, 0, sizeof(int) * (size_t)n_cells, s));
    FB_TRY(launch_1d(k_run_bounds<>, (long long)nv, s, nv, W.p_cell_s.p, (uint32_t)n_cells, W.cell_lo.p, W.cell_hi.p));
    FB_TRY(launch_1d(k_sc_point_store, nv, s, nv, W.p_v_s.p, SF.vnode.p, n_nodes, W.cur.p, W.p_key.p, W.p_xyz.p, W.p_key_s.p));
    I.n_point_grid_builds = 1;
    const PointsDev PD = {nv, prm.mode, W.cell_lo.p, W.cell_hi.p, W.p_xyz.p, W.p_key_s.p, W.p_v_s.p, W.slot.p};
    FB_TRY(launch_1d(k_sc_contain, n_tets, s, n_tets, h->tets.p, W.cur.p, part_of_element, pg, PD, W.flag.p));
    FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.wide.p, W.counts.p, (size_t)n_tets));
    FB_TRY(launch_grid(k_sc_contain_wide, dim3(kWideWorkgroups), s, W.counts.p, W.wide.p, n_tets, h->tets.p, W.cur.p, part_of_element, pad, PD));
    FB_TRY(launch_1d(k_sc_taken, nv, s, nv, W.slot.p, W.flag.p));
    FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.hit.p, W.counts.p + 1, (size_t)nv));
    FB_TRY(W.counts.download(&n_found, 1, s, 1));  // a host wait
    if (n_found < 0 || n_found > nv) return fail(FB_EDEVICE, "self contact: %d contacts of %d surface vertices", n_found, nv);
    FB_TRY(tm.end(1));
  }

  if (n_found > 0) {
    // ---- the path, and the face grid where it is the ring's ----
    GridDev fgrid = make_grid(box, box + 3, pad, nf);
    const bool ring = path_knob("FEMBRAIN_SELF_CONTACT") != FB_BODY_CONTACT_SCAN && grid_covered(fgrid);  // (default: the ring wherever its proof holds)
    I.path = ring ? FB_BODY_CONTACT_RING : FB_BODY_CONTACT_SCAN;
    FB_TRY(tm.begin());
    if (by_part) {
      FB_TRY(W.face_part.reserve((size_t)nf));
      FB_TRY(launch_1d(k_sc_face_part, nf, s, nf, SF.face_tets.p, n_tets, h->parts.element_part.p, W.face_part.p));
    }
    if (ring) {
      FB_TRY(build_face_grid(s, ws, W.fs, SF.faces_int.p, nf, n_nodes, W.cur.p, fgrid));
      I.n_face_grid_builds = 1;
    }
    FB_TRY(tm.end(2));

    // ---- the closest faces ----
    FB_TRY(tm.begin());
    SearchDev S;
    S.n_contacts = n_found; S.hit = W.hit.p; S.cand = W.ident.p; S.vnode = SF.vnode.p; S.vertex_ids = SF.vertex_ids.p; S.c_elem = W.slot.p;
    S.n_cand = nv; S.nv = nv; S.n_nodes_p = n_nodes; S.cur_p = W.cur.p;
    S.nf = nf; S.n_nodes_t = n_nodes; S.faces_int = SF.faces_int.p; S.cur_t = W.cur.p;
    const FaceExclusion ex = {prm.mode, nf, SF.faces_int.p, by_part ? W.face_part.p : nullptr, W.p_key.p};
    FB_TRY(search_faces(s, W.fs, S, ex, ring, fgrid, budget_knob("FEMBRAIN_SELF_CONTACT_BUDGET", nf)));
    FB_TRY(tm.end(3));

    // ---- forces ----
    FB_TRY(tm.begin());
    const FrictionLaw law = {fr ? fr->mu : 0.0, fr ? fr->slip_speed : 0.0, fr ? fr->damping : 0.0};
    FB_TRY(contact_forces<4>(s, ws, W.fs, S, prm.stiffness, prm.depth_cap, fr ? &law : nullptr, h->qvel.p, h->qvel.p, nullptr, fext, recs, &side));
    FB_TRY(tm.end(4));
  }

  // the sums, in record order; a contact without a face is dropped here (it made no record that counts)
  std::vector<BodyContactRec> kept;
  std::vector<ContactFrictionRec> kept_side;
  kept.reserve(recs.size());
  const ContactSums sums = contact_sums(recs, prm.depth_cap, ContactSums(), [&](size_t i, const BodyContactRec& r) {
    if (r.face < 0) return false;
    kept.push_back(r);
    if (fr) kept_side.push_back(side[i]);
    return true;
  });
  I.faces_tested = sums.faces_tested; I.n_degenerate = sums.n_degenerate; I.max_depth = sums.max_depth;
  for (int k = 0; k < 3; k++) { I.force_on_points[k] = sums.on_points[k]; I.force_on_faces[k] = sums.on_faces[k]; }
  I.n_contacts = (int)kept.size();
  if (fr) {
    fb_fem_contact_friction_info FI;
    memset(&FI, 0, sizeof(FI));
    friction_sums(kept, kept_side, *fr, 0, FI);
    if (fout) *fout = FI;
  }
  if (add) {
    W.host.swap(kept);
    W.info = I;
    if (fr) W.fric_host.swap(kept_side);
  }
  if (out) *out = I;
  return FB_OK;
}

}  // namespace
}  // namespace fb

// ---- the C ABI ----

int fb_fem_self_contact(fb_fem_t h, const fb_fem_self_contact_params* p, fb_fem_self_contact_info* out) {
  CHECK_HANDLE(h);
  FB_TRY(check_self(h, p));
  return self_contact(h, *p, true, nullptr, out);
}

int fb_fem_self_contact_friction(fb_fem_t h, const fb_fem_self_contact_params* p, const fb_fem_contact_friction_params* fr, fb_fem_self_contact_info* out,
                                 fb_fem_contact_friction_info* fout) {
  CHECK_HANDLE(h);
  FB_TRY(check_self(h, p));
  FB_TRY(check_friction(fr, "fb_fem_self_contact_friction"));
  return self_contact(h, *p, true, nullptr, out, fr, fout);
}

int fb_fem_read_self_contact_friction(fb_fem_t h, double* normal_force, double* slip3, double* friction3) {
  CHECK_HANDLE(h);
  read_friction(h->selfc.fric_host, normal_force, slip3, friction3);
  return FB_OK;
}

int fb_fem_read_self_contact(fb_fem_t h, int* node, int* element, int* face, double* closest_xyz, double* bary3, double* depth) {
  CHECK_HANDLE(h);
  read_contacts(h->selfc.host, node, element, face, closest_xyz, bary3, depth);
  return FB_OK;
}

int fb_fem_time_self_contact(fb_fem_t h, const fb_fem_self_contact_params* p, int reps, double seconds[5]) {
  CHECK_HANDLE(h);
  FB_TRY(check_self(h, p));
  if (reps < 1 || !seconds) return fail(FB_EINVAL, "fb_fem_time_self_contact: reps must be positive and seconds not null");
  FB_TRY(self_contact(h, *p, false, nullptr, nullptr));  // warm: the buffers exist, the labels are current
  double sum[5] = {0, 0, 0, 0, 0};
  for (int r = 0; r < reps; r++) FB_TRY(self_contact(h, *p, false, sum, nullptr));
  for (int k = 0; k < 5; k++) seconds[k] = sum[k] / reps;
  return FB_OK;
}
