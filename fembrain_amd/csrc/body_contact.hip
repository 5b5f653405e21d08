// Penalty contact between two handles on one device (body_contact.h), hand-written for gfx950.
//
// The rule is the header's (include/fembrain_hip.h, "Contact between two bodies"): the surface vertices of one body (P) that lie inside an
// element of the other (T) are pushed to the closest point of T's boundary, and the face that holds it is pushed back.  Per direction:
//  - candidates: a thread per surface vertex of P, the closed box of T's nodes, one compaction;
//  - containment: the elements of T whose current box meets the overlap of the two bodies' boxes -- a resting contact touches a thin layer,
//    and a large body does not pay a whole-mesh grid per step -- are binned into a grid over that overlap with the cell functions of
//    embed_grid.hip.h (an element over more than kEmbedWideCells cells goes to an overflow list, as in embed.hip); a thread per candidate
//    walks its cell, elements ascending, with embed's weight function: the first that contains it is the lowest;
//  - closest face: k_face_scan / k_face_ring of face_search.hip.h, nothing excluded (the argument why the ring misses no face is there);
//  - forces: contact_force.hip.h with three records per contact -- a thread per contact forms F and adds it to its own node of P (the
//    contacts of a direction are different nodes); the three corners of the face in T become records (node, 3 contact + corner), sorted
//    stably by node, and a thread per node's segment adds them in record order -- ascending contact, corners 0 1 2 -- onto the value
//    the vector had.  No floating-point atomics.
// Node ids cross from the caller's numbering to the handles' internal orders here: the surface's vnode / faces_int index the internal
// arrays, its vertex_ids / face order are what the caller reads.
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

struct Box3 {
  double lo[3], hi[3];
};

// ---- boxes ----

// A thread per surface vertex: the workgroup's box of their current positions
__global__ __launch_bounds__(kB) void k_bc_surface_box(int nv, const int* __restrict__ vnode, int n_nodes, const double* __restrict__ cur, double* __restrict__ part) {
  const int v = blockIdx.x * kB + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (v < nv) {
    const int nd = vnode[v];
    if ((unsigned)nd < (unsigned)n_nodes)
#pragma unroll
      for (int k = 0; k < 3; k++) lo[k] = hi[k] = cur[3 * (size_t)nd + k];
  }
  wg_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

// ---- candidates and containment ----

// A thread per surface vertex of P: inside the closed box of T's nodes
__global__ __launch_bounds__(kB) void k_bc_candidates(int nv, const int* __restrict__ vnode, int n_nodes, const double* __restrict__ cur, Box3 T, unsigned char* __restrict__ flag) {
  const int v = blockIdx.x * kB + threadIdx.x;
  if (v >= nv) return;
  const int nd = vnode[v];
  bool in = false;
  if ((unsigned)nd < (unsigned)n_nodes) {
    const double p[3] = {cur[3 * (size_t)nd], cur[3 * (size_t)nd + 1], cur[3 * (size_t)nd + 2]};
    in = in_box(p, T.lo, T.hi);
  }
  flag[v] = in ? 1 : 0;
}

// the box of element e at the current positions, padded
__device__ __forceinline__ void tet_box(const int4* __restrict__ tets, const double* __restrict__ cur, int e, double pad, double* a, double* b) {
  double v[4][3];
  load_tet(tets, cur, e, v);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    a[k] = fmin(fmin(v[0][k], v[1][k]), fmin(v[2][k], v[3][k])) - pad;
    b[k] = fmax(fmax(v[0][k], v[1][k]), fmax(v[2][k], v[3][k])) + pad;
  }
}

// A thread per element of T: its padded box meets the overlap box O
__global__ __launch_bounds__(kB) void k_bc_tet_flag(int n_tets, const int4* __restrict__ tets, const double* __restrict__ cur, Box3 O, double pad, unsigned char* __restrict__ flag) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  double a[3], b[3];
  tet_box(tets, cur, e, pad, a, b);
  bool meets = true;
#pragma unroll
  for (int k = 0; k < 3; k++) meets = meets && a[k] <= O.hi[k] && b[k] >= O.lo[k];
  flag[e] = meets ? 1 : 0;
}

// the cells of the grid over O that the padded box of element e overlaps (clamped into the grid: the element may reach beyond O)
__device__ __forceinline__ void tet_cells_clamped(const GridDev& g, const int4* __restrict__ tets, const double* __restrict__ cur, int e, int* c0, int* c1) {
  double a[3], b[3];
  tet_box(tets, cur, e, g.pad, a, b);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c0[k] = cell_clamped(g, k, a[k]);
    c1[k] = cell_clamped(g, k, b[k]);
    if (c1[k] < c0[k]) c1[k] = c0[k];
  }
}

// A thread per binned element: the cells it overlaps, 0 for one of the overflow list (one entry past the end: the scan leaves the total there)
__global__ __launch_bounds__(kB) void k_bc_tet_count(int m, int n_tets, const int* __restrict__ sel, GridDev g, const int4* __restrict__ tets, const double* __restrict__ cur,
                                                     int* __restrict__ cnt, unsigned char* __restrict__ wide_flag) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j > m) return;
  if (j == m) { cnt[j] = 0; return; }
  const int e = sel[j];
  if ((unsigned)e >= (unsigned)n_tets) { cnt[j] = 0; wide_flag[j] = 0; return; }
  int c0[3], c1[3];
  tet_cells_clamped(g, tets, cur, e, c0, c1);
  const long long n = (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  const bool wide = n > kEmbedWideCells;
  cnt[j] = wide ? 0 : (int)n;
  wide_flag[j] = wide ? 1 : 0;
}

__global__ __launch_bounds__(kB) void k_bc_tet_emit(int m, int n_tets, const int* __restrict__ sel, GridDev g, const int4* __restrict__ tets, const double* __restrict__ cur,
                                                    const int* __restrict__ cnt, const int* __restrict__ off, long long n_pairs, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= m || cnt[j] == 0) return;
  const int e = sel[j];
  if ((unsigned)e >= (unsigned)n_tets) return;
  int c0[3], c1[3];
  tet_cells_clamped(g, tets, cur, e, c0, c1);
  long long o = off[j];
  const long long end = o + cnt[j];
  for (int z = c0[2]; z <= c1[2]; z++)
    for (int y = c0[1]; y <= c1[1]; y++)
      for (int x = c0[0]; x <= c1[0]; x++) {
        if (o < 0 || o >= end || o >= n_pairs) return;
        keys[o] = (uint32_t)((z * g.dim[1] + y) * g.dim[0] + x);
        vals[o] = (uint32_t)e;
        o++;
      }
}

// A thread per candidate: the lowest element of T that contains it, or -1.  g.wide / g.n_wide: the overflow list, ascending.
__global__ __launch_bounds__(kB) void k_bc_contain(int n_cand, const int* __restrict__ cand, int nv, const int* __restrict__ vnode, int n_nodes_p, const double* __restrict__ cur_p,
                                                   GridDev g, long long n_pairs, int n_tets, const int4* __restrict__ tets, const double* __restrict__ cur_t, int* __restrict__ c_elem,
                                                   unsigned char* __restrict__ flag) {
  const int t = blockIdx.x * kB + threadIdx.x;
  if (t >= n_cand) return;
  int best = INT_MAX;
  const int vr = cand[t];
  const int nd = (unsigned)vr < (unsigned)nv ? vnode[vr] : -1;
  if ((unsigned)nd < (unsigned)n_nodes_p) {
    const double p[3] = {cur_p[3 * (size_t)nd], cur_p[3 * (size_t)nd + 1], cur_p[3 * (size_t)nd + 2]};
    if (in_box(p, g.lo, g.hi)) {
      const int c = (cell_of(g, 2, p[2]) * g.dim[1] + cell_of(g, 1, p[1])) * g.dim[0] + cell_of(g, 0, p[0]);
      const int j0 = max(g.cell_lo[c], 0), j1 = (int)min((long long)g.cell_hi[c], n_pairs);
      for (int j = j0; j < j1; j++) {
        const int e = g.cell_elem[j];
        if ((unsigned)e >= (unsigned)n_tets) continue;
        double v[4][3], w[4];
        load_tet(tets, cur_t, e, v);
        if (bary(v, p, w)) { best = e; break; }
      }
    }
    for (int j = 0; j < g.n_wide; j++) {
      const int e = g.wide[j];
      if (e >= best) break;  // (the list ascends)
      if ((unsigned)e >= (unsigned)n_tets) continue;
      double v[4][3], w[4];
      load_tet(tets, cur_t, e, v);
      if (bary(v, p, w)) { best = e; break; }
    }
  }
  c_elem[t] = best == INT_MAX ? -1 : best;
  flag[t] = best == INT_MAX ? 0 : 1;
}

// ---- host ----

// one body as a direction sees it
struct Body {
  fb_fem_s* h;
  int n_nodes, n_tets;
  const double* cur;
  double node_box[6], surf_box[6];
  double* fext;
};

int ensure_events(BodyContactWork& W) {
  if (!W.ev_in) FB_HIP(hipEventCreateWithFlags(&W.ev_in, hipEventDisableTiming));
  if (!W.ev_out) FB_HIP(hipEventCreateWithFlags(&W.ev_out, hipEventDisableTiming));
  return stage_events(W.fs);
}

// current positions of a body and the boxes of its nodes and of its surface vertices, into boxes[12 which ..]
int body_boxes(hipStream_t s, BodyContactWork& W, fb_fem_s* h, int which) {
  const int n = h->plan.n_global, nv = h->surf.n_vertices;
  const int nb = blocks_for(n), nbv = blocks_for(nv);
  FB_TRY(W.cur[which].reserve((size_t)3 * n));
  FB_TRY(W.box_part.reserve((size_t)6 * std::max(nb, nbv)));
  FB_TRY(launch_1d(k_contact_positions, n, s, n, h->x0.p, h->q.p, W.cur[which].p, W.box_part.p));
  FB_TRY(launch_grid(k_box_final<double>, dim3(1), s, nb, W.box_part.p, W.boxes.p + 12 * which));
  FB_TRY(launch_1d(k_bc_surface_box, nv, s, nv, h->surf.vnode.p, n, W.cur[which].p, W.box_part.p));
  FB_TRY(launch_grid(k_box_final<double>, dim3(1), s, nbv, W.box_part.p, W.boxes.p + 12 * which + 6));
  return FB_OK;
}

struct DirResult {
  int n_candidates = 0, n_contacts = 0, path = FB_BODY_CONTACT_NONE, tet_grids = 0, face_grids = 0;
};

// One direction: the surface vertices of P against T.  s: the calling handle's stream; fext_p / fext_t: where the forces are added.
// law: null for the frictionless rule; else the friction call's, its side records into side_out.
int run_direction(hipStream_t s, BodyContactWork& W, PlanWorkspace& ws, const Body& P, const Body& T, const fb_fem_body_contact_params& prm, double* fext_p, double* fext_t,
                  Stages& tm, std::vector<BodyContactRec>& out, DirResult& res, const FrictionLaw* law = nullptr, std::vector<ContactFrictionRec>* side_out = nullptr) {
  out.clear();
  if (side_out) side_out->clear();
  const SurfaceWork& SP = P.h->surf;
  const SurfaceWork& ST = T.h->surf;
  const int nv = SP.n_vertices, nf = ST.n_faces;
  // the overlap of P's surface box and T's node box; where they do not meet the direction ends
  Box3 O, TB;
  bool meet = nv > 0 && nf > 0 && T.n_tets > 0;
  for (int k = 0; k < 3; k++) {
    O.lo[k] = std::max(P.surf_box[k], T.node_box[k]); O.hi[k] = std::min(P.surf_box[3 + k], T.node_box[3 + k]);
    TB.lo[k] = T.node_box[k]; TB.hi[k] = T.node_box[3 + k];
    if (!(O.lo[k] <= O.hi[k])) meet = false;
  }
  if (!meet) return FB_OK;
  double ext_max = 0.0;
  for (int k = 0; k < 3; k++) ext_max = std::max(ext_max, TB.hi[k] - TB.lo[k]);
  if (!(ext_max > 0.0)) ext_max = 1.0;
  const double pad = std::ldexp(ext_max, -30);  // (embed_grid_build's padding: far above the rounding of a determinant test)

  // ---- candidates, element grid, containment ----
  FB_TRY(tm.begin());
  FB_TRY(W.counts.reserve(4));
  FB_TRY(W.flag.reserve((size_t)std::max(std::max(nv, T.n_tets), 1)));
  FB_TRY(W.cand.reserve((size_t)nv));
  FB_TRY(launch_1d(k_bc_candidates, nv, s, nv, SP.vnode.p, P.n_nodes, P.cur, TB, W.flag.p));
  FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.cand.p, W.counts.p, (size_t)nv));
  int n_cand = 0;
  FB_TRY(W.counts.download(&n_cand, 1, s));  // a host wait
  if (n_cand < 0 || n_cand > nv) return fail(FB_EDEVICE, "body contact: %d candidates of %d surface vertices", n_cand, nv);
  res.n_candidates = n_cand;
  int n_contacts = 0;
  GridDev tg;
  memset(&tg, 0, sizeof(tg));
  if (n_cand > 0) {
    FB_TRY(W.sel.reserve((size_t)T.n_tets));
    FB_TRY(launch_1d(k_bc_tet_flag, T.n_tets, s, T.n_tets, T.h->tets.p, T.cur, O, pad, W.flag.p));
    FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.sel.p, W.counts.p + 1, (size_t)T.n_tets));
    int m = 0;
    FB_TRY(W.counts.download(&m, 1, s, 1));  // a host wait
    if (m < 0 || m > T.n_tets) return fail(FB_EDEVICE, "body contact: %d of %d elements binned", m, T.n_tets);
    if (m > 0) {
      tg = make_grid(O.lo, O.hi, pad, m);
      const int n_cells = tg.dim[0] * tg.dim[1] * tg.dim[2];
      FB_TRY(W.t_cnt.reserve((size_t)m + 1)); FB_TRY(W.t_off.reserve((size_t)m + 1));
      FB_TRY(W.cell_lo.reserve((size_t)n_cells)); FB_TRY(W.cell_hi.reserve((size_t)n_cells));
      FB_TRY(ws.vals_s.reserve((size_t)m));  // (the overflow list: the plan builder's array, as the sort's below)
      int* wide = reinterpret_cast<int*>(ws.vals_s.p);
      FB_TRY(launch_1d(k_bc_tet_count, m + 1, s, m, T.n_tets, W.sel.p, tg, T.h->tets.p, T.cur, W.t_cnt.p, W.flag.p));
      FB_TRY(exclusive_scan(ws.temp, s, W.t_cnt.p, W.t_off.p, 0, (size_t)m + 1));
      FB_TRY(select_flagged(ws.temp, s, W.sel.p, W.flag.p, wide, W.counts.p + 2, (size_t)m));
      int total = 0, n_wide = 0;
      FB_HIP(hipMemcpyAsync(&total, W.t_off.p + m, sizeof(int), hipMemcpyDeviceToHost, s));
      FB_HIP(hipMemcpyAsync(&n_wide, W.counts.p + 2, sizeof(int), hipMemcpyDeviceToHost, s));
      FB_HIP(hipStreamSynchronize(s));  // a host wait
      if (total < 0 || (long long)total > (long long)kEmbedWideCells * m || n_wide < 0 || n_wide > m)
        return fail(FB_EDEVICE, "body contact grid: %d pairs, %d wide elements out of range", total, n_wide);
      FB_HIP(hipMemsetAsync(W.cell_lo.p, 0, sizeof(int) * (size_t)n_cells, s));
      FB_HIP(hipMemsetAsync(W.cell_hi.p, 0, sizeof(int) * (size_t)n_cells, s));
      FB_TRY(W.cell_elem.reserve((size_t)std::max(total, 1)));
      if (total) {
        FB_TRY(ws.keys.reserve(((size_t)total + 1) / 2)); FB_TRY(ws.keys_s.reserve(((size_t)total + 1) / 2)); FB_TRY(ws.vals.reserve((size_t)total));
        uint32_t* ck = reinterpret_cast<uint32_t*>(ws.keys.p);
        uint32_t* ck_s = reinterpret_cast<uint32_t*>(ws.keys_s.p);
        FB_TRY(launch_1d(k_bc_tet_emit, m, s, m, T.n_tets, W.sel.p, tg, T.h->tets.p, T.cur, W.t_cnt.p, W.t_off.p, (long long)total, ck, ws.vals.p));
        FB_TRY(sort_pairs(ws.temp, s, ck, ck_s, ws.vals.p, reinterpret_cast<uint32_t*>(W.cell_elem.p), (size_t)total, (unsigned)bits_of(n_cells)));
        FB_TRY(launch_1d(k_run_bounds<>, (long long)total, s, total, ck_s, (uint32_t)n_cells, W.cell_lo.p, W.cell_hi.p));
      }
      tg.n_wide = n_wide;
      tg.cell_lo = W.cell_lo.p; tg.cell_hi = W.cell_hi.p; tg.cell_elem = W.cell_elem.p; tg.wide = wide;
      res.tet_grids = 1;
      FB_TRY(W.c_elem.reserve((size_t)n_cand)); FB_TRY(W.hit.reserve((size_t)n_cand));
      FB_TRY(launch_1d(k_bc_contain, n_cand, s, n_cand, W.cand.p, nv, SP.vnode.p, P.n_nodes, P.cur, tg, (long long)total, T.n_tets, T.h->tets.p, T.cur, W.c_elem.p, W.flag.p));
      FB_TRY(select_flagged(ws.temp, s, rocprim::counting_iterator<int>(0), W.flag.p, W.hit.p, W.counts.p + 3, (size_t)n_cand));
      FB_TRY(W.counts.download(&n_contacts, 1, s, 3));  // a host wait
      if (n_contacts < 0 || n_contacts > n_cand) return fail(FB_EDEVICE, "body contact: %d contacts of %d candidates", n_contacts, n_cand);
    }
  }
  FB_TRY(tm.end(1));
  res.n_contacts = n_contacts;
  if (n_contacts == 0) return FB_OK;

  // ---- the path, and the face grid where it is the ring's ----
  GridDev fgrid = make_grid(TB.lo, TB.hi, pad, nf);
  const bool ring = path_knob("FEMBRAIN_BODY_CONTACT") != FB_BODY_CONTACT_SCAN && grid_covered(fgrid);  // (default: the ring wherever its proof holds; DESIGN.md 3k has the table)
  res.path = ring ? FB_BODY_CONTACT_RING : FB_BODY_CONTACT_SCAN;
  FB_TRY(tm.begin());
  if (ring) {
    FB_TRY(build_face_grid(s, ws, W.fs, ST.faces_int.p, nf, T.n_nodes, T.cur, fgrid));
    res.face_grids = 1;
  }
  FB_TRY(tm.end(2));

  // ---- the closest faces ----
  FB_TRY(tm.begin());
  SearchDev S;
  S.n_contacts = n_contacts; S.hit = W.hit.p; S.cand = W.cand.p; S.vnode = SP.vnode.p; S.vertex_ids = SP.vertex_ids.p; S.c_elem = W.c_elem.p;
  S.n_cand = n_cand; S.nv = nv; S.n_nodes_p = P.n_nodes; S.cur_p = P.cur;
  S.nf = nf; S.n_nodes_t = T.n_nodes; S.faces_int = ST.faces_int.p; S.cur_t = T.cur;
  FB_TRY(search_faces(s, W.fs, S, NoExclusion(), ring, fgrid, budget_knob("FEMBRAIN_BODY_CONTACT_BUDGET", nf)));
  FB_TRY(tm.end(3));

  // ---- forces ----
  FB_TRY(tm.begin());
  FB_TRY(contact_forces<3>(s, ws, W.fs, S, prm.stiffness, prm.depth_cap, law, P.h->qvel.p, T.h->qvel.p, fext_p, fext_t, out, side_out));
  FB_TRY(tm.end(4));
  return FB_OK;
}

int check_pair(fb_fem_s* a, fb_fem_s* b, const fb_fem_body_contact_params* p) {
  if (a == b) return fail(FB_EINVAL, "fb_fem_body_contact: the two handles are the same (self-contact is not built)");
  if (a->plan.n_ranks > 1 || b->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_body_contact is for unsharded handles");
  if (a->prm.device != b->prm.device) return fail(FB_EINVAL, "fb_fem_body_contact: the handles are on devices %d and %d", a->prm.device, b->prm.device);
  if (!p) return fail(FB_EINVAL, "null body contact parameters");
  FB_TRY(check_penalty("body contact", p->stiffness, p->depth_cap));
  if ((p->directions & (FB_BODY_A_INTO_B | FB_BODY_B_INTO_A)) == 0 || (p->directions & ~(FB_BODY_A_INTO_B | FB_BODY_B_INTO_A)) != 0)
    return fail(FB_EINVAL, "body contact directions %d", p->directions);
  if (a->plan.n_global <= 0 || b->plan.n_global <= 0 || a->plan.n_global >= (1 << 28) || b->plan.n_global >= (1 << 28))
    return fail(FB_EINVAL, "fb_fem_body_contact: %d and %d nodes", a->plan.n_global, b->plan.n_global);
  return FB_OK;
}

// add: into the two external force vectors, the result kept for fb_fem_read_body_contact; else into scratch, nothing kept (seconds: the stages).
// fr: null for the frictionless call; else the friction call's parameters, fout its info.
int body_contact(fb_fem_s* a, fb_fem_s* b, const fb_fem_body_contact_params& prm, bool add, double* seconds, fb_fem_body_contact_info* out,
                 const fb_fem_contact_friction_params* fr = nullptr, fb_fem_contact_friction_info* fout = nullptr) {
  BodyContactWork& W = a->bodyc;
  hipStream_t s = a->stream;
  // both surfaces belong to the current meshes (each is built on its own handle's stream, with its host waits)
  FB_TRY(surface_current(a));
  FB_TRY(surface_current(b));
  FB_TRY(ensure_events(W));
  // after what b has queued
  FB_HIP(hipEventRecord(W.ev_in, b->stream));
  FB_HIP(hipStreamWaitEvent(s, W.ev_in, 0));
  Stages tm;
  tm.ev = W.fs.ev_t; tm.s = s; tm.seconds = seconds;
  FB_TRY(tm.begin());
  const size_t n_boxes = fr ? 25 : 24;  // (the friction call: behind the boxes the flag of a velocity that is not finite, read in the same wait)
  FB_TRY(W.boxes.reserve(n_boxes));
  FB_TRY(body_boxes(s, W, a, 0));
  FB_TRY(body_boxes(s, W, b, 1));
  if (fr) {
    FB_HIP(hipMemsetAsync(W.boxes.p + 24, 0, sizeof(double), s));
    FB_TRY(launch_1d(k_cf_finite, 3LL * a->plan.n_global, s, 3LL * a->plan.n_global, a->qvel.p, W.boxes.p + 24));
    FB_TRY(launch_1d(k_cf_finite, 3LL * b->plan.n_global, s, 3LL * b->plan.n_global, b->qvel.p, W.boxes.p + 24));
  }
  double boxes[25];
  boxes[24] = 0.0;
  FB_TRY(W.boxes.download(boxes, n_boxes, s));  // a host wait
  FB_TRY(tm.end(0));
  Body A = {a, a->plan.n_global, a->plan.n_tets, W.cur[0].p, {}, {}, a->fext.p}, B = {b, b->plan.n_global, b->plan.n_tets, W.cur[1].p, {}, {}, b->fext.p};
  memcpy(A.node_box, boxes, sizeof(double) * 6); memcpy(A.surf_box, boxes + 6, sizeof(double) * 6);
  memcpy(B.node_box, boxes + 12, sizeof(double) * 6); memcpy(B.surf_box, boxes + 18, sizeof(double) * 6);
  for (int k = 0; k < 6; k++)
    if (!std::isfinite(A.node_box[k]) || !std::isfinite(B.node_box[k])) return fail(FB_EINVAL, "fb_fem_body_contact: a position of a body is not finite");
  if (boxes[24] != 0.0) return fail(FB_EINVAL, "fb_fem_body_contact_friction: a velocity of a body is not finite");
  if (!add) {
    FB_TRY(W.scratch[0].reserve((size_t)3 * A.n_nodes)); FB_TRY(W.scratch[1].reserve((size_t)3 * B.n_nodes));
    FB_TRY(W.scratch[0].zero(s)); FB_TRY(W.scratch[1].zero(s));
    A.fext = W.scratch[0].p; B.fext = W.scratch[1].p;
  }
  fb_fem_body_contact_info I;
  memset(&I, 0, sizeof(I));
  std::vector<BodyContactRec> recs[2];
  std::vector<ContactFrictionRec> side[2];
  fb_fem_contact_friction_info FI;
  memset(&FI, 0, sizeof(FI));
  const FrictionLaw law = {fr ? fr->mu : 0.0, fr ? fr->slip_speed : 0.0, fr ? fr->damping : 0.0};
  int rc = FB_OK;
  for (int dir = 0; dir < 2 && rc == FB_OK; dir++) {
    if (!(prm.directions & (dir == 0 ? FB_BODY_A_INTO_B : FB_BODY_B_INTO_A))) continue;
    const Body& P = dir == 0 ? A : B;
    const Body& T = dir == 0 ? B : A;
    DirResult R;
    rc = run_direction(s, W, a->plan_ws, P, T, prm, P.fext, T.fext, tm, recs[dir], R, fr ? &law : nullptr, fr ? &side[dir] : nullptr);
    if (rc != FB_OK) break;
    if (fr) friction_sums(recs[dir], side[dir], *fr, dir, FI);
    I.n_candidates[dir] = R.n_candidates; I.n_contacts[dir] = R.n_contacts;
    I.n_tet_grid_builds += R.tet_grids; I.n_face_grid_builds += R.face_grids;
    if (R.n_contacts > 0) I.path = R.path;
    double* on_p = dir == 0 ? I.force_on_a : I.force_on_b;
    double* on_t = dir == 0 ? I.force_on_b : I.force_on_a;
    ContactSums sums;
    sums.faces_tested = I.faces_tested; sums.max_depth = I.max_depth;
    for (int k = 0; k < 3; k++) { sums.on_points[k] = on_p[k]; sums.on_faces[k] = on_t[k]; }
    sums = contact_sums(recs[dir], prm.depth_cap, sums, [](size_t, const BodyContactRec&) { return true; });
    I.faces_tested = sums.faces_tested; I.n_degenerate[dir] = sums.n_degenerate; I.max_depth = sums.max_depth;
    for (int k = 0; k < 3; k++) { on_p[k] = sums.on_points[k]; on_t[k] = sums.on_faces[k]; }
  }
  // what b queues from here on runs after this call (also after a failure: the kernels launched so far read b's arrays)
  const hipError_t e1 = hipEventRecord(W.ev_out, s);
  const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(b->stream, W.ev_out, 0) : e1;
  FB_TRY(rc);
  FB_HIP(e1);
  FB_HIP(e2);
  if (add) {
    W.host[0].swap(recs[0]); W.host[1].swap(recs[1]);
    W.info = I;
    if (fr) { W.fric_host[0].swap(side[0]); W.fric_host[1].swap(side[1]); }
  }
  if (out) *out = I;
  if (fr && fout) *fout = FI;
  return FB_OK;
}

}  // namespace
}  // namespace fb

// ---- the C ABI ----

int fb_fem_body_contact(fb_fem_t a, fb_fem_t b, const fb_fem_body_contact_params* p, fb_fem_body_contact_info* out) {
  CHECK_HANDLE(a);
  CHECK_HANDLE(b);
  FB_TRY(check_pair(a, b, p));
  return body_contact(a, b, *p, true, nullptr, out);
}

int fb_fem_body_contact_friction(fb_fem_t a, fb_fem_t b, const fb_fem_body_contact_params* p, const fb_fem_contact_friction_params* fr, fb_fem_body_contact_info* out,
                                 fb_fem_contact_friction_info* fout) {
  CHECK_HANDLE(a);
  CHECK_HANDLE(b);
  FB_TRY(check_pair(a, b, p));
  FB_TRY(check_friction(fr, "fb_fem_body_contact_friction"));
  return body_contact(a, b, *p, true, nullptr, out, fr, fout);
}

int fb_fem_read_body_contact_friction(fb_fem_t a, int direction, double* normal_force, double* slip3, double* friction3) {
  CHECK_HANDLE(a);
  if (direction != FB_BODY_A_INTO_B && direction != FB_BODY_B_INTO_A) return fail(FB_EINVAL, "fb_fem_read_body_contact_friction: direction %d", direction);
  read_friction(a->bodyc.fric_host[direction == FB_BODY_A_INTO_B ? 0 : 1], normal_force, slip3, friction3);
  return FB_OK;
}

int fb_fem_read_body_contact(fb_fem_t a, int direction, int* node, int* element, int* face, double* closest_xyz, double* bary3, double* depth) {
  CHECK_HANDLE(a);
  if (direction != FB_BODY_A_INTO_B && direction != FB_BODY_B_INTO_A) return fail(FB_EINVAL, "fb_fem_read_body_contact: direction %d", direction);
  read_contacts(a->bodyc.host[direction == FB_BODY_A_INTO_B ? 0 : 1], node, element, face, closest_xyz, bary3, depth);
  return FB_OK;
}

int fb_fem_time_body_contact(fb_fem_t a, fb_fem_t b, const fb_fem_body_contact_params* p, int reps, double seconds[5]) {
  CHECK_HANDLE(a);
  CHECK_HANDLE(b);
  FB_TRY(check_pair(a, b, p));
  if (reps < 1 || !seconds) return fail(FB_EINVAL, "fb_fem_time_body_contact: reps must be positive and seconds not null");
  FB_TRY(body_contact(a, b, *p, false, nullptr, nullptr));  // warm: the buffers exist
  double sum[5] = {0, 0, 0, 0, 0};
  for (int r = 0; r < reps; r++) FB_TRY(body_contact(a, b, *p, false, sum, nullptr));
  for (int k = 0; k < 5; k++) seconds[k] = sum[k] / reps;
  return FB_OK;
}
