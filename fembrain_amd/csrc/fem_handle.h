// The FEM handle (fb_fem_t of include/fembrain_hip.h) and what the units that work on it share: fem.hip (assembly, the two-launch
// solver, the steps and the rest of the C ABI), fem_build.hip (life cycle: plan build, creation, re-sync, cut), fem_persist.hip (the
// persistent solver's host side), haptic.hip (the probe's entry points), stress.hip (element stress and strain), parts.hip (disjoint parts),
// detach.hip (a part into a handle of its own), embed.hip (point sets bound to the elements), embed_touch.hip (forces, picks and stress on them), contact.hip (the probe's box contact), body_contact.hip (contact between two handles), self_contact.hip (a handle with itself), tool_contact.hip (a rigid tool's shapes against the tissue) and motion.hip (constrained DOFs that follow a tool).
// Internal: not installed, included by these units only.
#pragma once
#include "comm.h"
#include "common.h"
#include "fem_kernels.h"
#include "fem_plan.h"
#include "plan_device.h"
#include "renumber.h"
#include "delta.h"
#include "subdivide.h"
#include "surface.h"
#include "haptic.h"
#include "stress.h"
#include "parts.h"
#include "detach.h"
#include "embed.h"
#include "contact.h"
#include "body_contact.h"
#include "self_contact.h"
#include "motion.h"
#include "tool_contact.h"

namespace fb {

struct PipeKernel;  // fem_persist.hip: one instantiation of k_pcg_pipe / k_pcg_pipe2

// The persistent solver's state in a handle (fem_persist.hip; pcg_pipe.hip.h), by lifetime.  Buffers keep their ALLOCATION across
// re-syncs (DevBuf::alloc) unless reset_plan() releases them: never reset this by assigning a fresh struct.
struct PersistState {
  // ---- per handle: survives every re-sync ----
  int pipe_mir_knob = -1;              // FEMBRAIN_PIPE_MIRROR as it was when the handle was made (-1: not read yet)
  int persist_fallbacks = 0;           // solves that had to be repeated with the two-launch form
  int persist_launches = 0;            // persistent launches made by this handle
  int persist_rearms = 0;
  double persist_seconds = 0;          // device seconds of all persistent launches of this handle (HIP events on its stream)
  long long persist_iterations = 0;    // PCG iterations they ran

  // ---- carried across small re-syncs: a re-sync that changes the mesh by a few per cent keeps the counts of the plan before it (the
  // read-back is a host wait; pipe_layout) ----
  int pipe_lines_nodes = 0;            // nodes of the plan the counts below were taken on
  double pipe_gather_lines[2] = {0, 0};  // cache lines a slot's gathers touch on average: three planes | 24-byte records (k_gather_lines; 0: not measured)

  // ---- per plan: decided by setup_persist for every (re)built plan; what reset_plan() does not touch is meaningful while `persist` or
  // `persist_broken` only ----
  // one workgroup per CU, `persist_waves` wavefronts = slices each, the whole solve in one launch
  bool persist = false;
  int persist_blocks = 0, persist_waves = 0;
  const PipeKernel* kernel = nullptr;  // the instantiation this plan launches (resolved once, at the end of the set-up)
  int pipe_rows = 1;                   // rows per lane: 1 = k_pcg_pipe (up to 12 slices per CU), 2 = k_pcg_pipe2 (13..24)
  int pipe_wmax = 0;                   // wavefronts the instantiation is built for (5 | 8 | 12)
  int pipe_slots_dealt = 0;            // LDS slots per slice that were dealt (fb_fem_persist_info) -- NOT the template's unroll bound, kernel->klt
  int pipe_help_waves = 0;             // wavefronts launched beyond slices + service wavefront, for the helpers (0: none)
  int pipe_n_help = 0, pipe_help_tasks = 0;  // most helper tasks of a workgroup; all of them
  bool pipe_xyz = false;               // the published vector node by node instead of in planes (irregular meshes; k_pcg_pipe<..., XYZ>)
  int pipe_plain_local = 0;            // interior workgroups publish with plain stores (FEMBRAIN_PIPE_PLAIN_STORES)
  int pipe_flag_extra = 0;             // flag slots after the workgroups' (the proxies' flags of a sharded handle)
  int pipe_max_producers = 0;          // longest producer list (-1: some workgroup polls all)
  bool pipe_stats_pending = false;     // ... still on the device (pipe_stats: [0] longest list, [1] someone polls all)
  int pipe_timing_level = 0;           // FEMBRAIN_PERSIST_TIMING as the plan build read it (print_pipe_timing)
  long long persist_timeout_ticks = 0; // wall_clock64 ticks (100 MHz) a wait inside a persistent launch may last (per plan and per re-arm)
  bool persist_broken = false;  // a launch timed out: the handle runs the two-launch iteration until it is re-armed (below) or re-synced
  // Re-arming: one co-tenant burst must not cost a 1M-tet host 40 % of its speed for the life of the handle.  After
  // `rearm_after` clean two-launch solves an unsharded handle tries the persistent launch again; every further time-out doubles the
  // wait (32, 64, 128, ... solves; FEMBRAIN_PERSIST_REARM=n sets the first, 0 = never).  A sharded handle re-arms at a re-sync only
  // (the ranks must switch together).
  int rearm_after = 32, clean_solves = 0;
  // sharded persistent solver (pcg_shard_box.hip.h; opt-in FEMBRAIN_SHARDED_PERSIST=1, unmeasured on multi-GPU hardware)
  bool shard_persist = false;
  int sh_n_proxy = 1, sh_relief = 0;
  char* sbox = nullptr;                // my box (fine-grained, mapped by the peers)
  void* sbox_opened[kP2PMaxRanks] = {nullptr};
  long long sbox_halo_cap = 0;
  // the LDS window of the one-row kernel (pcg_pipe_mirror.h; k_pipe_mirror_plan in setup_pipe_mirror), pipe_mir empty: none
  // (FEMBRAIN_PIPE_MIRROR=0, or another instantiation).  pipe_mir_stats: mirror layers, pool entries, fewest plain layers of a slice --
  // fetched when asked
  int pipe_mir_got[4] = {0, 0, 0, 0};  // (the fourth: register slots over all slices, fb_fem_persist_regs)
  int pipe_regs = 0;                   // register slots per slice this plan's launches may hold (pcg_pipe_regs.hip.h): the kernel's, capped by FEMBRAIN_PIPE_REGS
  bool pipe_mir_pending = false;

  // per plan, released by reset_plan(): a plan that does not use one must not find the previous plan's
  DevBuf<int> pipe_wg_first;           // the deal of the slices to the workgroups balanced by slots (pipe_deal), empty: equal numbers
  std::vector<int> pipe_wg_first_host;
  DevBuf<int4> pipe_mir;
  DevBuf<int> sh_halo_off, sh_row_send_off, sh_row_send_rank, sh_row_send_pos, sh_proxy_wg, sh_wg_duty;
  DevBuf<int2> sh_wg_range;
  DevBuf<unsigned int> sh_wg_send_mask;
  // per plan, released where the set-up finds them unused (pipe_tasks, persist_timing, the window's tables)
  DevBuf<int4> pipe_tasks;             // per workgroup and wavefront its share of the slices (helpers, pcg_pipe.hip.h PipeArgs)
  DevBuf<long long> persist_timing;    // FEMBRAIN_PERSIST_TIMING=1 (development aid)
  DevBuf<unsigned short> pipe_mir_addr;
  DevBuf<int2> pipe_mir_wg;
  DevBuf<int> pipe_mir_pool;
  // per plan, allocation kept from plan to plan
  DevBuf<int> pipe_mir_stats;
  DevBuf<unsigned long long> pipe_lines;  // k_gather_lines' three sums
  DevBuf<unsigned long long> pipe_post;
  DevBuf<unsigned int> pipe_flags;     // [blocks padded to 4] flags, [+4] the error word, [+8..9] the two sequence numbers
  DevBuf<int> pipe_prod, pipe_prod_count, pipe_prod_xcd;
  DevBuf<unsigned int> pipe_xcc;       // per workgroup: the XCC id it announced in the current launch (k_pcg_pipe: plain-store publish)
  DevBuf<double> pipe_planes, pipe_z, pipe_s, pipe_state;
  DevBuf<int> pipe_owner, pipe_stats;
  DevBuf<unsigned int> pipe_mask;
  DevBuf<char*> sbox_peers;
  DevBuf<int> sh_peer_seg, sh_n_senders;

  // What a plan build starts from.  Nothing of the previous plan's sharded persistent solver survives a rebuild: a re-sync to
  // a mesh that is no longer eligible must not leave attach_pipe_shard a stale "keep", stale send lists or a stale workgroup deal.
  // setup_persist_shard_local is the only place that sets shard_persist again; a fresh plan also gets a fresh chance after a time-out.
  void reset_plan(int rearm) {
    persist = false;
    kernel = nullptr;
    pipe_mir.release(); pipe_mir_pending = false;  // (setup_pipe_mirror plans the window again where it applies)
    pipe_mir_got[0] = pipe_mir_got[1] = pipe_mir_got[2] = pipe_mir_got[3] = 0;
    pipe_regs = 0;
    shard_persist = false;
    persist_broken = false;
    pipe_stats_pending = false;
    clean_solves = 0;
    rearm_after = rearm;
    sh_halo_off.release(); sh_row_send_off.release(); sh_row_send_rank.release(); sh_row_send_pos.release(); sh_proxy_wg.release();
    sh_wg_duty.release(); sh_wg_range.release(); sh_wg_send_mask.release();
    pipe_wg_first_host.clear();
    pipe_wg_first.release();
  }
};

// The environment knobs of the assembly and the SpMV.  read_host_knobs() (fem.hip) is the one place that reads them, once per plan build
// (upload_plan: handle creation and every re-sync; the three plan builders that decide c16 ask it too).  Nothing is cached per process.
struct HostKnobs {
  bool asm_rows = false, asm_tets1 = false;  // FEMBRAIN_ASM_KERNEL=rows: the slot-major kernel; =tets1: the unstaged element-major one (same bits)
  int asm_per_cu = 0;          // FEMBRAIN_ASM_PER_CU (development aid): at most so many element-major workgroups per CU; 0 = not set
  int asm_wide_grid = 0;       // FEMBRAIN_ASM_WIDE_GRID (tests: several slices per workgroup): at most so many workgroups of k_assemble_wide; 0 = not set
  bool asm_wide_rows = false;  // FEMBRAIN_ASM_WIDE_ROWS (development aid): the wide slices in the one-wavefront-per-slice form (same bits)
  bool asm_profile = false;    // FEMBRAIN_ASM_PROFILE: where the wavefronts of the element-major kernels spend their time, printed per assembly
  int spmv_nt = -1;            // FEMBRAIN_SPMV_NT=0/1: matrix values streamed non-temporally; -1 = not set, upload_plan's size rule
  bool spmv_c16 = true;        // FEMBRAIN_SPMV_C16=0: 32-bit column words even where the 16-bit ones fit
  bool verbose = false;        // FEMBRAIN_TIMING is set: the two assembly diagnostics of upload_plan
};

// What a plan launches of the assembly families, resolved from the table of their instantiations (fem.hip resolve_asm_kernels: for every
// plan, and again when a handle gets its element map).  [2]: without | with qacc; tets_st and mass: staged plans only
struct AsmKernels { const void *warp = nullptr, *rows = nullptr, *wide = nullptr, *k0 = nullptr, *mass = nullptr, *tets[2] = {nullptr, nullptr}, *tets_st[2] = {nullptr, nullptr}; };

}  // namespace fb

using namespace fb;  // (the units do; the handle's members are fb's types)

struct fb_fem_s {
  fb_fem_params prm;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;          // the slot-major assembly of the few slices too wide for the element-major kernel runs beside it (launch_rows)
  hipEvent_t ev_side[2] = {nullptr, nullptr};
  fb_comm_s* comm = nullptr;  // not owned
  P2P* p2p = nullptr;         // direct peer mailboxes for halo refresh and dots (comm.h); null = collective library
  int xch_mode = FB_XCH_COLLECTIVE;     // how the exchanges of a sharded handle run (fb_fem_set_exchange_mode)
  DevBuf<int> send_off_dev, halo_off_dev;
  DevBuf<unsigned char> slice_halo;
  FemPlan plan;
  double lambda = 0, mu = 0;
  int grid = 8;
  bool f64 = false;
  // Per-element materials (fb_fem_set_materials / fb_fem_set_element_materials).  The table lives on the host; entry 0 is prm.E / nu / rho
  // and what lambda / mu above are made of.  The element map and the device table exist only once a map was set: a handle without one
  // allocates nothing here and launches the kernels' uniform instantiations.
  std::vector<double> mat_E, mat_nu, mat_rho;    // 1 .. kMaxMaterials entries
  double force_scale = 1.0;                      // fb_fem_set_internal_force_scaling: scales every material's E
  bool map_from_delta = false;                   // fb_fem_resync_delta's full rebuild is running: build() leaves the map to it
  int mat_hi = 0;                                // upper bound of the ids in use (the table may not shrink to it or below)
  DevBuf<unsigned char> mat_ids, mat_ids_next;   // material id per element, caller's element order (at least one entry: padding lanes read element 0)
  DevBuf<double> mat_tab;                        // lambda | mu | rho/20, kMaxMaterials doubles each, padded with entry 0
  // mesh
  DevBuf<int4> tets;
  DevBuf<double> x0, rest, fe;
  DevBuf<char> rec;  // MT[16] per tet
  DevBuf<char> kcorr;  // exact tangent (warp = 2): MT[144] per tet, the rotation-derivative terms of the element stiffness
  // Newmark (ImplicitNewmarkSparse): acceleration and the state at the start of the step
  DevBuf<double> qacc, q1, qvel1, qacc1;
  double nm_beta = 0.25, nm_gamma = 0.5, nm_eps = 1e-6;
  int nm_max_newton = 1;
  bool pcg_warm = false;  // the next solve starts from the x left by the previous one (Newmark), not from 0
  // matrix
  DevBuf<int> slice_off, colidx, slot_coff, slot_ccnt, send_local;
  DevBuf<uint32_t> contrib;
  DevBuf<short> coldelta;  // 16-bit column words (device-built plans); c16 says whether the SpMV may use them and in which form:
  int c16 = 0;             // 0 no, 1 column - row (unsharded), 2 the halo form of a shard (plan_device.hip k_plan_sell)
  DevBuf<int> halo_base;   // c16 == 2: lowest halo column of every slice
  PlanWorkspace plan_ws;  // the device plan builder's temporaries, kept for the next re-sync
  MeshDelta delta;        // fb_fem_resync_delta: the change on the device and its scratch
  CutWork cut;            // fb_fem_cut: the last cut's codes, edges, pieces and new nodes (fb_fem_read_cut)
  DevBuf<double> carry;   // fb_fem_cut, FB_CUT_CARRY: the state in the caller's order across the re-sync
  SurfaceWork surf;       // fb_fem_surface: the boundary of the current mesh (surface.h); empty until somebody asks
  StressWork stress;      // fb_fem_stress: von Mises, energy density, J (and tensors) per element of the last call (stress.h); empty until somebody asks
  PartsWork parts;        // fb_fem_parts: face-connected parts of the current mesh (parts.h); empty until somebody asks
  DetachWork detach;      // fb_fem_detach_part: the constrained DOFs of the part being detached (detach.h); empty until somebody asks
  EmbedWork embed;        // fb_fem_embed: point sets bound to the elements, and their search grid (embed.h); empty until somebody asks
  ContactWork contact;    // fb_fem_contact_move / apply: the probe's touched set, force list and spread records (contact.h); empty until somebody asks
  BodyContactWork bodyc;  // fb_fem_body_contact: contact with another handle, kept in the handle the call names first (body_contact.h); empty until somebody asks
  SelfContactWork selfc;  // fb_fem_self_contact: contact of this handle with itself (self_contact.h); empty until somebody asks
  ToolContactWork toolc;  // fb_fem_tool_contact: a rigid tool's spheres, capsules and boxes against the points (tool_contact.h); empty until somebody asks
  MotionWork motion;      // fb_fem_set_constrained_motion / fb_fem_grasp: the moved constrained DOFs, their element table and reactions (motion.h); empty until somebody asks
  HapticWork hap;         // fb_fem_add_haptic_forces / pick / volume: level array and scratch (haptic.h); empty until somebody asks
  std::vector<int> fixed_caller;  // the constrained DOFs in the caller's numbering (unsharded): what fb_fem_cut keeps
  DevBuf<int4> tets_next, tets_caller;   // (the element list being built; swapped with `tets`)
  DevBuf<double> x0_next;
  DevBuf<int> map_next_a, map_next_b;
  int last_resync_path = FB_RESYNC_FULL;
  int ren_nodes_at_build = 0;  // nodes when the internal order was last built from scratch
  DevBuf<int> flat_flag;
  DevBuf<int> inc_off;               // element-major assembly (k_assemble_tets): incidence lists per slice, see fem_device.hip.h
  DevBuf<uint32_t> inc, inc_slot;
  bool asm_tets = false;             // the assembly kernel in use
  int asm_lds = 0, asm_grid = 0, asm_max_width = 0;
  int asm_wide = 0;                  // slices wider than the element-major kernel takes (kIncMaxWidth slots): k_assemble_wide assembles those
  int asm_wide_slots = 0, asm_wide_grid = 0;  // the widest of them; workgroups of k_assemble_wide (each with a scratch area of asm_wide_slots slots)
  DevBuf<int> wide_list;             // their slice numbers
  DevBuf<double> res_all;            // Newmark, several Newton iterations: the residual of every DOF (AsmOut::res_all)
  DevBuf<double> wide_scratch;
  bool asm_staged = false;           // k_assemble_tets_st (records staged in LDS, mass entries precomputed) instead of k_assemble_tets
  int asm_lds_st = 0, asm_grid_st = 0;
  bool mass_valid = false;           // h->mblk holds the mass entries of the current rest data (k_mass_blocks)
  fb::HostKnobs knobs;               // as the last plan build read them
  fb::AsmKernels asm_k;              // the assembly kernels of this plan
  // Per mesh generation -- begin_mesh_generation (fem_build.hip) is the one place that resets them, for build(), its host-builder fallback
  // and fb_fem_resync_delta: ren, l2c, order_sum, x0_ready, masks_ready, caller_pattern, csr_ready, span_stale (all below), the embeddings' grid and bindings (embed_mesh_changed), the contact session (contact_mesh_changed), surf.valid,
  // stress.valid, parts.valid and motion.table_valid (above); batch_graph is dropped with them.  (fb_fem_resync_delta keeps ren, and csr_ready while it decides, and says so.)
  // locality renumbering behind the ABI (renumber.h): the handle works in its own node order, ids are mapped on the way in and out
  Renumbering ren;
  DevBuf<double> xyz_in;               // the caller-order rest positions the order was derived from
  DevBuf<double> io;                   // staging of a caller-order vector on its way to / from the internal order
  bool x0_ready = false;               // build_plan_on_device has put the (permuted) rest positions in place already
  bool masks_ready = false;            // ... and the constraint masks (device_constraint_masks)
  std::vector<int> l2c;                // a renumbered SHARDED handle: caller id of every local node (owned, then halo); empty otherwise
  unsigned long long order_sum = 0;    // ... and a checksum of the order, compared across the ranks
  int n_cu_device = 256;               // CUs of the device (FB_MATRIX_AUTO's size rule; setup_persist asks the device itself)
  bool shard_auto_on = false;          // FB_RENUMBER_AUTO on a sharded handle: the ranks voted for the internal order (vote_shard_order)
  int shard_vote_neighbours = 0;       // most neighbour ranks any rank would have had under the caller's numbering (what the vote saw)
  DevBuf<int> fixed_stage;
  std::vector<int> c_bptr, c_bcol, c_src;  // the pattern in the caller's numbering and the internal block behind each of its blocks (inspection entry points)
  bool caller_pattern = false;
  std::vector<double> x0_stage;  // host staging of the rest positions in local numbering (kept: a re-sync does not fault fresh pages)
  DevBuf<int> d_bptr, d_bcol, d_blk_slot;  // device-built plan only: pattern and slot table, fetched when an inspection entry point asks
  DevBuf<unsigned int> d_ucnt;             // ... and the pairs of every block (unsharded): with the three above and the contribution table, what fb_fem_resync_delta updates
  bool span_stale = false;                 // ren.span_after / mean_after are to be measured again (fb_fem_renumbering)
  bool csr_ready = false;                  // the four describe the current plan
  bool device_plan = false, host_pattern = true;
  DevBuf<uint8_t> dofmask;
  DevBuf<uint8_t> nodemask;  // the three dofmask bytes of a node as bits 0..2 (one gather per column in the assembly)
  DevBuf<char> vals;  // MT[n_slots][9][64]
  DevBuf<char> dlo;   // MT[n_slices][9][64]: low part of every row's diagonal block
  DevBuf<double> mblk;
  DevBuf<float> volf;                // rest volumes as the fp32 records hold them (k_tet_rest -> k_mass_blocks)
  DevBuf<double> invblk;  // FB_PCG_BLOCK_JACOBI: inverse 3x3 diagonal block per row
  // vectors (3*n_local each)
  DevBuf<double> q, qvel, fext, fint, rhs, x, r, d, Ad, invdiag, tmp, sendbuf;
  DevBuf<double> part_a, part_b, part_c, scal;
  DevBuf<CGState> st;
  DevBuf<int> counter;
  CGState* st_host = nullptr;  // pinned, 2 slots
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr}, ev_batch[2] = {nullptr, nullptr};
  bool system_valid = false;
  bool poisoned = false;  // a re-sync failed half way: the buffers no longer belong to one mesh; only a successful re-sync (or destroy) is accepted
  double last_assembly_s = 0, last_solve_s = 0;
  // one batch of 30 PCG iterations (29 merged + the exact-residual one) captured once and replayed: the launch sequence
  // and every kernel argument repeat from batch to batch, and on meshes of ~100k tets the host's launch rate, not the
  // device, would otherwise bound the iteration time
  int split = 0;       // wavefronts per slice of the SpMV on small / mid-size meshes (k_spmv_split): 0 (row kernel), 2 or 4
  int sgrid = 8;       // blocks (= partial sums) of the SpMV launches; equals grid unless split
  bool spmv_nt = false;  // stream the matrix values non-temporally (systems larger than the Infinity Cache, see k_spmv)
  const void* spmv_fn[4] = {nullptr, nullptr, nullptr, nullptr};  // the SpMV of this plan by MODE (fem.hip resolve_spmv_kernels), and
  const void* spmv_xch_fn = nullptr;                              // MODE 3 with the halo refresh in its prologue (XCH = 2)
  int vgrid = 8;       // blocks of the merged vector pass: one 16-byte pair per thread
  hipGraphExec_t batch_graph = nullptr;
  const double* graph_rhs = nullptr;
  bool use_graph = true;
  bool literal_now = false, graph_literal = false;  // this solve runs the literal two-reduction sequence (tolerance below kPersistMinEps); what the captured batch runs
  fb::PersistState ps;                 // the persistent solver (fem_persist.hip)
  int last_pcg_path = 0;               // FB_PCG_PATH_* of the last solve
  int cu_limit = 0;                    // > 0: the stream is confined to this many CUs (FEMBRAIN_CU_MASK)
  hipEvent_t ev_p[2] = {nullptr, nullptr};  // around every persistent launch
};

namespace fb {

inline bool motion_active(const fb_fem_s* h) { return !h->motion.dofs.empty(); }  // (no set: the step launches nothing of motion.hip)
inline bool has_material_map(const fb_fem_s* h) { return h->mat_ids.p != nullptr; }  // (none: nothing allocated, the kernels' uniform instantiations)

inline SellView sell_view(const fb_fem_s* h) {
  SellView sv;
  sv.slice_off = h->slice_off.p; sv.colidx = h->colidx.p; sv.n_slices = h->plan.n_slices; sv.n_owned = h->plan.n_owned;
  sv.coldelta = h->c16 ? h->coldelta.p : nullptr;
  sv.halo_base = h->c16 == 2 ? h->halo_base.p : nullptr;
  return sv;
}

#define CHECK_HANDLE(h)                                                                                                        \
  if (!(h)) return fail(FB_EINVAL, "null FEM handle");                                                                        \
  if ((h)->poisoned) return fail(FB_EINVAL, "handle unusable after a failed fb_fem_resync: re-sync it with a valid mesh or destroy it"); \
  FB_HIP(hipSetDevice((h)->prm.device))

// Zero fills of a (re-)build, batched: about twenty buffers are cleared, and a fill per buffer costs 4-5 us of launch each however
// small it is.  add() notes them (4-byte granularity), flush() clears up to kZeroMax per launch.
constexpr int kZeroMax = 24;
struct ZeroBatch {   // (fem.hip, next to its kernel)
  unsigned int* p[kZeroMax]; unsigned long long end[kZeroMax]; unsigned int tail_words[kZeroMax]; int n = 0;  // end: running total of 16-byte chunks
  hipStream_t s;
  int rc = FB_OK;
  explicit ZeroBatch(hipStream_t stream) : s(stream) {}
  // p: 16-byte aligned (the start of an allocation); bytes: a multiple of 4 (else the runtime's fill takes it)
  void add(void* p, size_t bytes);
  template <typename T>
  void add(DevBuf<T>& b) { add(b.p, b.n * sizeof(T)); }
  int flush();
};

// fem.hip
int assemble_system(fb_fem_s* h);
int handle_slack_now(const fb_fem_s* h);   // the slack rule of this handle's allocations at its current mesh (SlackScope)
int surface_current(fb_fem_s* h);          // builds the surface where it is stale (fb_fem_surface_update's first step)
// fem_build.hip
int refresh_node_order(fb_fem_s* h);      // a renumbered handle whose rest positions moved: built again in the order a new handle would get, state and forces carried
// an unsharded handle from a mesh on its device (fp64 positions, local ids), on a stream of its own: fb_fem_create without the host hop
int create_from_device_mesh(fb_fem_t* out, const DeviceTetMesh& dm, int n_fixed, const int* fixed, const fb_fem_params* params);
// fb_fem_resync_delta(removed = the ascending device list) with q, qvel, (qaccel) and the external forces carried; a failure poisons the handle
int remove_elements_device(fb_fem_s* h, int n_removed, const int* d_removed);
// ... and what fem_build.hip builds a handle with
int handle_slack(const fb_fem_s* h, int n_nodes, int n_tets);  // the slack rule at a mesh of this size
int renumber_mode(const fb_fem_s* h);      // FB_RENUMBER_* of this handle
HostKnobs read_host_knobs();
int upload_masks(fb_fem_s* h);             // the plan's constraint mask to the device (host-built plans, sharded handles)
int upload_plan(fb_fem_s* h, const double* xyz_global, const float* xyz_device = nullptr, const double* xyz_device64 = nullptr);  // everything per plan
int launch_rest(fb_fem_s* h, int* first_flat = nullptr);
void drop_graph(fb_fem_s* h);
int widen_positions(hipStream_t s, long long n, const float* in, double* out);  // float positions handed over on the device -> doubles
int download_owned(fb_fem_s* h, const DevBuf<double>& src, double* g);          // owned part of a device vector -> its place in a global-length host vector
// the material side of a handle made from elements of `src`: force scaling and table, and -- ids non-null -- the filled element map (swapped in)
int inherit_materials(fb_fem_s* h, const fb_fem_s* src, DevBuf<unsigned char>* ids);

// stress.hip: FB_EINVAL with who's name unless h holds a fb_fem_stress of its current mesh
int stress_current(const fb_fem_s* h, const char* who);
// embed.hip: the embedding of a slot, its orphans searched first (FB_EINVAL: a sharded handle, no such embedding)
int embedding_current(fb_fem_s* h, int id, Embedding** out);

// parts.hip
PartsMesh parts_mesh(fb_fem_s* h);         // the handle's arrays the calls of parts.h work on
int parts_current(fb_fem_s* h, bool force = false);  // builds the labels where they are stale (what fb_fem_parts does first); force: in any case

// fem_persist.hip
bool auto_matrix_f64(const fb_fem_s* h, int n_nodes, int n_ranks);
int setup_persist(fb_fem_s* h);            // for every (re)built plan
int attach_pipe_shard(fb_fem_s* h);        // the collective half of the sharded set-up
void release_shard_persist(fb_fem_s* h);
void read_persist_timeout(fb_fem_s* h);
int launch_pipe(fb_fem_s* h, const double* b, int start, int n_iters, double eps, int max_iter);
void print_pipe_timing(fb_fem_s* h);
int persist_plan_array(fb_fem_s* h, const char* name, std::vector<int>* out);  // fb_fem_device_plan_get's pipe_* names

}  // namespace fb
