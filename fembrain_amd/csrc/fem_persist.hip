// Host side of the persistent solver (k_pcg_pipe / k_pcg_pipe2, pcg_pipe*.hip.h): its knobs, the table of its instantiations, the
// set-up of a plan, the one launch, and the entry points that report on it.  The only unit that includes the kernels' headers.
// The two-launch solver and pcg_solve_pipe, which falls back to it, are in fem.hip; the seam is fem_handle.h.
#include <cmath>
#include <cstring>

#include "fem_handle.h"
#include "pcg_pipe.hip.h"
#include "pcg_pipe2.hip.h"
#include "pcg_pipe_plan.h"

using namespace fb;

namespace fb {

// One instantiation of the persistent kernel: what selects it, and its address.
struct PipeKernel {
  int rows;             // rows per lane: 1 = k_pcg_pipe, 2 = k_pcg_pipe2
  bool c16;             // 16-bit column words
  int wmax, klt;        // wavefronts it is built for; most LDS slots per wavefront (the unroll bound of the loop over resident slots)
  bool timing, shard, bj, help, xyz;
  bool ahead;           // the run-ahead form: for launches with a service wavefront (pcg_pipe.hip.h)
  int regs;             // register slots per slice it holds (pcg_pipe_regs.hip.h), 0: none
  int prio;             // wavefront priority through the product (pcg_pipe.hip.h): 0 none, 1 progress, 2 static, 3 progress + service wavefront
  const void* fn;
};

namespace {

// The instantiations, all of them: (wavefronts, most LDS slots per wavefront) = (8, 8) up to 8 slices per CU, (12, 6) up to 12 -- (12, 7)
// at 9 and 10 --, (5, 16) on request (PersistKnobs::small); 16- or 32-bit column words; two rows per lane (k_pcg_pipe2) for 13..24 slices
// per CU; SHARD on a sharded handle (32-bit local column ids); TIMING: the development build with the phase clocks, for the 1M-tet
// configuration, the small ones and the helpers'; BJ: the block preconditioner; HELP: the task table, which also carries XYZ.  Every
// unsharded one-row kernel without the task table comes in two forms, one per launch form: with its barriers (as many slices as
// wavefronts) and run-ahead (a service wavefront); the others keep their barriers with or without a service wavefront.  The run-ahead LDS-window
// kernels of the plain Jacobi solver -- (12, 6) and (12, 7), the headline's -- come a second time with register slots (k_pcg_pipe_regs, REGS = 3);
// FEMBRAIN_PIPE_REGS=0 launches the one without.  Those four, and the TIMING (12, 6) run-ahead pair for the phase tables, come once more per priority
// form (PRIO = 1, 2, 3; FEMBRAIN_PIPE_PRIO picks, 0 launches the one without).
#define FB_PIPE1F(C16, WMAX, KLT, TIMING, SHARD, BJ, HELP, XYZ, AHEAD, REGS) \
  {1, C16, WMAX, KLT, TIMING, SHARD, BJ, HELP, XYZ, AHEAD, REGS, 0, (const void*)k_pcg_pipe<float, C16, WMAX, KLT, TIMING, SHARD, BJ, HELP, XYZ, AHEAD, REGS>}
#define FB_PIPE1(C16, WMAX, KLT, TIMING, SHARD, BJ, HELP, XYZ) FB_PIPE1F(C16, WMAX, KLT, TIMING, SHARD, BJ, HELP, XYZ, false, 0)
#define FB_PIPE1A(C16, WMAX, KLT, TIMING, BJ) FB_PIPE1F(C16, WMAX, KLT, TIMING, false, BJ, false, false, true, 0)
#define FB_PIPE1R(C16, KLT) \
  {1, C16, 12, KLT, false, false, false, false, false, true, kPipeRegsMax, 0, (const void*)k_pcg_pipe_regs<float, C16, 12, KLT, false, false, false, false, false, true, kPipeRegsMax>}
#define FB_PIPE1RP(C16, KLT, PRIO) \
  {1, C16, 12, KLT, false, false, false, false, false, true, kPipeRegsMax, PRIO, (const void*)k_pcg_pipe_regs<float, C16, 12, KLT, false, false, false, false, false, true, kPipeRegsMax, PRIO>}
#define FB_PIPE1TP(C16, PRIO) \
  {1, C16, 12, 6, true, false, false, false, false, true, 0, PRIO, (const void*)k_pcg_pipe<float, C16, 12, 6, true, false, false, false, false, true, 0, PRIO>}
#define FB_PIPE2(C16, SHARD, XYZ) {2, C16, 12, kPipe2Klt, false, SHARD, false, false, XYZ, false, 0, 0, (const void*)k_pcg_pipe2<C16, SHARD, XYZ>}
const PipeKernel kPipeKernels[] = {
    FB_PIPE1(true, 5, 16, false, false, false, false, false),  FB_PIPE1(false, 5, 16, false, false, false, false, false),
    FB_PIPE1(true, 8, 8, false, false, false, false, false),   FB_PIPE1(false, 8, 8, false, false, false, false, false),
    FB_PIPE1(true, 12, 6, false, false, false, false, false),  FB_PIPE1(false, 12, 6, false, false, false, false, false),
    FB_PIPE1(true, 12, 7, false, false, false, false, false),  FB_PIPE1(false, 12, 7, false, false, false, false, false),
    FB_PIPE1(true, 5, 16, true, false, false, false, false),
    FB_PIPE1(true, 8, 8, true, false, false, false, false),    FB_PIPE1(false, 8, 8, true, false, false, false, false),
    FB_PIPE1(true, 12, 6, true, false, false, false, false),   FB_PIPE1(false, 12, 6, true, false, false, false, false),
    FB_PIPE1(false, 8, 8, false, true, false, false, false),   FB_PIPE1(false, 12, 6, false, true, false, false, false),
    FB_PIPE1(true, 8, 8, false, false, true, false, false),    FB_PIPE1(false, 8, 8, false, false, true, false, false),
    FB_PIPE1(true, 12, 6, false, false, true, false, false),   FB_PIPE1(false, 12, 6, false, false, true, false, false),
    FB_PIPE1(true, 12, 6, false, false, false, true, false),   FB_PIPE1(false, 12, 6, false, false, false, true, false),
    FB_PIPE1(true, 12, 6, false, false, false, true, true),    FB_PIPE1(false, 12, 6, false, false, false, true, true),
    FB_PIPE1(true, 12, 6, true, false, false, true, false),    FB_PIPE1(false, 12, 6, true, false, false, true, false),
    FB_PIPE1(true, 12, 6, true, false, false, true, true),     FB_PIPE1(false, 12, 6, true, false, false, true, true),
    FB_PIPE1A(true, 5, 16, false, false),  FB_PIPE1A(false, 5, 16, false, false),  FB_PIPE1A(true, 8, 8, false, false),   FB_PIPE1A(false, 8, 8, false, false),
    FB_PIPE1A(true, 12, 6, false, false),  FB_PIPE1A(false, 12, 6, false, false),  FB_PIPE1A(true, 12, 7, false, false),  FB_PIPE1A(false, 12, 7, false, false),
    FB_PIPE1A(true, 5, 16, true, false),   FB_PIPE1A(true, 8, 8, true, false),     FB_PIPE1A(false, 8, 8, true, false),
    FB_PIPE1A(true, 12, 6, true, false),   FB_PIPE1A(false, 12, 6, true, false),
    FB_PIPE1A(true, 8, 8, false, true),    FB_PIPE1A(false, 8, 8, false, true),    FB_PIPE1A(true, 12, 6, false, true),   FB_PIPE1A(false, 12, 6, false, true),
    FB_PIPE1R(true, 6),  FB_PIPE1R(false, 6),  FB_PIPE1R(true, 7),  FB_PIPE1R(false, 7),
    FB_PIPE1RP(true, 6, 1),  FB_PIPE1RP(false, 6, 1),  FB_PIPE1RP(true, 7, 1),  FB_PIPE1RP(false, 7, 1),  FB_PIPE1TP(true, 1),  FB_PIPE1TP(false, 1),
    FB_PIPE1RP(true, 6, 2),  FB_PIPE1RP(false, 6, 2),  FB_PIPE1RP(true, 7, 2),  FB_PIPE1RP(false, 7, 2),  FB_PIPE1TP(true, 2),  FB_PIPE1TP(false, 2),
    FB_PIPE1RP(true, 6, 3),  FB_PIPE1RP(false, 6, 3),  FB_PIPE1RP(true, 7, 3),  FB_PIPE1RP(false, 7, 3),  FB_PIPE1TP(true, 3),  FB_PIPE1TP(false, 3),
    FB_PIPE2(true, false, false),  FB_PIPE2(false, false, false),  FB_PIPE2(true, false, true),  FB_PIPE2(false, false, true),
    FB_PIPE2(false, true, false),
};
#undef FB_PIPE2
#undef FB_PIPE1TP
#undef FB_PIPE1RP
#undef FB_PIPE1R
#undef FB_PIPE1A
#undef FB_PIPE1
#undef FB_PIPE1F
static_assert(sizeof(double) * kPipeSyncDoubles + (size_t)kPipeMaxWaves * 2 * kPipe2LdsWordsPerRow * 64 * 4 <= 160 * 1024, "LDS budget of k_pcg_pipe2");

int env_int(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}

// A launch has one wavefront more than slices where the instantiation has room: it collects the sums while the others multiply.
bool pipe_has_service(const PersistState& ps) {
  const int cwaves = ps.pipe_rows == 2 ? ceil_div(ps.persist_waves, 2) : ps.persist_waves;  // wavefronts that own slices
  return cwaves + ps.pipe_help_waves < ps.pipe_wmax;
}

PersistKnobs read_persist_knobs() {
  PersistKnobs k;
  k.pcg_persist = env_int("FEMBRAIN_PCG_PERSIST", -1);
  k.min_waves = env_int("FEMBRAIN_PERSIST_MIN_WAVES", 2);
  k.rows2 = env_int("FEMBRAIN_PERSIST_ROWS", 0) == 2;
  k.rearm = std::max(0, env_int("FEMBRAIN_PERSIST_REARM", 32));
  k.timing = getenv("FEMBRAIN_PERSIST_TIMING") ? std::max(1, env_int("FEMBRAIN_PERSIST_TIMING", 1)) : 0;  // (set, whatever to: on)
  k.poll_all = env_int("FEMBRAIN_PERSIST_POLL_ALL", 0) != 0;
  k.sharded = env_int("FEMBRAIN_SHARDED_PERSIST", 0) != 0;
  k.shard_relief = env_int("FEMBRAIN_SHARD_RELIEF", -1);
  k.balance = env_int("FEMBRAIN_PIPE_BALANCE", -1);
  k.small = env_int("FEMBRAIN_PIPE_SMALL", 0) != 0;
  k.klt7 = env_int("FEMBRAIN_PIPE_KLT7", 1) != 0;
  k.helpers = env_int("FEMBRAIN_PIPE_HELPERS", -1);
  k.help_minlen = env_int("FEMBRAIN_PIPE_HELP_MINLEN", 16);
  k.xyz = env_int("FEMBRAIN_PIPE_XYZ", -1);
  k.lds_by_width = env_int("FEMBRAIN_PIPE_LDS_BY_WIDTH", 0) != 0;
  k.lds_cap = getenv("FEMBRAIN_PIPE_LDS_CAP") ? std::max(1, env_int("FEMBRAIN_PIPE_LDS_CAP", 1)) : 0;
  k.plain_stores = env_int("FEMBRAIN_PIPE_PLAIN_STORES", -1);
  k.mirror = env_int("FEMBRAIN_PIPE_MIRROR", 1) != 0;
  k.regs = env_int("FEMBRAIN_PIPE_REGS", -1);
  k.prio = env_int("FEMBRAIN_PIPE_PRIO", -1);
  k.verbose = getenv("FEMBRAIN_TIMING") != nullptr;
  return k;
}

// The row of the table this plan launches, from what the set-up decided; stored in the handle.  A combination that was not built is
// refused here.  (12, 7): 9 or 10 slices per CU in the plain 12-wavefront kernel -- unsharded Jacobi handles without the task table.
int resolve_pipe_kernel(fb_fem_s* h, const PersistKnobs& kn) {
  PersistState& ps = h->ps;
  PipeKernel want;
  want.rows = ps.pipe_rows;
  want.shard = ps.shard_persist;
  want.bj = h->prm.pcg_variant == FB_PCG_BLOCK_JACOBI;  // (setup_persist: unsharded, one row per lane)
  want.help = ps.pipe_tasks.p != nullptr;               // (one row per lane)
  want.xyz = ps.pipe_xyz;
  want.c16 = !want.shard && h->c16 != 0;                // (a shard's columns are 32-bit local ids)
  want.timing = ps.persist_timing.p != nullptr && want.rows == 1;
  if (want.bj && want.timing) return fail(FB_EINVAL, "FEMBRAIN_PERSIST_TIMING is built for the Jacobi kernel");
  const bool klt7 = kn.klt7 && want.rows == 1 && ps.pipe_wmax == 12 && !want.shard && !want.bj && !want.help && !want.timing &&
                    (ps.persist_waves == 9 || ps.persist_waves == 10);
  want.wmax = ps.pipe_wmax;
  want.ahead = want.rows == 1 && !want.shard && !want.help && pipe_has_service(ps);
  want.klt = want.rows == 2 ? kPipe2Klt : (want.wmax == 5 ? 16 : (want.wmax == 8 ? 8 : (klt7 ? 7 : 6)));
  // register slots: the run-ahead LDS-window kernels of a handle that keeps its window; FEMBRAIN_PIPE_REGS caps them (0: the kernel without)
  const bool regs_form = want.rows == 1 && want.wmax == 12 && want.ahead && !want.timing && !want.bj && !want.xyz && ps.pipe_mir_knob != 0 && kn.regs != 0;
  want.regs = regs_form ? kPipeRegsMax : 0;
  ps.pipe_regs = kn.regs < 0 ? want.regs : std::min(kn.regs, want.regs);
  // wavefront priority: the kernels with register slots, and the TIMING (12, 6) run-ahead kernel; FEMBRAIN_PIPE_PRIO picks the form (0: the kernel without)
  const bool prio_form = regs_form || (want.rows == 1 && want.wmax == 12 && want.klt == 6 && want.ahead && want.timing && !want.bj && !want.xyz);
  want.prio = prio_form ? (kn.prio < 0 ? kPipePrioDefault : std::min(kn.prio, 3)) : 0;
  ps.kernel = nullptr;
  for (const PipeKernel& k : kPipeKernels)
    if (k.rows == want.rows && k.c16 == want.c16 && k.wmax == want.wmax && k.klt == want.klt && k.timing == want.timing && k.shard == want.shard && k.bj == want.bj &&
        k.help == want.help && k.xyz == want.xyz && k.ahead == want.ahead && k.regs == want.regs && k.prio == want.prio)
      ps.kernel = &k;
  if (!ps.kernel) return fail(FB_EINVAL, "FEMBRAIN_PERSIST_TIMING is built for one row per lane: (12, 6) and (5, 16) with 16-bit column words, (8, 8)");
  return FB_OK;
}

// The rank-local half of the sharded persistent solver's set-up (pcg_shard_box.hip.h): planes over owned + halo columns, per-row send
// lists, producer lists with the proxies' flags.  The collective half (boxes, sender counts) is attach_pipe_shard.
int setup_persist_shard_local(fb_fem_s* h, int nb, int w, const PersistKnobs& kn) {
  const FemPlan& P = h->plan;
  PersistState& ps = h->ps;
  hipStream_t s = h->stream;
  const int R = P.n_ranks;
  if (R > kP2PMaxRanks) return FB_OK;
  FB_TRY(ps.sh_halo_off.upload(P.halo_off, s));
  // per slice: its owned column range and the ranks whose halo rows it gathers
  DevBuf<int4> range;
  FB_TRY(range.alloc((size_t)std::max(1, P.n_slices)));
  hipLaunchKernelGGL(k_slice_colrange_shard, dim3(ceil_div(std::max(1, P.n_slices), kWavesPerBlock)), dim3(kBlock), 0, s, P.n_slices, P.n_owned, R, h->slice_off.p,
                     h->colidx.p, ps.sh_halo_off.p, range.p);
  FB_HIP(hipGetLastError());
  std::vector<int4> rg((size_t)std::max(1, P.n_slices));
  FB_TRY(range.download(rg.data(), rg.size(), s));
  std::vector<int2> wg_range;
  w = shard_deal(rg, P.n_slices, nb, w, kn, &wg_range, &ps.sh_relief);
  ps.pipe_rows = w < kPipeMaxWaves ? 1 : 2;   // 12..22 slices per CU: two rows per lane (k_pcg_pipe2_shard)
  ps.pipe_wmax = ps.pipe_rows == 2 ? 12 : (w < 8 ? 8 : 12);   // (one wavefront more than slices / slice pairs: the spare one serves the proxies and the sums)
  ps.pipe_slots_dealt = ps.pipe_rows == 2 ? std::min(kPipe2Klt, pipe2_lds_slots(w, false) / std::max(w, 1)) : std::min(ps.pipe_wmax == 8 ? 8 : 6, pipe_lds_slots(false) / std::max(w, 1));  // (a shard's columns are 32-bit)
  ps.persist_blocks = nb; ps.persist_waves = w;
  ps.pipe_flag_extra = kP2PMaxRanks * kShardProxies;
  FB_TRY(ps.sh_wg_range.upload(wg_range, s));
  FB_TRY(ps.pipe_post.alloc((size_t)2 * nb * 4));
  FB_TRY(ps.pipe_post.zero(s));
  FB_TRY(ps.pipe_flags.alloc((size_t)nb + ps.pipe_flag_extra + 16));
  FB_TRY(ps.pipe_flags.zero(s));
  const size_t n_pad = (size_t)ceil_div(P.n_local, 64) * 64, nv = (size_t)3 * P.n_local + 2;
  FB_TRY(ps.pipe_planes.alloc(2 * 3 * n_pad));
  FB_TRY(ps.pipe_planes.zero(s));
  FB_TRY(ps.pipe_z.alloc(nv));
  FB_TRY(ps.pipe_s.alloc(nv));
  FB_TRY(ps.pipe_state.alloc(2));
  FB_TRY(ps.pipe_state.zero(s));
  ps.persist_timing.release();
  std::vector<int> owner((size_t)P.n_slices, 0);
  for (int b = 0; b < nb; b++)
    for (int k = 0; k < wg_range[b].y; k++) owner[wg_range[b].x + k] = b;
  const ShardSendLists sl = shard_send_lists(P, owner, nb);
  FB_TRY(ps.sh_row_send_off.upload(sl.row_off, s));
  FB_TRY(ps.sh_row_send_rank.upload(sl.row_rank, s));
  FB_TRY(ps.sh_row_send_pos.upload(sl.row_pos, s));
  FB_TRY(ps.sh_wg_send_mask.upload(sl.wg_mask, s));
  std::vector<int> proxy, duty, prod, cnt, far((size_t)nb, 1);
  const int K = shard_proxies(P, nb, &proxy, &duty);
  ps.sh_n_proxy = K;
  FB_TRY(ps.sh_proxy_wg.upload(proxy, s));
  FB_TRY(ps.sh_wg_duty.upload(duty, s));
  ps.pipe_max_producers = shard_producers(rg, wg_range, owner, proxy, P.n_slices, nb, R, K, &prod, &cnt);
  ps.pipe_stats_pending = false;
  FB_TRY(ps.pipe_prod.upload(prod, s));
  FB_TRY(ps.pipe_prod_count.upload(cnt, s));
  FB_TRY(ps.pipe_prod_xcd.upload(far, s));
  ps.pipe_plain_local = 0;
  ps.shard_persist = true;  // (confirmed or withdrawn by attach_pipe_shard, collectively)
  return resolve_pipe_kernel(h, kn);
}

// The LDS window of the one-row (12, 6) / (12, 7) kernel (pcg_pipe_mirror.h): planned on the device for every (re)built plan -- for the
// unroll bound of the row resolve_pipe_kernel stored --, so a full re-sync, both outcomes of a delta re-sync and a fresh node order all
// get the table of their own plan.  FEMBRAIN_PIPE_MIRROR=0 when the handle is made: none.
int setup_pipe_mirror(fb_fem_s* h) {
  const FemPlan& P = h->plan;
  PersistState& ps = h->ps;
  hipStream_t s = h->stream;
  const PipeKernel& K = *ps.kernel;
  ps.pipe_mir_pending = false;
  ps.pipe_mir_got[0] = ps.pipe_mir_got[1] = ps.pipe_mir_got[2] = ps.pipe_mir_got[3] = 0;
  if (ps.pipe_mir_knob == 0 || K.rows != 1 || K.wmax != 12 || K.shard || K.help || K.bj || ps.pipe_xyz || P.n_slices <= 0) {
    ps.pipe_mir.release(); ps.pipe_mir_addr.release(); ps.pipe_mir_wg.release(); ps.pipe_mir_pool.release();
    return FB_OK;
  }
  const int nb = ps.persist_blocks;
  FB_TRY(ps.pipe_mir.alloc((size_t)nb * kMirWaves));
  FB_TRY(ps.pipe_mir_addr.alloc((size_t)P.n_slices * kMirMax * 64));
  FB_TRY(ps.pipe_mir_wg.alloc((size_t)nb));
  FB_TRY(ps.pipe_mir_pool.alloc((size_t)nb * kMirPoolMax));
  FB_TRY(ps.pipe_mir_stats.alloc(4));
  FB_HIP(hipMemsetAsync(ps.pipe_mir_stats.p, 0, 2 * sizeof(int), s));
  FB_HIP(hipMemsetAsync(ps.pipe_mir_stats.p + 3, 0, sizeof(int), s));
  FB_HIP(hipMemsetAsync(ps.pipe_mir_stats.p + 2, 0x7f, sizeof(int), s));  // (a minimum)
  hipLaunchKernelGGL(k_pipe_mirror_plan, dim3(nb), dim3(64 * kMirWaves), 0, s, P.n_slices, P.n_owned, h->slice_off.p, h->colidx.p, ps.pipe_wg_first.p, K.klt,
                     h->c16 ? 1 : 0, std::min(ps.pipe_regs, K.regs), ps.pipe_mir.p, ps.pipe_mir_addr.p, ps.pipe_mir_pool.p, ps.pipe_mir_wg.p, ps.pipe_mir_stats.p);
  FB_HIP(hipGetLastError());
  ps.pipe_mir_pending = true;
  return FB_OK;
}

// Where do the columns of a slot lie?  On a structured mesh the 64 rows of a slice have consecutive columns and a gather touches 4 lines
// of each of the three planes of the published vector; on an unstructured one it touches ~50 of each, and a vector stored node by node
// (24-byte records) costs half of those.  Sampled on the device (every 8th slice), decided here: node by node where the planes cost 30 lines
// and more per slot and half again the records' (606k-tet Delaunay probe: 80 against 44 lines, 18.9 -> 16.4 us per iteration; the cube
// after a cut: 19 against 15, and there the planes are the faster form, 19.4 against 20.6, each load touching 4 lines instead of 12).
// FEMBRAIN_PIPE_XYZ=0/1 overrides.  (The table-driven instantiation carries the layout.)
int pipe_layout(fb_fem_s* h, const PersistKnobs& kn, bool* want_xyz) {
  const FemPlan& P = h->plan;
  PersistState& ps = h->ps;
  hipStream_t s = h->stream;
  *want_xyz = false;
  // (a re-sync that changes the mesh by a few per cent keeps the counts of the plan before it: the read-back is a host wait)
  const bool keep_lines = ps.pipe_gather_lines[0] > 0.0 && ps.pipe_lines_nodes > 0 && std::abs(P.n_local - ps.pipe_lines_nodes) * 20 <= ps.pipe_lines_nodes;
  bool measured = keep_lines;
  if (!keep_lines) {
    ps.pipe_gather_lines[0] = ps.pipe_gather_lines[1] = 0.0;
    ps.pipe_lines_nodes = 0;
    if (P.n_local >= (1 << 24) || !h->colidx.p) return FB_OK;
    FB_TRY(ps.pipe_lines.alloc(4));
    FB_HIP(hipMemsetAsync(ps.pipe_lines.p, 0, 4 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_gather_lines, dim3(64), dim3(256), 0, s, P.n_slices, 8, h->slice_off.p, h->colidx.p, ps.pipe_lines.p);
    FB_HIP(hipGetLastError());
    unsigned long long got[3] = {0, 0, 0};
    FB_HIP(hipMemcpyAsync(got, ps.pipe_lines.p, sizeof got, hipMemcpyDeviceToHost, s));
    FB_HIP(hipStreamSynchronize(s));
    measured = got[2] != 0;
    if (measured) { ps.pipe_gather_lines[0] = 3.0 * (double)got[0] / (double)got[2]; ps.pipe_gather_lines[1] = (double)got[1] / (double)got[2]; ps.pipe_lines_nodes = P.n_local; }
  }
  *want_xyz = P.n_local < (1 << 24) &&
              (kn.xyz >= 0 ? kn.xyz != 0 : (measured && ps.pipe_gather_lines[0] >= 30.0 && ps.pipe_gather_lines[0] >= 1.5 * ps.pipe_gather_lines[1]));
  return FB_OK;
}

// Helpers and layout of an unsharded Jacobi plan (one row per lane: both; two rows per lane: the layout): decides pipe_xyz and, where
// helpers, deep LDS shares or the node-by-node vector ask for it, uploads the task table of the (12, 6, HELP) kernel.
int setup_pipe_tasks(fb_fem_s* h, int nb, int w, const PersistKnobs& kn) {
  const FemPlan& P = h->plan;
  PersistState& ps = h->ps;
  int mx = 0;
  long long tot = 0;
  for (int sl = 0; sl < P.n_slices; sl++) { const int wd = P.slice_off[sl + 1] - P.slice_off[sl]; mx = std::max(mx, wd); tot += wd; }
  const double mean = P.n_slices ? (double)tot / P.n_slices : 0.0;
  const bool want_h = ps.pipe_rows == 1 && (kn.helpers >= 0 ? kn.helpers != 0 : (mx > 24 && (double)mx >= 1.5 * mean));
  bool want_xyz = false;
  FB_TRY(pipe_layout(h, kn, &want_xyz));
  ps.pipe_xyz = ps.pipe_rows == 2 && want_xyz;  // (the two-row kernel: a template parameter; the one-row kernel: with its task table, below)
  if (ps.pipe_rows != 1 || !(want_h || want_xyz) || w > kPipeMaxWaves) return FB_OK;
  const PipeTasks T = pipe_help_tasks(P.slice_off.data(), P.n_slices, ps.pipe_wg_first_host.empty() ? nullptr : ps.pipe_wg_first_host.data(), nb, w, h->c16 != 0, want_h,
                                      want_xyz, kn);
  if (!(T.all > 0 || T.deepest > 6 || want_xyz || kn.helpers == 2)) return FB_OK;  // (=2, development: the task table without a single helper)
  FB_TRY(ps.pipe_tasks.upload(T.tasks, h->stream));
  ps.pipe_wmax = 12;
  ps.pipe_slots_dealt = T.deepest;
  ps.pipe_help_waves = T.help_waves; ps.pipe_n_help = T.most; ps.pipe_help_tasks = T.all;
  ps.pipe_xyz = want_xyz;
  if (kn.verbose) fprintf(stderr, "[fembrain] persistent solver: %d helper tasks (at most %d per workgroup), widest slice %d slots, mean %.1f, up to %d slots of a slice in LDS; a slot's gathers touch %.1f lines in planes, %.1f node by node -> %s\n", T.all, T.most, mx, mean, T.deepest, ps.pipe_gather_lines[0], ps.pipe_gather_lines[1], want_xyz ? "node by node" : "planes");
  return FB_OK;
}

// what the launches of an unsharded plan read and write, and the producer lists: the workgroups that own the rows this workgroup's
// columns lie in, exactly (k_slice_producers)
int alloc_persist(fb_fem_s* h, int nb, const PersistKnobs& kn) {
  const FemPlan& P = h->plan;
  PersistState& ps = h->ps;
  hipStream_t s = h->stream;
  ZeroBatch zb(s);  // (the clears of this set-up in one launch)
  FB_TRY(ps.pipe_post.alloc((size_t)2 * nb * 4));
  zb.add(ps.pipe_post);
  ps.pipe_flag_extra = P.n_ranks > 1 ? kP2PMaxRanks : 0;
  FB_TRY(ps.pipe_flags.alloc((size_t)nb + ps.pipe_flag_extra + 16));
  zb.add(ps.pipe_flags);
  const size_t n_pad = (size_t)P.n_slices * 64, nv = (size_t)3 * P.n_local + 2;
  FB_TRY(ps.pipe_planes.alloc(2 * 3 * n_pad));
  zb.add(ps.pipe_planes);
  FB_TRY(ps.pipe_z.alloc(nv));
  FB_TRY(ps.pipe_s.alloc(nv));
  FB_TRY(ps.pipe_state.alloc(2));
  zb.add(ps.pipe_state);
  if (kn.timing) {
    FB_TRY(ps.persist_timing.alloc((size_t)nb * kPipeMaxWaves * kPipeTimingSlots));
    FB_TRY(ps.persist_timing.zero(s));
  } else {
    ps.persist_timing.release();
  }
  static_assert(kPipeMaxBlocks <= 256, "k_slice_producers holds 256 workgroups in its 8 mask words");
  FB_TRY(ps.pipe_owner.alloc((size_t)std::max(1, P.n_slices)));
  FB_TRY(ps.pipe_mask.alloc((size_t)std::max(1, P.n_slices) * 8));
  FB_TRY(ps.pipe_prod.alloc((size_t)nb * kPipeMaxProducers));
  FB_TRY(ps.pipe_prod_count.alloc((size_t)nb));
  FB_TRY(ps.pipe_prod_xcd.alloc((size_t)nb));
  FB_TRY(ps.pipe_stats.alloc(2));
  zb.add(ps.pipe_stats);
  FB_TRY(zb.flush());
  hipLaunchKernelGGL(k_slice_owner, dim3(ceil_div(nb, kBlock)), dim3(kBlock), 0, s, P.n_slices, nb, ps.pipe_wg_first.p, ps.pipe_owner.p);
  hipLaunchKernelGGL(k_slice_producers, dim3(ceil_div(std::max(1, P.n_slices), kWavesPerBlock)), dim3(kBlock), 0, s, P.n_slices, P.n_owned, h->slice_off.p, h->colidx.p,
                     ps.pipe_owner.p, ps.pipe_mask.p);
  hipLaunchKernelGGL(k_wg_producers, dim3(ceil_div(nb, kBlock)), dim3(kBlock), 0, s, P.n_slices, nb, ps.pipe_wg_first.p, ps.pipe_mask.p, kn.poll_all ? 1 : 0, ps.pipe_prod.p, ps.pipe_prod_count.p,
                     ps.pipe_prod_xcd.p, ps.pipe_stats.p);
  FB_HIP(hipGetLastError());
  ps.pipe_stats_pending = true;  // (the longest list is fetched when fb_fem_pcg_path asks)
  ps.pipe_max_producers = 0;
  FB_TRY(ps.pipe_xcc.alloc((size_t)nb));
  zb.add(ps.pipe_xcc);
  return zb.flush();
}

}  // namespace

// FB_MATRIX_AUTO: fp32 values from 2 slices per CU on (setup_persist's `w`, the persistent solver's range) and where the persistent solver is
// asked for by name; fp64 below (include/fembrain_hip.h).  A shard decides by the WHOLE mesh, so that the sharded and the unsharded handle
// of one mesh store the same values; the sharded persistent solver, asked for through the environment, needs fp32 as the unsharded one does.
bool auto_matrix_f64(const fb_fem_s* h, int n_nodes, int n_ranks) {
  const int cus = h->cu_limit > 0 ? std::min(h->cu_limit, h->n_cu_device) : h->n_cu_device;
  const int nb = std::min(kPipeMaxBlocks, (cus / 8) * 8);
  const int w = nb >= 8 ? ceil_div(ceil_div(ceil_div(n_nodes, 64), 8), nb / 8) : 0;
  const bool shard_persist_asked = n_ranks > 1 && read_persist_knobs().sharded;
  return h->prm.pcg_variant != FB_PCG_PERSISTENT && !shard_persist_asked && w < 2;
}

void release_shard_persist(fb_fem_s* h) {
  for (auto& o : h->ps.sbox_opened) { if (o) (void)hipIpcCloseMemHandle(o); o = nullptr; }
  if (h->ps.sbox) (void)hipFree(h->ps.sbox);
  h->ps.sbox = nullptr;
  h->ps.shard_persist = false;
}

// how long a wait inside a persistent launch may last before the launch gives up (read when a plan is built and when the solver is re-armed)
void read_persist_timeout(fb_fem_s* h) {
  const char* t = getenv("FEMBRAIN_PERSIST_TIMEOUT_MS");
  // default 50 ms: a whole 1M-tet solve is ~25 ms, one wait is microseconds.  A sharded handle also waits for the OTHER RANKS' launches
  // to begin, and those are separated by host jitter (first launch: code object load): 2 s there
  const double ms = t ? atof(t) : (h->plan.n_ranks > 1 ? 2000.0 : 50.0);
  h->ps.persist_timeout_ticks = std::max(1LL, (long long)(ms * 1e5));  // 100 MHz
}

// Decides whether this handle solves inside persistent launches and allocates what they need (called for every (re)built plan):
// eligibility, the deal, the kernel form, tasks and layout, allocation and producer lists, the instantiation, the LDS window.
int setup_persist(fb_fem_s* h) {
  const FemPlan& P = h->plan;
  PersistState& ps = h->ps;
  const PersistKnobs kn = read_persist_knobs();
  if (ps.pipe_mir_knob < 0) ps.pipe_mir_knob = kn.mirror ? 1 : 0;  // (the handle's first plan: its re-syncs keep what it was made with)
  ps.pipe_timing_level = kn.timing;
  ps.reset_plan(kn.rearm);
  hipDeviceProp_t prop;
  FB_HIP(hipGetDeviceProperties(&prop, h->prm.device));
  const int nb = std::min(kPipeMaxBlocks, ((h->cu_limit > 0 ? std::min(h->cu_limit, prop.multiProcessorCount) : prop.multiProcessorCount) / 8) * 8);
  int w = nb >= 8 ? ceil_div(ceil_div(P.n_slices, 8), nb / 8) : 0;
  if (P.n_ranks == 1 && !P.slice_off.empty()) {
    w = pipe_deal_by_slots(P.slice_off.data(), P.n_slices, nb, w, kn, &ps.pipe_wg_first_host);
    if (!ps.pipe_wg_first_host.empty()) FB_TRY(ps.pipe_wg_first.upload(ps.pipe_wg_first_host, h->stream));
  }
  read_persist_timeout(h);
  const bool explicit_p = h->prm.pcg_variant == FB_PCG_PERSISTENT;
  const bool shard_opt = P.n_ranks > 1 && kn.sharded;
  if (explicit_p && P.n_ranks > 1 && !shard_opt) return fail(FB_EINVAL, "FB_PCG_PERSISTENT on a sharded handle needs FEMBRAIN_SHARDED_PERSIST=1 (unmeasured on multi-GPU hardware)");
  if (explicit_p && h->f64) return fail(FB_EINVAL, "FB_PCG_PERSISTENT needs FB_MATRIX_F32 storage (part of the matrix is kept in LDS as fp32 words)");
  if (explicit_p && (nb < 8 || w < 1 || w > 2 * kPipeMaxWaves))
    return fail(FB_EINVAL, "FB_PCG_PERSISTENT needs at most %d slices per CU, this mesh has %d on %d CUs", 2 * kPipeMaxWaves, w, nb);
  // asked for explicitly (parameter or FEMBRAIN_PCG_PERSIST=1), or by default where it was measured faster than the
  // two-launch iteration: fp32 storage, up to 12 slices per CU
  // (a sharded handle: opt-in, one row per lane, and a spare wavefront per workgroup for the proxies and the sums)
  const bool eligible = !h->f64 && nb >= 8 && w >= 1 && (P.n_ranks == 1 ? w <= 2 * kPipeMaxWaves : (shard_opt && w <= 2 * (kPipeMaxWaves - 1)));  // (sharded: the spare wavefront leaves 11 for slices, two rows per lane from 12 slices on)
  // FB_PCG_BLOCK_JACOBI (opt-in, outside parity): the one-row persistent kernel with the block preconditioner, same rule
  const bool bj = h->prm.pcg_variant == FB_PCG_BLOCK_JACOBI;
  const bool by_default = (h->prm.pcg_variant == FB_PCG_MERGED || bj) && w >= kn.min_waves;
  const bool want_p = kn.pcg_persist >= 0 ? kn.pcg_persist != 0 && (h->prm.pcg_variant == FB_PCG_MERGED || explicit_p || bj) : (explicit_p || by_default);
  if (!want_p || !eligible) return FB_OK;
  if (bj && (w > kPipeMaxWaves || kn.rows2 || P.n_ranks > 1)) return FB_OK;  // (no two-row form with the block preconditioner)
  if (P.n_ranks > 1) return setup_persist_shard_local(h, nb, w, kn);
  ps.persist = true; ps.persist_blocks = nb; ps.persist_waves = w;
  // up to 12 slices per CU: one row per lane (k_pcg_pipe); 13..24: two (k_pcg_pipe2, no LDS-resident slots)
  ps.pipe_rows = w > kPipeMaxWaves || kn.rows2 ? 2 : 1;
  const bool small = ps.pipe_rows == 1 && w <= 4 && !bj && kn.small;
  ps.pipe_wmax = ps.pipe_rows == 2 ? 12 : (small ? 5 : (w <= 8 ? 8 : 12));
  // slots of every slice resident in LDS at least: the CU's 62 / 65 (16-bit columns) wavefront-slots dealt to the slices of a workgroup (k_pcg_pipe), at most 16 / 8 / 6
  ps.pipe_slots_dealt = ps.pipe_rows == 2 ? std::min(kPipe2Klt, pipe2_lds_slots(w, h->c16 != 0) / std::max(w, 1))
                                          : std::min(small ? 16 : (w <= 8 ? 8 : 6), pipe_lds_slots(h->c16 != 0) / std::max(w, 1));
  ps.pipe_tasks.release();
  ps.pipe_help_waves = 0; ps.pipe_n_help = 0; ps.pipe_help_tasks = 0;
  ps.pipe_xyz = false;
  if (!bj && !small && !P.slice_off.empty()) FB_TRY(setup_pipe_tasks(h, nb, w, kn));
  FB_TRY(alloc_persist(h, nb, kn));
  ps.pipe_plain_local = kn.plain_stores >= 0 ? kn.plain_stores : (w <= 8 ? 1 : 0);
  FB_TRY(resolve_pipe_kernel(h, kn));
  return setup_pipe_mirror(h);
}

// The collective half: every rank allocates its box, the ranks exchange the IPC handles, the halo sizes and how many of their
// workgroups send to whom, map each other's boxes, and agree that all of it worked -- otherwise every rank alike runs the
// two-launch iteration.
int attach_pipe_shard(fb_fem_s* h) {
  const FemPlan& P = h->plan;
  PersistState& ps = h->ps;
  const int R = P.n_ranks, me = P.rank;
  if (R < 2 || !h->comm) return FB_OK;
  const PersistKnobs kn = read_persist_knobs();
  if (!kn.sharded) return FB_OK;  // (the same on every rank)
  {  // a re-sync: the previous box and mappings go first
    const bool keep = ps.shard_persist;
    release_shard_persist(h);
    ps.shard_persist = keep;
  }
  struct Meta { hipIpcMemHandle_t handle; long long n_halo; int halo_off[kP2PMaxRanks + 1]; int senders_to[kP2PMaxRanks]; int ok; };
  Meta mine;
  memset(&mine, 0, sizeof mine);
  bool ok = ps.shard_persist && R <= kP2PMaxRanks;
  // the box is sized by the largest halo of all ranks, so a first round agrees on that
  long long nh = ok ? P.n_local - P.n_owned : -1;
  std::vector<long long> nhs((size_t)R);
  FB_TRY(comm_allgather_bytes(h->comm, &nh, nhs.data(), sizeof nh, h->stream));
  long long cap = 1;
  for (int q = 0; q < R; q++) { if (nhs[q] < 0) ok = false; cap = std::max(cap, nhs[q]); }
  const ShardBoxLayout BL = shard_box_layout(cap);
  if (ok) {
    ok = hipExtMallocWithFlags((void**)&ps.sbox, BL.bytes, hipDeviceMallocFinegrained) == hipSuccess;
    ok = ok && hipMemsetAsync(ps.sbox, 0, BL.bytes, h->stream) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess;
    ok = ok && hipIpcGetMemHandle(&mine.handle, ps.sbox) == hipSuccess;
    (void)hipGetLastError();
    mine.n_halo = P.n_local - P.n_owned;
    for (int q = 0; q <= R; q++) mine.halo_off[q] = P.halo_off[q];
    std::vector<unsigned int> wg_mask((size_t)ps.persist_blocks);
    ok = ok && ps.sh_wg_send_mask.download(wg_mask.data(), wg_mask.size(), h->stream) == FB_OK;
    for (unsigned int m : wg_mask)
      for (int q = 0; q < R; q++) mine.senders_to[q] += (m >> q) & 1u;
  }
  mine.ok = ok ? 1 : 0;
  std::vector<Meta> all((size_t)R);
  FB_TRY(comm_allgather_bytes(h->comm, &mine, all.data(), sizeof(Meta), h->stream));
  bool all_ok = true;
  for (int q = 0; q < R; q++) all_ok = all_ok && all[q].ok;
  int opened_ok = 1;
  std::vector<char*> peers((size_t)R, nullptr);
  std::vector<int> seg((size_t)R, 0), senders((size_t)R, 0);
  if (all_ok) {
    for (int q = 0; q < R; q++) {
      seg[q] = all[q].halo_off[me];
      senders[q] = all[q].senders_to[me];
      if (q == me) { peers[q] = ps.sbox; continue; }
      void* ptr = nullptr;
      if (hipIpcOpenMemHandle(&ptr, all[q].handle, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); opened_ok = 0; break; }
      ps.sbox_opened[q] = ptr;
      peers[q] = (char*)ptr;
    }
  }
  std::vector<int> oks((size_t)R);
  FB_TRY(comm_allgather_bytes(h->comm, &opened_ok, oks.data(), sizeof(int), h->stream));
  for (int q = 0; q < R; q++) all_ok = all_ok && oks[q];
  if (!all_ok) { release_shard_persist(h); ps.persist = false; return FB_OK; }
  ps.sbox_halo_cap = cap;
  FB_TRY(ps.sbox_peers.upload(peers.data(), peers.size(), h->stream));
  FB_TRY(ps.sh_peer_seg.upload(seg, h->stream));
  FB_TRY(ps.sh_n_senders.upload(senders, h->stream));
  ps.persist = true;
  if (kn.verbose) fprintf(stderr, "[fembrain] rank %d: sharded persistent solver attached (%d workgroups, up to %d slices per CU, %d fewer where halo rows are gathered, %d proxies per source rank, halo %lld of cap %lld)\n", me, ps.persist_blocks, ps.persist_waves, ps.sh_relief, ps.sh_n_proxy, (long long)(P.n_local - P.n_owned), cap);
  return FB_OK;
}

// One launch of the pipelined persistent solver (pcg_pipe.hip.h): `start` 1 = new solve from x = 0, 2 = new solve from the x in
// memory, 0 = continue; at most n_iters iterations
int launch_pipe(fb_fem_s* h, const double* b, int start, int n_iters, double eps, int max_iter) {
  PersistState& ps = h->ps;
  if (!ps.kernel) return fail(FB_EINVAL, "internal: persistent launch on a handle whose plan resolved no kernel");
  const PipeKernel& K = *ps.kernel;
  PipeArgs pa;
  pa.post = ps.pipe_post.p; pa.flags = ps.pipe_flags.p; pa.error = ps.pipe_flags.p + ps.persist_blocks + ps.pipe_flag_extra + 4; pa.seqs = ps.pipe_flags.p + ps.persist_blocks + ps.pipe_flag_extra + 8;
  pa.producers = ps.pipe_prod.p; pa.prod_count = ps.pipe_prod_count.p; pa.prod_xcd = ps.pipe_prod_xcd.p; pa.plain_local = ps.pipe_plain_local; pa.xcc = ps.pipe_xcc.p;
  pa.start = start; pa.n_iters = n_iters; pa.eps2 = eps * eps; pa.max_iter = max_iter;
  pa.timeout_ticks = ps.persist_timeout_ticks;
  pa.timing = ps.persist_timing.p;
  pa.planes = ps.pipe_planes.p; pa.n_pad = ps.shard_persist ? (size_t)ceil_div(h->plan.n_local, 64) * 64 : (size_t)h->plan.n_slices * 64;
  pa.pstate = ps.pipe_state.p;
  pa.tasks = ps.pipe_tasks.p; pa.n_help = ps.pipe_n_help;
  pa.wg_first = ps.pipe_wg_first.p;
  // the LDS window (setup_pipe_mirror planned it for this row's unroll bound, or not at all)
  pa.mirror = ps.pipe_mir.p; pa.mir_addr = ps.pipe_mir_addr.p; pa.mir_wg = ps.pipe_mir_wg.p; pa.mir_pool = ps.pipe_mir_pool.p;
  // one wavefront more than slices where the instantiation has room: it collects the sums while the others multiply
  const int cwaves = K.rows == 2 ? ceil_div(ps.persist_waves, 2) : ps.persist_waves;  // wavefronts that own slices
  pa.service = pipe_has_service(ps) ? 1 : 0;
  if (K.ahead != (K.rows == 1 && !K.shard && !K.help && pa.service != 0)) return fail(FB_EINVAL, "internal: the resolved kernel's launch form is not this launch's");
  // values of the first streamed slots pulled into L2 during the neighbour wait: pays where the product is bandwidth-bound (9 and more
  // slices per CU: -6 % per iteration at 1M tets; neutral at 1,000 slices)
  pa.prefetch_slots = ps.persist_waves >= 9 ? (K.rows == 2 ? 3 : 4) : 0;
  ShardArgs sa;
  memset(&sa, 0, sizeof sa);
  if (ps.shard_persist) {
    sa.rank = h->plan.rank; sa.n_ranks = h->plan.n_ranks; sa.n_owned = h->plan.n_owned; sa.n_halo = h->plan.n_local - h->plan.n_owned;
    sa.box = ps.sbox; sa.peer_box = ps.sbox_peers.p; sa.peer_seg = ps.sh_peer_seg.p; sa.halo_cap = ps.sbox_halo_cap;
    sa.halo_off = ps.sh_halo_off.p; sa.row_send_off = ps.sh_row_send_off.p; sa.row_send_rank = ps.sh_row_send_rank.p; sa.row_send_pos = ps.sh_row_send_pos.p;
    sa.wg_send_mask = ps.sh_wg_send_mask.p; sa.n_senders = ps.sh_n_senders.p; sa.proxy_wg = ps.sh_proxy_wg.p; sa.n_proxy = ps.sh_n_proxy; sa.wg_duty = ps.sh_wg_duty.p; sa.wg_range = ps.sh_wg_range.p;
    sa.delay_ticks = remote_delay_ticks();
  }
  // every instantiation takes the same arguments; the block-Jacobi ones read 9 doubles per row where the others read 1 / diag
  SellView sv = sell_view(h);
  const float *vals = (const float*)h->vals.p, *dlo = (const float*)h->dlo.p;
  const double* inv = K.bj ? h->invblk.p : h->invdiag.p;
  void* args[] = {&sv, &vals, &dlo, &inv, &b, &h->x.p, &h->r.p, &h->Ad.p, &ps.pipe_z.p, &ps.pipe_s.p, &h->d.p, &h->st.p, &pa, &sa};
  // LDS: the sync buffers, then KLT slots of every slice; the request is the whole 160 KB of a CU, so exactly one workgroup lands on each
  const size_t lds = 160 * 1024;
  const dim3 grid(ps.persist_blocks), block(64 * (cwaves + ps.pipe_help_waves + pa.service));  // slices | helpers | the service wavefront
  FB_HIP(hipEventRecord(h->ev_p[0], h->stream));
  // (the attribute is per device and cheap to set: set at every launch)
  FB_HIP(hipFuncSetAttribute(K.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  FB_HIP(hipLaunchKernel(K.fn, grid, block, args, lds, h->stream));
  FB_HIP(hipEventRecord(h->ev_p[1], h->stream));
  return FB_OK;
}

void print_pipe_timing(fb_fem_s* h) {
  std::vector<long long> tm((size_t)h->ps.persist_blocks * kPipeMaxWaves * kPipeTimingSlots);
  if (h->ps.persist_timing.download(tm.data(), tm.size(), h->stream) != FB_OK) return;
  (void)h->ps.persist_timing.zero(h->stream);
  const bool ahead = h->ps.kernel && h->ps.kernel->ahead;  // (run-ahead form: a wavefront's own wait for the totals stands where the sweep's barrier stood)
  const char* names[5] = {"publish (drained)", "flag+wait+acquire", "product", ahead ? "wait for the totals" : "sums sweep", "recurrences(+refresh)"};
  for (int k = 0; k < 5; k++) {
    double mn = 1e30, mx = 0, av = 0;
    int cnt = 0;
    for (int b = 0; b < h->ps.persist_blocks; b++)
      for (int w = 0; w < h->ps.persist_waves; w++) {
        const long long* t = &tm[((size_t)b * kPipeMaxWaves + w) * kPipeTimingSlots];
        if (t[5] <= 0) continue;
        const double us = (double)t[k] / (double)t[5] * 0.01;
        mn = std::min(mn, us); mx = std::max(mx, us); av += us; cnt++;
      }
    fprintf(stderr, "[fembrain] pipelined PCG %-22s per iteration: avg %.2f us  min %.2f  max %.2f (over %d waves)\n", names[k], av / std::max(cnt, 1), mn, mx, cnt);
  }
  if (h->ps.kernel && h->ps.kernel->wmax == 12 && !h->ps.kernel->help) {
    // the product phase of the LDS window's kernels in its three parts (words 6, 7 and the rest of word 2), over all wavefronts and over
    // the slowest wavefront of every workgroup -- the one its barrier waits for
    const char* parts[3] = {"product: streamed [0,a)", "product: on-chip run", "product: streamed rest"};
    for (int k = 0; k < 3; k++) {
      double av = 0, mx = 0, sav = 0;
      int cnt = 0, wgs = 0;
      for (int b = 0; b < h->ps.persist_blocks; b++) {
        double slowest = -1, part = 0;
        for (int w = 0; w < h->ps.persist_waves; w++) {
          const long long* t = &tm[((size_t)b * kPipeMaxWaves + w) * kPipeTimingSlots];
          if (t[5] <= 0) continue;
          const double us = (double)(k == 0 ? t[6] : (k == 1 ? t[7] : t[2] - t[6] - t[7])) / (double)t[5] * 0.01;
          av += us; mx = std::max(mx, us); cnt++;
          if ((double)t[2] > slowest) { slowest = (double)t[2]; part = us; }
        }
        if (slowest >= 0) { sav += part; wgs++; }
      }
      fprintf(stderr, "[fembrain] pipelined PCG %-24s per iteration: avg %.2f us  max %.2f; in the slowest wavefront of a workgroup: avg %.2f\n", parts[k], av / std::max(cnt, 1), mx,
              sav / std::max(wgs, 1));
    }
  }
  if (h->ps.pipe_timing_level >= 2) {
    // where the slow products are: by wavefront index, by XCD (workgroup & 7), and the slowest workgroups
    for (int k = 1; k <= 2; k++) {
      fprintf(stderr, "[fembrain] %s by wavefront:", names[k]);
      for (int w = 0; w < h->ps.persist_waves; w++) {
        double av = 0; int cnt = 0;
        for (int b = 0; b < h->ps.persist_blocks; b++) { const long long* t = &tm[((size_t)b * kPipeMaxWaves + w) * kPipeTimingSlots]; if (t[5] > 0) { av += (double)t[k] / (double)t[5] * 0.01; cnt++; } }
        fprintf(stderr, " %.2f", av / std::max(cnt, 1));
      }
      fprintf(stderr, "\n[fembrain] %s by XCD (avg / max over its workgroups' slowest wavefront):", names[k]);
      for (int x = 0; x < 8; x++) {
        double av = 0, mx = 0; int cnt = 0;
        for (int b = x; b < h->ps.persist_blocks; b += 8) {
          double wmx = 0;
          for (int w = 0; w < h->ps.persist_waves; w++) { const long long* t = &tm[((size_t)b * kPipeMaxWaves + w) * kPipeTimingSlots]; if (t[5] > 0) wmx = std::max(wmx, (double)t[k] / (double)t[5] * 0.01); }
          av += wmx; mx = std::max(mx, wmx); cnt++;
        }
        fprintf(stderr, " %.2f/%.2f", av / std::max(cnt, 1), mx);
      }
      fprintf(stderr, "\n");
    }
    std::vector<std::pair<double, int>> slow;
    for (int b = 0; b < h->ps.persist_blocks; b++) {
      double wmx = 0;
      for (int w = 0; w < h->ps.persist_waves; w++) { const long long* t = &tm[((size_t)b * kPipeMaxWaves + w) * kPipeTimingSlots]; if (t[5] > 0) wmx = std::max(wmx, (double)t[2] / (double)t[5] * 0.01); }
      slow.push_back({wmx, b});
    }
    std::sort(slow.begin(), slow.end());
    fprintf(stderr, "[fembrain] slowest product of a workgroup: median %.2f us, fastest", slow[slow.size() / 2].first);
    for (int k = 0; k < 6 && k < (int)slow.size(); k++) fprintf(stderr, " wg%d %.2f", slow[k].second, slow[k].first);
    fprintf(stderr, "; slowest");
    for (int k = 0; k < 12 && k < (int)slow.size(); k++) fprintf(stderr, " wg%d %.2f", slow[slow.size() - 1 - k].second, slow[slow.size() - 1 - k].first);
    fprintf(stderr, "\n");
  }
}

// What the live plan decided, for fb_fem_device_plan_get (read-only): "pipe_tasks" the int4 rows of the task table ([workgroup][kPipeTaskStride],
// pcg_pipe_plan.h), "pipe_windows" per slice (first slot a, mirror layers m, plain resident slots p) of the LDS window (pcg_pipe_mirror.h),
// "pipe_wg_first" the deal by slots (pipe_deal's table).  1: filled, 0: no such name or this plan has none, < 0: an error.
int persist_plan_array(fb_fem_s* h, const char* name, std::vector<int>* out) {
  PersistState& ps = h->ps;
  const std::string n(name);
  out->clear();
  if (!ps.persist) return 0;
  if (n == "pipe_tasks" && ps.pipe_tasks.p) {
    out->resize((size_t)4 * ps.persist_blocks * kPipeTaskStride);
    FB_TRY(ps.pipe_tasks.download((int4*)out->data(), (size_t)ps.persist_blocks * kPipeTaskStride, h->stream));
    return 1;
  }
  if (n == "pipe_wg_first" && !ps.pipe_wg_first_host.empty()) { *out = ps.pipe_wg_first_host; return 1; }
  if (n == "pipe_windows" && ps.pipe_mir.p) {
    const int nb = ps.persist_blocks, ns = h->plan.n_slices;
    std::vector<int4> mt((size_t)nb * kPipeMaxWaves);
    FB_TRY(ps.pipe_mir.download(mt.data(), mt.size(), h->stream));
    out->assign((size_t)3 * ns, 0);
    for (int b = 0; b < nb; b++) {
      int first, count;
      pipe_deal(ps.pipe_wg_first_host.empty() ? nullptr : ps.pipe_wg_first_host.data(), ns, nb, b, &first, &count);
      for (int w = 0; w < count && w < kPipeMaxWaves && first + w < ns; w++) {
        const int x = mt[(size_t)b * kPipeMaxWaves + w].x;
        int* o = &(*out)[(size_t)3 * (first + w)];
        o[0] = x & 0xff; o[1] = (x >> 8) & 0xff; o[2] = (x >> 16) & 0xff;
      }
    }
    return 1;
  }
  return 0;
}

}  // namespace fb

extern "C" {

int fb_fem_sharded_persist(fb_fem_t h) {
  if (!h) return 0;
  return h->ps.shard_persist && h->ps.persist ? 1 : 0;
}

int fb_fem_set_sharded_persist(fb_fem_t h, int on) {
  CHECK_HANDLE(h);
  if (!h->ps.shard_persist || !h->ps.sbox) return fail(FB_EINVAL, "the sharded persistent solver is not attached to this handle (FEMBRAIN_SHARDED_PERSIST=1 at creation, <= %d slices per CU)", 2 * (kPipeMaxWaves - 1));
  if (on && h->ps.persist_broken) return fail(FB_EDEVICE, "the sharded persistent solver of this handle timed out before; it stays with the two-launch iteration");
  FB_HIP(hipStreamSynchronize(h->stream));
  h->ps.persist = on != 0;
  return FB_OK;
}

int fb_fem_persist_info(fb_fem_t h, int* waves_per_cu, int* workgroups, int* lds_slots) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  if (waves_per_cu) *waves_per_cu = h->ps.persist ? h->ps.persist_waves : 0;
  if (workgroups) *workgroups = h->ps.persist ? h->ps.persist_blocks : 0;
  if (lds_slots) {
    *lds_slots = 0;
    if (h->ps.persist) *lds_slots = h->ps.pipe_slots_dealt;
  }
  return h->ps.persist ? 1 : 0;
}

int fb_fem_pcg_path(fb_fem_t h, char* name, int name_len, int* persist_launches, int* persist_fallbacks, int* max_producers) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  if (name && name_len > 0) {
    const PipeKernel* K = h->ps.persist ? h->ps.kernel : nullptr;
    if (!K) name[0] = 0;
    else if (K->shard && K->rows == 2) snprintf(name, name_len, "k_pcg_pipe2_shard");
    else if (K->shard) snprintf(name, name_len, "k_pcg_pipe_shard<%d,%d>", K->wmax, K->klt);
    else if (K->rows == 2) snprintf(name, name_len, "k_pcg_pipe2<%s>", K->c16 ? "c16" : "c32");
    else snprintf(name, name_len, "k_pcg_pipe<float,%s,%d,%d%s>", K->c16 ? "c16" : "c32", K->wmax, K->klt, K->bj ? ",bj" : "");
  }
  if (persist_launches) *persist_launches = h->ps.persist_launches;
  if (persist_fallbacks) *persist_fallbacks = h->ps.persist_fallbacks;
  if (max_producers && h->ps.persist && h->ps.pipe_stats_pending) {
    int st[2] = {0, 0};
    FB_TRY(h->ps.pipe_stats.download(st, 2, h->stream));
    h->ps.pipe_max_producers = st[1] ? -1 : st[0];
    h->ps.pipe_stats_pending = false;
  }
  if (max_producers) *max_producers = h->ps.persist ? h->ps.pipe_max_producers : 0;
  return h->last_pcg_path;
}

int fb_fem_persist_rearms(fb_fem_t h) { return h ? h->ps.persist_rearms : 0; }
int fb_fem_persist_helpers(fb_fem_t h) { return h && h->ps.persist ? h->ps.pipe_help_tasks : 0; }
int fb_fem_persist_mirror(fb_fem_t h, int* mirror_layers, int* pool_entries, int* plain_slots) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  if (h->ps.pipe_mir_pending) {
    FB_TRY(h->ps.pipe_mir_stats.download(h->ps.pipe_mir_got, 4, h->stream));
    h->ps.pipe_mir_pending = false;
  }
  const bool on = h->ps.persist && h->ps.pipe_mir.p;
  if (mirror_layers) *mirror_layers = on ? h->ps.pipe_mir_got[0] : 0;
  if (pool_entries) *pool_entries = on ? h->ps.pipe_mir_got[1] : 0;
  if (plain_slots) *plain_slots = on ? h->ps.pipe_mir_got[2] : 0;
  return on && h->ps.pipe_mir_got[0] > 0 ? 1 : 0;
}

int fb_fem_persist_regs(fb_fem_t h, int* slots_per_slice) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  const bool on = h->ps.persist && h->ps.pipe_mir.p && h->ps.kernel && h->ps.kernel->regs > 0;
  if (on && h->ps.pipe_mir_pending) {
    FB_TRY(h->ps.pipe_mir_stats.download(h->ps.pipe_mir_got, 4, h->stream));
    h->ps.pipe_mir_pending = false;
  }
  if (slots_per_slice) *slots_per_slice = on ? std::min(h->ps.pipe_regs, h->ps.kernel->regs) : 0;
  return on ? h->ps.pipe_mir_got[3] : 0;
}

int fb_fem_persist_prio(fb_fem_t h) { return h && h->ps.persist && h->ps.kernel ? h->ps.kernel->prio : 0; }

int fb_fem_persist_gather(fb_fem_t h, double* lines_planes, double* lines_records) {
  if (lines_planes) *lines_planes = h && h->ps.persist ? h->ps.pipe_gather_lines[0] : 0.0;
  if (lines_records) *lines_records = h && h->ps.persist ? h->ps.pipe_gather_lines[1] : 0.0;
  return h && h->ps.persist && h->ps.pipe_xyz ? 1 : 0;
}

int fb_fem_persist_stats(fb_fem_t h, int* launches, double* seconds, long long* iterations) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  if (launches) *launches = h->ps.persist_launches;
  if (seconds) *seconds = h->ps.persist_seconds;
  if (iterations) *iterations = h->ps.persist_iterations;
  return FB_OK;
}

int fb_fem_time_persist(fb_fem_t h, int reps, int n_iters, double* seconds_per_launch) {
  CHECK_HANDLE(h);
  if (reps < 1 || n_iters < 1 || n_iters > 100000 || !seconds_per_launch) return fail(FB_EINVAL, "bad arguments");
  if (!h->ps.persist) return fail(FB_EINVAL, "this handle does not run the persistent PCG iterations");
  if (!h->system_valid) FB_TRY(assemble_system(h));
  double total = 0.0;
  for (int r = -1; r < reps; r++) {  // r = -1: warm-up
    double t = 0.0;
    // a solve of the current right-hand side with a tolerance it cannot reach, cut after n_iters iterations; each launch is timed and waited for
    FB_TRY(timed_reps(h, 1, [&] { return launch_pipe(h, h->rhs.p, 1, n_iters, 1e-30, 1 << 30); }, &t));
    if (r >= 0) total += t;
  }
  unsigned int err = 0;
  FB_HIP(hipMemcpy(&err, h->ps.pipe_flags.p + h->ps.persist_blocks + h->ps.pipe_flag_extra + 4, sizeof err, hipMemcpyDeviceToHost));
  if (err) {
    FB_TRY(h->ps.pipe_flags.zero(h->stream));
    FB_TRY(h->ps.pipe_post.zero(h->stream));
    if (h->ps.shard_persist) {
      // the peers' cumulative box counters are ahead of the flags just cleared: this handle must not launch the sharded kernel again
      // (ADVICE r3); its solves run the two-launch iteration until a re-sync attaches fresh boxes
      h->ps.persist = false;
      h->ps.persist_broken = true;
    }
    return fail(FB_EDEVICE, "persistent PCG: a wait inside the launch timed out");
  }
  h->system_valid = false;
  *seconds_per_launch = total / reps;
  return FB_OK;
}

}  // extern "C"
