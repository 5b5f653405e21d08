// Host side of the persistent solver's plan (fem_persist.hip): its environment knobs and the host arithmetic that deals slices, LDS
// slots, helper tasks and -- on a shard -- send lists, proxies and producer lists.  No handle and no HIP call in here: functions of the
// plan's arrays.  Uses the constants and the two deal functions of the kernel headers, so it is included by fem_persist.hip only.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "fem_plan.h"
#include "pcg_pipe2.hip.h"

namespace fb {

// The persistent solver's environment knobs.  read_persist_knobs() (fem_persist.hip) is the one place that reads them, once per plan
// build (handle creation and every re-sync) unless a field says otherwise.  -1 = not set: the rule next to the field decides.
// Read elsewhere, at another moment: FEMBRAIN_PERSIST_TIMEOUT_MS (read_persist_timeout: per plan build and per re-arm) and
// FEMBRAIN_PERSIST_MAX_RUN / _STRICT / _CAP_CHECK (fem.hip pcg_solve_pipe: per solve, on a live handle).
constexpr int kPipePrioDefault = 1;  // FEMBRAIN_PIPE_PRIO not set (PersistKnobs::prio)
struct PersistKnobs {
  // FEMBRAIN_PCG_PERSIST=0/1: off / on for FB_PCG_MERGED, FB_PCG_PERSISTENT and FB_PCG_BLOCK_JACOBI handles.  Not set: asked for
  // explicitly (FB_PCG_PERSISTENT), or by default where it was measured faster than the two-launch iteration (min_waves)
  int pcg_persist = -1;
  // FEMBRAIN_PERSIST_MIN_WAVES: slices per CU from which the persistent solver is the default (us per iteration, two-launch vs persistent,
  // on MI355X: 7.83 / 7.87 at 125 slices = 1 per CU, 8.74 / 8.74 at 308 and 8.98 / 8.64 at 466 = 2 per CU, 10.9 / 8.8 at 614 = 3 per CU,
  // 14.0 / 10.3 at 792, 15.8 / 8.9 at 1,000, 27.4 / 15.75 at 2,744 = 1M tets)
  int min_waves = 2;
  // FEMBRAIN_PERSIST_ROWS=2 forces the two-row kernel on a smaller system (tests)
  bool rows2 = false;
  // FEMBRAIN_PERSIST_REARM=n: clean two-launch solves after which a handle that fell back tries the persistent launch again (0 = never)
  int rearm = 32;
  // FEMBRAIN_PERSIST_TIMING (development aid): set = the instantiation with the phase clocks, printed after every solve; >= 2 = also by
  // wavefront, by XCD and the slowest workgroups
  int timing = 0;
  // FEMBRAIN_PERSIST_POLL_ALL=1 (development aid): every workgroup polls all others instead of its producer list
  bool poll_all = false;
  // FEMBRAIN_SHARDED_PERSIST=1: the sharded persistent solver (opt-in, unmeasured on multi-GPU hardware); the same on every rank
  bool sharded = false;
  // FEMBRAIN_SHARD_RELIEF=n: slices fewer that a workgroup whose slices gather halo rows is dealt.  Not set (profiles/r04_remote_delay.json:
  // two and four ranks on CU shares of one GPU, remote signals delayed by 0 / 1 / 2 / 5 us): relief pays where FEW workgroups gather halo
  // rows -- 1M tets on two ranks, 2 of 28 planes per rank: 18.5 against 20.6 us per iteration, and still 21.4 against 22.8 with 2 us added
  // per hop -- and costs where many do: on four ranks (14 planes per rank, the geometry of the 8M-tet mesh on eight GPUs) the even deal
  // runs 20.4 against 23.5.  So: 35 % of the slices per CU while at most a twelfth of the slices gather halo rows, none beyond.
  int shard_relief = -1;
  // FEMBRAIN_PIPE_BALANCE=0/1: the slices dealt to the workgroups by slots instead of in equal numbers.  Not set: pipe_deal_by_slots' rule
  int balance = -1;
  // FEMBRAIN_PIPE_SMALL=1: up to 4 slices per CU (BASELINE config 2: 105k tets = 2 per CU) k_pcg_pipe<..,5,16> keeps the WHOLE slice in LDS
  // -- 16 slots each where (8, 8) keeps 8 of ~15 and streams the rest from L2 in every product.  Built, tested, measured
  // -- and NOT the default: 9.24 / 9.50 / 9.63 us per iteration at 27^3 / 33^3 / 37^3 against 8.82 / 9.06 / 9.58 with (8, 8).  The phase
  // table says why (profiles/r05_small_mesh_phase_table.txt): the product is 2.2 of the 8.9 us, the other 6.6 are the hand-offs between the
  // CUs (drain of the publish stores 1.0, flag + neighbour wait + acquire 3.2, sweep of the sums 2.0, recurrences 0.5), which no residency
  // shortens.
  bool small = false;
  // FEMBRAIN_PIPE_KLT7=0 keeps the (12, 6) instantiation at 9 and 10 slices per CU, where the LDS has room for 7 slots of a slice (65 / 9)
  // and the (12, 7) instantiation -- the same kernel with that unroll bound -- is the default
  bool klt7 = true;
  // FEMBRAIN_PIPE_HELPERS=0/1: helper wavefronts for very wide slices off / on; 2 (development) = the task table without a single helper.
  // Not set: the widest slice at least half again as wide as the average and wider than 24 slots
  int helpers = -1;
  // FEMBRAIN_PIPE_HELP_MINLEN (development): the shortest stream a helper halves
  int help_minlen = 16;
  // FEMBRAIN_PIPE_XYZ=0/1: the published vector in planes / node by node.  Not set: by the gather-line counts (fem_persist.hip pipe_layout)
  int xyz = -1;
  // FEMBRAIN_PIPE_LDS_BY_WIDTH=1 (measured and NOT the default): the workgroup's LDS dealt to its slices by width instead of in equal
  // shares, so that every wavefront streams about the same number of slots (the 27-slot slices of a cut among slices of 15 would keep 17
  // here instead of 5).  It is slower -- cut cube 21.9 against 20.1 us per iteration, Delaunay probe 22.0 against 18.6: a resident slot
  // still gathers its x entries from L2 / the fabric, and the compiled loop over resident slots has 6 slots' gathers in flight where
  // the hand-written stream never drains; on these meshes the product waits for gathers, not for matrix bytes.
  bool lds_by_width = false;
  // FEMBRAIN_PIPE_LDS_CAP=n (development): most slots of a slice in LDS with equal shares -- further groups of six run in the table-driven
  // kernel's second loop.  Not set (0): the unroll bound of the plain kernel, 6, or 12 with the node-by-node vector (pipe_help_tasks)
  int lds_cap = 0;
  // FEMBRAIN_PIPE_PLAIN_STORES=0/1: interior workgroups publish with plain stores.  Not set: where the iteration is latency-bound, up to 8
  // slices per CU (measured, us per iteration with / without: 9.5 / 10.2 at 466 slices, 9.5 / 9.9 at 1,000; 17.4 / 17.1 at 2,744 = 1M
  // tets, where the matrix stream evicts the lines from L2 anyway)
  int plain_stores = -1;
  // FEMBRAIN_PIPE_MIRROR=0: no LDS window (pcg_pipe_mirror.h).  Per HANDLE: what the first plan build read holds for its re-syncs
  bool mirror = true;
  // FEMBRAIN_PIPE_REGS=0|2|3: streamed slots per slice whose values the run-ahead LDS-window kernels keep in registers for a launch
  // (pcg_pipe_regs.hip.h).  Not set: as many as the instantiation holds, 3; 0: the kernel without
  int regs = -1;
  // FEMBRAIN_PIPE_PRIO=0|1|2|3: wavefront priority through the product of the register-slot kernels (and of the TIMING (12, 6) run-ahead kernel):
  // off, by progress, static (wavefronts 8-10 at 1), by progress + the service wavefront's collection at 1 (pcg_pipe.hip.h, "Priority 0 before
  // every wait").  Not set: kPipePrioDefault, what profiles/r10_prio_ab_cube56.txt decided; 0: the kernel without
  int prio = -1;
  // FEMBRAIN_TIMING (the library's): one line per decision on stderr
  bool verbose = false;
};

// The deal of the slices to the workgroups.  Equal NUMBERS of slices per workgroup (pipe_slices) is equal work only where the slices are
// alike; on a mesh with hull nodes of 40-60 neighbours the workgroups of the hull stream 2.5 x the slots of the others and every
// iteration waits for them (606k-tet Delaunay probe: product 18 us there, 7.5 on average).  Where the fullest workgroup of the equal
// deal has a quarter more slots than the average, the slices of every XCD's share are dealt to its workgroups by SLOTS instead
// (contiguous runs still, at most 12 -- or 24 where the two-row kernel is the mesh's anyway -- slices each).
// w: slices per workgroup of the equal deal.  Returns the most slices of a workgroup and fills wg_first (pipe_deal's table), or returns w
// and leaves it empty: equal numbers.
inline int pipe_deal_by_slots(const int* slice_off, int n_slices, int nb, int w, const PersistKnobs& kn, std::vector<int>* wg_first) {
  wg_first->clear();
  if (nb < 8 || w < 1 || w > 2 * kPipeMaxWaves) return w;
  const int per = nb / 8, chunk = ceil_div(n_slices, 8), cap = w <= kPipeMaxWaves ? kPipeMaxWaves : 2 * kPipeMaxWaves;
  long long total = 0, worst = 0;
  for (int b = 0; b < nb; b++) {
    int first, count;
    pipe_slices(n_slices, nb, b, &first, &count);
    const long long sl = count > 0 ? slice_off[first + count] - slice_off[first] : 0;
    total += sl;
    worst = std::max(worst, sl);
  }
  // (a fullest workgroup a quarter above the average -- or 15 % above it on a mesh whose widest slice is half again as wide as the mean:
  // the 56^3 cube after one cut, 200 slots against 171, 20.2 -> 19.3 us per iteration.  Forced on a uniform mesh the deal by slots is
  // SLOWER, 16.4 against 15.6 at 1M tets: some workgroups then hold 12 slices and a smaller LDS share each.)
  int widest = 0;
  for (int sl = 0; sl < n_slices; sl++) widest = std::max(widest, slice_off[sl + 1] - slice_off[sl]);
  const bool uneven = n_slices > 0 && (long long)widest * 2 * n_slices >= 3 * (long long)slice_off[n_slices];
  // (uneven WIDTHS only: on a small uniform mesh the fullest workgroup is a quarter above the average because it holds 2 slices where others
  // hold 1, which no deal changes -- and dealt by slots such a mesh was 2-5 % slower: 27^3 cube 8.65 -> 8.86 us per iteration, ventricle.blob 8.28 -> 8.62)
  const bool want = kn.balance >= 0 ? kn.balance != 0 : (uneven && (worst * nb * 4 > total * 5 || (w <= kPipeMaxWaves && worst * nb * 100 > total * 115)));  // (the two-row kernel at 13 slices per CU: 28.7 with the equal deal, 29.9 by slots)
  if (!want) return w;
  std::vector<int>& tab = *wg_first;
  tab.assign((size_t)2 * nb + 2, 0);
  int most = 0;
  for (int x = 0; x < 8; x++) {
    const int lo = std::min(x * chunk, n_slices), hi = std::min((x + 1) * chunk, n_slices);
    int at = lo;
    for (int j = 0; j < per; j++) {
      const int b = x + 8 * j, left = per - j;
      const long long rest = slice_off[hi] - slice_off[at];
      const double target = (double)rest / left;
      int n = 0;
      long long cum = 0;
      // at least what the workgroups behind cannot take, then slices while the run stays closer to its share than without the next one
      const int must = std::max(0, (hi - at) - (left - 1) * cap);
      while (at + n < hi && n < cap) {
        const long long wd = slice_off[at + n + 1] - slice_off[at + n];
        if (n >= must && left > 1 && (double)cum + 0.5 * (double)wd > target) break;
        cum += wd;
        n++;
      }
      tab[b] = at;
      tab[(size_t)nb + 1 + b] = n;
      at += n;
      most = std::max(most, n);
    }
  }
  tab[nb] = n_slices;
  if (kn.verbose) fprintf(stderr, "[fembrain] persistent solver: slices dealt by slots (fullest workgroup of the equal deal: %lld slots, average %.1f); up to %d slices per workgroup\n", worst, (double)total / nb, most);
  return std::max(1, most);
}

// LDS-resident slots of a workgroup's slices (widths wd): equal shares up to `cap` (the plain kernel's deal), or -- by_width -- the lowest
// level L with sum_j max(0, wd_j - L) <= the workgroup's wavefront-slots -- every slice then streams min(wd, L) slots -- and what is left
// over one more for the first slices that still stream.
inline void pipe_deal_lds(const std::vector<int>& wd, int lds_slots, bool by_width, int cap, std::vector<int>* res_out) {
  std::vector<int>& res = *res_out;
  const int count = (int)wd.size();
  if (!by_width) {
    const int lbase = std::min(cap, lds_slots / std::max(count, 1)), lrem = lbase < cap ? std::min(count, lds_slots - lbase * count) : 0;
    for (int j = 0; j < count; j++) res[j] = std::min(wd[j], lbase + (j < lrem ? 1 : 0));
    return;
  }
  int L = 0, widest = 0;
  for (int j = 0; j < count; j++) widest = std::max(widest, wd[j]);
  for (L = 0; L <= widest; L++) {
    int sum = 0;
    for (int j = 0; j < count; j++) sum += std::max(0, wd[j] - L);
    if (sum <= lds_slots) break;
  }
  int used = 0;
  for (int j = 0; j < count; j++) { res[j] = std::max(0, wd[j] - L); used += res[j]; }
  for (int j = 0; j < count && used < lds_slots; j++) if (res[j] < wd[j]) { res[j]++; used++; }
}

// One workgroup's row of the task table (PipeArgs::tasks): its slices' wavefronts own their streams; wavefronts without a slice -- idle
// slice wavefronts first, then the extra ones, up to `waves` -- take the upper halves of the longest streams, longest first, until none
// is left or no stream is as long as min_len slots (16 = 2 x 8).  Returns the helpers dealt.
inline int pipe_deal_streams(const std::vector<int>& wd, const std::vector<int>& res, bool want_h, int waves, int min_len, int4* tk) {
  struct Stream { int wave, slice, k0, k1, floor; };
  const int count = (int)wd.size();
  std::vector<Stream> st;
  int n_h = 0;
  for (int j = 0; j < kPipeTaskStride; j++) tk[j] = make_int4(-1, 0, 0, 0);
  for (int j = 0; j < count; j++) st.push_back({j, j, 0, wd[j], res[j]});
  std::vector<unsigned> mask(count, 0u);
  for (int hw = count; want_h && hw < waves && n_h < kPipeMaxHelpers; hw++) {
    int best = -1, len = 0;
    for (int i = 0; i < (int)st.size(); i++) {
      const int l = st[i].k1 - std::max(st[i].k0, st[i].floor);  // what it streams
      if (l > len) { len = l; best = i; }
    }
    if (best < 0 || len < min_len) break;
    const int lo = std::max(st[best].k0, st[best].floor), mid = lo + (st[best].k1 - lo + 1) / 2;
    const Stream up = {hw, st[best].slice, mid, st[best].k1, mid};
    st[best].k1 = mid;
    st.push_back(up);
    tk[hw] = make_int4(up.slice, up.k0, up.k1, n_h);
    mask[up.slice] |= 1u << n_h;  // the owner adds this helper's partial sums
    n_h++;
  }
  for (const Stream& S : st) {
    if (S.wave < count) tk[S.wave] = make_int4(res[S.wave], 0, S.k1, (int)mask[S.wave]);  // owner: resident slots, (their place: below), end of its own stream, its helpers
    else { tk[S.wave].y = S.k0; tk[S.wave].z = S.k1; }                                   // (ends moved by later splits)
  }
  int at = 0;
  for (int j = 0; j < count; j++) { tk[j].y = at; at += res[j]; }
  return n_h;
}

// The task table of the (12, 6, HELP) kernel and its LDS deal, for every workgroup.  Helpers for very wide slices (unsharded, one row per
// lane, Jacobi): a workgroup's wavefronts without a slice of their own -- those its neighbours' fuller deal leaves idle, and the ones
// launched for the purpose: the 12-wavefront instantiation then serves fewer than 9 slices per CU too -- take the upper halves of the
// longest streams.  wg_first: pipe_deal's table or nullptr; w: most slices of a workgroup (<= kPipeMaxWaves).
struct PipeTasks {
  std::vector<int4> tasks;               // [nb][kPipeTaskStride]
  int most = 0, all = 0, deepest = 0;    // most helper tasks of a workgroup; all of them; most LDS-resident slots of a slice
  int help_waves = 0;                    // wavefronts launched for the helpers beyond slices + the service wavefront
};
inline PipeTasks pipe_help_tasks(const int* slice_off, int n_slices, const int* wg_first, int nb, int w, bool c16, bool want_h, bool want_xyz, const PersistKnobs& kn) {
  PipeTasks T;
  T.help_waves = std::max(0, kPipeMaxWaves - w - 1);   // (the 12-wavefront kernel: slices, helpers, the service wavefront)
  T.tasks.assign((size_t)nb * kPipeTaskStride, make_int4(-1, 0, 0, 0));
  const int lds_all = pipe_lds_slots(c16), lds_help = pipe_help_slots(c16);
  // (with the node-by-node vector a resident slot's gathers cost a third of the lines, and slices that keep up to 12 slots in LDS instead
  // of 6 pay: sliver-free unstructured probe 16.2 -> 14.4 us per iteration, Delaunay probe 16.25 -> 15.9; 18 buys nothing more)
  // -- from 6 slices per CU on: with fewer, idle wavefronts split the streams (helpers) and a long LDS loop in the owner only delays them:
  // 27,000 / 46,656 / 64,000-node lattices 11.0 / 12.2 / 13.5 us per iteration with 6 slots against 12.9 / 13.4 / 14.1 with 12
  const int cap = kn.lds_cap > 0 ? kn.lds_cap : (want_xyz && w >= 6 ? 12 : 6);
  for (int b = 0; b < nb; b++) {
    int first, count;
    pipe_deal(wg_first, n_slices, nb, b, &first, &count);
    int4* tk = &T.tasks[(size_t)b * kPipeTaskStride];
    std::vector<int> wd(count), res(count);
    for (int j = 0; j < count; j++) wd[j] = slice_off[first + j + 1] - slice_off[first + j];
    // first with the helpers' hand-over area set aside; a workgroup that gets no helper is dealt again with all of the LDS
    pipe_deal_lds(wd, lds_all - lds_help, kn.lds_by_width, cap, &res);
    int n_h = pipe_deal_streams(wd, res, want_h, w + T.help_waves, kn.help_minlen, tk);
    if (n_h == 0) {
      pipe_deal_lds(wd, lds_all, kn.lds_by_width, cap, &res);
      n_h = pipe_deal_streams(wd, res, want_h, w + T.help_waves, kn.help_minlen, tk);
    }
    for (int j = 0; j < count; j++) T.deepest = std::max(T.deepest, res[j]);
    T.most = std::max(T.most, n_h);
    T.all += n_h;
  }
  return T;
}

// ---- the sharded persistent solver (pcg_shard_box.hip.h).  rg: per slice (first owned column, last, bit mask of the ranks whose halo
// rows it gathers), k_slice_colrange_shard's output ----

// slice -> workgroup.  A workgroup whose slices gather halo rows gets its input later than the others by the length of the
// cross-rank chain (drain -> counter -> proxy copy -> flag; ~4.5 us between two processes on one MI355X) EVERY iteration, and the
// whole grid ends up at its pace.  So it is dealt fewer slices ("relief", PersistKnobs::shard_relief, default 35 % of the
// slices per CU): its shorter product absorbs the wait.  Returns the most slices of a workgroup; *relief_out: the relief that held.
inline int shard_deal(const std::vector<int4>& rg, int n_slices, int nb, int w, const PersistKnobs& kn, std::vector<int2>* wg_range_out, int* relief_out) {
  std::vector<int2>& wg_range = *wg_range_out;   // first slice and slice count of every workgroup
  wg_range.assign((size_t)nb, make_int2(0, 0));
  int halo_slices = 0;
  for (int sl = 0; sl < n_slices; sl++) halo_slices += rg[sl].z != 0 ? 1 : 0;
  const int relief_default = 12 * halo_slices <= n_slices ? std::max(0, (w * 35 + 50) / 100) : 0;
  int Q = w, relief = std::min(w - 1, kn.shard_relief >= 0 ? kn.shard_relief : relief_default);
  for (;; relief--) {
    Q = 0;
    if (relief <= 0 || (nb & 7)) {  // the even deal of the unsharded kernel
      relief = 0;
      for (int b = 0; b < nb; b++) {
        int first, count;
        pipe_slices(n_slices, nb, b, &first, &count);
        wg_range[b] = make_int2(first, count);
        Q = std::max(Q, count);
      }
      break;
    }
    // a slice that gathers halo rows weighs w / (w - relief) slices; equal weight per workgroup, contiguous, and in pipe_slices'
    // order: the workgroups of XCD b & 7 (round-robin dispatch) hold a contiguous eighth
    const double rho = (double)w / (double)(w - relief);
    double W = 0;
    for (int sl = 0; sl < n_slices; sl++) W += rg[sl].z != 0 ? rho : 1.0;
    std::vector<int> start((size_t)nb + 1, n_slices);
    double acc = 0;
    int pos = 0;
    for (int sl = 0; sl < n_slices; sl++) {
      while (pos < nb && acc >= W * pos / nb - 1e-9) start[pos++] = sl;   // position pos starts at the first slice at or past its share
      acc += rg[sl].z != 0 ? rho : 1.0;
    }
    const int per = nb >> 3;
    for (int p2 = 0; p2 < nb; p2++) {
      const int b = (p2 % per) * 8 + p2 / per;
      wg_range[b] = make_int2(start[p2], start[p2 + 1] - start[p2]);
      Q = std::max(Q, start[p2 + 1] - start[p2]);
    }
    if (Q <= 2 * (kPipeMaxWaves - 1)) break;
  }
  *relief_out = relief;
  return Q;
}

// per-row send lists and per-workgroup destination masks from the plan's send lists (ascending owned ids per destination: the
// position of a row in that list is its position in the destination's halo segment of this rank).  owner: workgroup of every slice
struct ShardSendLists { std::vector<int> row_off, row_rank, row_pos; std::vector<unsigned int> wg_mask; };
inline ShardSendLists shard_send_lists(const FemPlan& P, const std::vector<int>& owner, int nb) {
  ShardSendLists L;
  const int R = P.n_ranks;
  L.row_off.assign((size_t)P.n_owned + 1, 0);
  for (int q = 0; q < R; q++)
    for (int k = P.send_off[q]; k < P.send_off[q + 1]; k++) L.row_off[(size_t)P.send_local[k] + 1]++;
  for (int a = 0; a < P.n_owned; a++) L.row_off[(size_t)a + 1] += L.row_off[a];
  L.row_rank.assign((size_t)std::max(1, L.row_off[P.n_owned]), 0);
  L.row_pos.assign(L.row_rank.size(), 0);
  std::vector<int> fill(L.row_off.begin(), L.row_off.end() - 1);
  L.wg_mask.assign((size_t)nb, 0u);
  for (int q = 0; q < R; q++)
    for (int k = P.send_off[q]; k < P.send_off[q + 1]; k++) {
      const int a = P.send_local[k];
      L.row_rank[fill[a]] = q; L.row_pos[fill[a]] = k - P.send_off[q]; fill[a]++;
      L.wg_mask[owner[a >> 6]] |= 1u << q;
    }
  return L;
}

// proxies: up to kShardProxies per rank I have halo nodes of, dealt to the workgroups from the last one downwards.  Returns K, the
// proxies per source rank; proxy[q * K + k]: its workgroup or -1; duty[b * kShardDuties + i]: the proxies workgroup b serves
inline int shard_proxies(const FemPlan& P, int nb, std::vector<int>* proxy, std::vector<int>* duty) {
  const int R = P.n_ranks;
  int n_src = 0;
  for (int q = 0; q < R; q++) n_src += P.halo_off[q + 1] > P.halo_off[q];
  const int K = std::max(1, std::min(kShardProxies, nb * kShardDuties / std::max(1, n_src)));
  proxy->assign((size_t)R * K, -1);
  duty->assign((size_t)nb * kShardDuties, -1);
  std::vector<int> n_duty((size_t)nb, 0);
  for (int q = 0, idx = 0; q < R; q++)
    for (int k = 0; k < K; k++) {
      int lo, hi;
      shard_proxy_rows(P.halo_off[q], P.halo_off[q + 1], K, k, &lo, &hi);
      if (hi <= lo) continue;
      const int b = nb - 1 - (idx++ % nb);   // (idx < nb * kShardDuties by the choice of K)
      (*proxy)[(size_t)q * K + k] = b;
      (*duty)[(size_t)b * kShardDuties + n_duty[b]++] = q * K + k;
    }
  return K;
}

// producer lists: local workgroups from the owned column range of every slice, proxies from the ranks its halo columns belong to.
// Returns the longest list (-1: some workgroup polls all); cnt[b] = -1: workgroup b polls all
inline int shard_producers(const std::vector<int4>& rg, const std::vector<int2>& wg_range, const std::vector<int>& owner, const std::vector<int>& proxy, int n_slices,
                           int nb, int R, int K, std::vector<int>* prod_out, std::vector<int>* cnt_out) {
  std::vector<int>& prod = *prod_out;
  std::vector<int>& cnt = *cnt_out;
  prod.assign((size_t)nb * kPipeMaxProducers, -1);
  cnt.assign((size_t)nb, 0);
  std::vector<char> mark((size_t)nb + (size_t)R * K);
  int longest = 0;
  for (int b = 0; b < nb; b++) {
    std::fill(mark.begin(), mark.end(), 0);
    int n = 0;
    for (int sl0 = wg_range[b].x; sl0 < wg_range[b].x + wg_range[b].y; sl0++) {
      const int4 r = rg[sl0];
      for (int sl = r.x >> 6; r.y >= r.x && sl <= (r.y >> 6) && sl < n_slices; sl++) {
        const int o = owner[sl];
        if (o != b && !mark[o]) { mark[o] = 1; n++; }
      }
      for (int q = 0; q < R; q++)
        if ((unsigned int)r.z >> q & 1u)
          for (int kk = 0; kk < K; kk++)   // (all proxies of a rank this slice gathers halo rows of)
            if (proxy[(size_t)q * K + kk] >= 0 && !mark[nb + q * K + kk]) { mark[nb + q * K + kk] = 1; n++; }
    }
    if (n > kPipeMaxProducers) { cnt[b] = -1; longest = -1; continue; }
    cnt[b] = n;
    if (longest >= 0) longest = std::max(longest, n);
    for (int o = 0, k = 0; o < nb + R * K; o++) if (mark[o]) prod[(size_t)b * kPipeMaxProducers + k++] = o;
  }
  return longest;
}

}  // namespace fb
