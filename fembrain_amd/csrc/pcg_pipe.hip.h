// Persistent PIPELINED Jacobi-PCG (included by fem_persist.hip only): a whole solve of CGSolver.cpp:129-190 inside ONE launch, for
// systems whose vectors fit on the chip.  One workgroup per CU owns a fixed run of SELL slices, one wavefront per slice, one
// lane per block row; the lane keeps its row of x, r, w, z, s, p and 1/diag in REGISTERS for the whole solve.
//
// Why pipelined.  The merged-reduction iteration of round 2 (k_pcg_persist) crossed the chip twice per iteration: the three
// sums all-to-all (alpha, beta are needed before the new search direction exists), then the new direction to the neighbours
// -- 9 of its 22 us at 1M tets were those two hand-offs, with the memory system idle.  The recurrences of Ghysels & Vanroose
// (pipelined CG, Parallel Computing 40 (2014), Alg. 4; M = diag folded in: u = r/diag, m = w/diag) compute the SAME iterates in
// exact arithmetic from
//     gamma = r . u,  delta = w . u                (both sums of LOCAL quantities, known before the product starts)
//     n = A m,  m = w / diag                       (the product of the iteration)
//     beta = gamma / gamma_old,  alpha = gamma / (delta - beta gamma / alpha_old)
//     z = n + beta z,  s = w + beta s,  p = u + beta p,  x += alpha p,  r -= alpha s,  w -= alpha z
// so the sums are POSTED before the product and READ after it (their trip across the chip hides behind ~10 us of matrix
// stream), and the only wait of an iteration is for the m of the few workgroups whose rows this workgroup's columns touch
// (+-5 workgroups on the slab-ordered cube; per-workgroup producer lists built at plan time, "all" as the fall-back).
// Every 30th iteration takes the exact residual r = b - A x as the reference does (CGSolver.cpp:159-166), and with it
// w = A (r / diag), as two more in-launch products.  Measured against the literal solver on the oracle's systems
// (tools/pipelined_pcg_numerics.py): identical iteration counts at 4k..1M tets, solutions equal to 1e-7 (both stop at 1e-6).
//
// Hand-off form (MI355X_MICROARCH.md, "valid forms"): payload sc1 stores -> s_waitcnt vmcnt(0) -> workgroup barrier -> ONE
// sc1 flag store per workgroup; consumer: agent-scope acquire issued early (buffer_inv sc1: nothing of this CU loads the
// planes between it and the barrier), sc1 poll of the producers' flags, s_waitcnt vmcnt(0), workgroup barrier, plain loads.
// The sums travel as tagged 8-byte granules (value half + sequence number in one store: no flag, no ordering).
// Hazards: the planes are double-buffered by publish parity -- a workgroup overwrites buffer P two publishes after it was
// filled, and it can be there only after every consumer of its rows has published in between, i.e. finished its reads
// (consumers of my rows = producers of my columns: A is symmetric, and the wait on them is part of every product); sums are
// double-buffered by sequence parity the same way.  Every spin is bounded by the wall clock; on expiry an error word is
// set, every other spin sees it, the launch drains WITHOUT writing any state back and the host re-solves with the
// two-launch form (fb_step_info.pcg_path says so).
//
// Run-ahead form (round 8; the AHEAD instantiations, chosen per LAUNCH by the host for every launch with a service wavefront of an unsharded
// handle without helpers -- never per wavefront: all wavefronts of a workgroup execute the same barriers).  The wavefronts of a workgroup
// finish a product in tiers 1.7 us apart (oldest-first arbitration per SIMD), and the barrier behind the sums, which the data flow does
// not need, made the fast ones wait for the slowest before any of them started its recurrences and publish stores.  The cross-workgroup
// protocol above is untouched; inside the workgroup the service wavefront writes the totals and the failure word bc[0..2] and then
// RELEASES (workgroup scope) a sequence word, bc[6], holding their `sums` number; a wavefront whose product is done ACQUIRES that word
// until it holds the current number -- it normally does, the collection ran during the product -- reads the totals and goes on alone:
// convergence test, recurrences, publish, its parts of the next gamma and delta into wsum, the drain of its stores.  The two barriers of
// product() stay.  (An arrival counter in place of the first of them, so that only wavefront 0 waits for the drains, was measured and did
// not pay: docs/HISTORY.md B.)
// Hazards of the form.  The totals need no double buffer: the service wavefront writes iteration i+1's only behind the barrier that follows
// the poll of product i+1, and every sibling reaches that barrier after it has read iteration i's.  The sequence word is set to the previous
// launch's last `sums` number before the first product's barriers, the first wait for it lies behind them.  A publish overwrites the
// buffer of two products ago: this wavefront is behind the barriers of the last product, so every producer (= consumer) of its rows had
// flagged that product, and a flag follows a barrier of its workgroup behind the product before.  wsum is rewritten behind the barrier
// that follows wavefront 0's read of it, bc[3] / bc[5] are read behind the barrier they are written in front of, as before.
// Bounded waits, uniform exits.  Every decision to leave the solver loop is taken from values all wavefronts of the workgroup read alike:
// the bits of gamma and bc[2] from the hand-over (done, a failed collection), bc[3] behind the poll's barrier (a failed wait for the
// neighbours), and the count of iterations against n_iters (every wavefront counts the same iterations).  The siblings decide nothing on
// their own: their wait for the totals has no clock because the service wavefront's collection has one and ALWAYS ends in a hand-over, of
// totals or of failure, and the service wavefront meets no wait between the barrier behind the poll and its collection.  A wavefront that
// leaves the loop executes no barrier any more, and no sibling waits at one for it: between the second barrier of a product and the exits
// that follow it (the hand-over, the iteration count at the head of the loop) there is none, and every sibling takes the same exit.
// Priority 0 before every wait (round 10; the PRIO instantiations: the (12, 6) and (12, 7) register-slot kernels and the TIMING (12, 6) run-ahead one,
// FEMBRAIN_PIPE_PRIO).  VALU issue on a SIMD goes by priority, then age, so the youngest of a SIMD's three slice wavefronts finishes its product 1.7-2 us
// behind the oldest, and the product's barrier waits for it.  PRIO = 1 (progress): a slice wavefront raises itself to 3 behind the second barrier of
// product() and steps down as it gets on -- 2 into the on-chip run, 1 into the plain layers, 0 into the register layers behind the window or the streamed
// rest -- so the sibling furthest behind wins the arbitration; PRIO = 2 (static): wavefronts 8-10 run their product at 1; PRIO = 3: progress, and the
// service wavefront collects the sums at 1.  The rule that keeps this from starving anyone: a wavefront is above priority 0 ONLY between the second barrier
// of a product and that product's last slot (the service wavefront: between that barrier and its hand-over, and not while it polls a record that is
// missing).  It is at 0 at both barriers, during wavefront 0's poll, in every spin and s_sleep, through the wait for the totals, the recurrences, the
// publish stores and their drain, and at every exit: the raised region contains no wait, no branch that leaves the loop and no return -- a failed wait
// for the neighbours returns in front of it, a failed collection is handed over behind it, the iteration cap is tested at 0.  The steps are taken from
// the wave-uniform values the regions are entered by; no control flow depends on them.
#pragma once
#include "fem_kernels.h"
#include "pcg_pipe_stream.hip.h"
#include "pcg_pipe_onchip.hip.h"
#include "pcg_pipe_mirror.h"
#include "pcg_pipe_regs.hip.h"  // (last of the three: it renames the temporaries of their text)

namespace fb {

constexpr int kPipeMaxWaves = 12;    // wavefronts (= slices) per workgroup
constexpr int kPipeMaxBlocks = 256;  // workgroups = CUs
constexpr int kPipeSyncDoubles = 2 * 16 + 2 * kPipeMaxBlocks + 8;  // LDS in front of the resident values: wave sums | gathered sums | broadcast
constexpr int kPipeMaxProducers = 64;
// LDS-resident slots of the matrix: 9 values and the column per lane.  With 32-bit columns a wavefront-slot is 10 x 64 words = 2,560 B and 62 fit
// the CU's 160 KB beside the sync buffers; with 16-bit column differences (C16) it is 9 x 64 words + 64 halfwords = 2,432 B and 65 fit (round 5;
// rounds 3-4: 60 slots of 2,560 B either way -- a streamed slot of a slice costs 1.0 us per iteration at 1M tets).
constexpr int pipe_slot_bytes(bool c16) { return c16 ? 9 * 256 + 128 : 10 * 256; }
constexpr int pipe_lds_slots(bool c16) { return c16 ? 65 : 62; }
static_assert(sizeof(double) * kPipeSyncDoubles + (size_t)pipe_lds_slots(false) * pipe_slot_bytes(false) <= 160 * 1024, "LDS budget of k_pcg_pipe");
static_assert(sizeof(double) * kPipeSyncDoubles + (size_t)pipe_lds_slots(true) * pipe_slot_bytes(true) <= 160 * 1024, "LDS budget of k_pcg_pipe<c16>");
static_assert(mir_slot_bytes(true) == pipe_slot_bytes(true) && mir_slot_bytes(false) == pipe_slot_bytes(false) && mir_lds_slots(true) == pipe_lds_slots(true) &&
              mir_lds_slots(false) == pipe_lds_slots(false) && kMirWaves == kPipeMaxWaves, "the LDS window's planner sees the kernel's LDS");
static_assert(pipe_lds_slots(true) * pipe_slot_bytes(true) / 4 < 65536 && pipe_lds_slots(false) * pipe_slot_bytes(false) / 4 < 65536, "16-bit LDS word addresses of the mirror layers");

struct PipeArgs {
  unsigned long long* post;   // [2][n_blocks][4] granules: (hi, lo) of gamma, delta, each | sequence << 32
  unsigned int* flags;        // [n_blocks (padded to 4)]: publish number of the workgroup's last complete plane store
  unsigned int* error;        // set on a timed-out wait
  unsigned int* seqs;         // [2] publish / sum sequence numbers reached by the previous launch (block 0 writes them at the end)
  const int* producers;       // [n_blocks][64] workgroups whose rows this workgroup's columns touch; prod_count < 0: poll all
  const int* prod_count;      // [n_blocks]
  const int* prod_xcd;        // [n_blocks] non-zero: a producer (= consumer) of this workgroup sits on another XCD, or it polls all
  int plain_local;            // non-zero: workgroups without such a neighbour publish with plain stores (see publish)
  unsigned int* xcc;          // [n_blocks] (first publish number of the launch) << 4 | HW_REG_XCC_ID of the workgroup: where it REALLY runs
  int prefetch_slots;         // streamed slots per slice whose values the idle wavefronts pull into L2 during the neighbour wait (0..4)
  int service;                // non-zero: the workgroups were launched with one wavefront more than slices; it collects the sums
  int start;                  // 0 continue a solve (state from memory), 1 new solve from x = 0, 2 new solve from the x in memory
  int n_iters;                // at most this many iterations in this launch
  double eps2;                // squared tolerance (start != 0; a continued solve reads the CGState)
  int max_iter;
  long long timeout_ticks;    // wall_clock64 ticks (100 MHz)
  long long* timing;          // development aid (FEMBRAIN_PERSIST_TIMING=1), else null: per wavefront kPipeTimingSlots words: 5 accumulated phase times,
                              // the iterations, and of the product phase the first streamed part and the on-chip run (the LDS window's kernels)
  double* planes;             // [2][3][n_pad]: the published vector as the gathers read it, x | y | z planes
  size_t n_pad;               // rows padded to whole slices
  double* pstate;             // [2] gamma_old, alpha_old between the launches of one solve
  // Helpers (round 5): on a mesh with a few very wide slices (hull nodes of a Delaunay mesh: 59 slots against 19 on average) the product
  // of an iteration is as slow as the widest slice of the slowest workgroup -- one wavefront streams a slice's slots one after the other
  // (18 us against 7.5 on average on the 606k-tet probe, profiles/r05_delaunay_phase_table.txt).  Wavefronts without a slice of their own
  // then take the upper part of a wide slice's slots.  tasks[b][wv] of a HELPER = (slice of the workgroup, first slot, end slot, its number
  // in the workgroup = its place in the LDS hand-over), slice -1 = no task; of the wavefront that OWNS a slice = (slots of the slice resident
  // in LDS, where in LDS (in wavefront-slots), end of what it streams itself, bit mask of the helpers whose partial sums it adds -- ascending:
  // a fixed order).  The resident slots of a workgroup are dealt by WIDTH (pcg_pipe_plan.h, pipe_deal_lds): the slices stream equal numbers of slots
  // as far as the LDS goes, where the plain kernel gives every slice the same share.  nullptr: the plain kernel (every regular mesh).
  const int* wg_first;        // the deal of the slices to the workgroups balanced by slots (pipe_deal), or nullptr: equal numbers of slices
  const int4* tasks;          // [n_blocks][kPipeTaskStride]
  int n_help;                 // most helpers of any workgroup (0: none; LDS for their partial sums is set aside when > 0)
  // The LDS window (pcg_pipe_mirror.h, k_pipe_mirror_plan; the (12, 6) and (12, 7) instantiations only), nullptr: the first slots of every slice
  // are its resident ones.  mirror[b][wv] = (a | m << 8 | p << 16, first wavefront-slot of the plain layers, byte offset of the mirror table,
  // register slots r of the slice: read by the REGS instantiations only, pcg_pipe_regs.hip.h);
  // mir_addr[slice][kMirMax][64] LDS word addresses of the blocks the mirror layers read transposed; the pool: mir_wg[b] = (first LDS word,
  // entries), mir_pool[b][kMirPoolMax] the index in `vals` of each entry's block.
  const int4* mirror;
  const unsigned short* mir_addr;
  const int2* mir_wg;
  const int* mir_pool;
};
constexpr int kPipeTaskStride = 16;
constexpr int kPipeTimingSlots = 8;  // PipeArgs::timing words per wavefront
constexpr int kPipeMaxHelpers = 8;   // per workgroup
constexpr int pipe_help_slots(bool c16) { return c16 ? 6 : 5; }  // LDS wavefront-slots set aside for their partial sums (8 x 3 x 64 doubles = 12,288 B, at the end of the slots)
static_assert(pipe_help_slots(true) * pipe_slot_bytes(true) >= kPipeMaxHelpers * 3 * 64 * 8 && pipe_help_slots(false) * pipe_slot_bytes(false) >= kPipeMaxHelpers * 3 * 64 * 8, "helpers' hand-over area");

__device__ __forceinline__ void st_sc1_u64(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1_u32(unsigned int* p, unsigned int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned int ld_sc1_u32(const unsigned int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1_f64(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a node's three doubles (24 consecutive bytes, 8-byte aligned) in two stores instead of three, write-through like st_sc1_f64
__device__ __forceinline__ void st_sc1_xyz(double* p, double x, double y, double z) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const d2 xy = {x, y};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\tglobal_store_dwordx2 %0, %2, off offset:16 sc1" : : "v"(p), "v"(xy), "v"(z) : "memory");
}
// one 16-byte sc1 load, waited for (a poll of four flags / two granules in one request)
__device__ __forceinline__ uint4 ld_sc1_u128(const void* p) {
  uint4 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}

// The wavefront's issue priority (0..3; header, "Priority 0 before every wait").  The instruction is scalar and ignores EXEC; as a volatile statement it
// keeps its place among the volatile assembly regions and every memory operation, and a branch around it is kept even where no lane is active.
template <int P>
__device__ __forceinline__ void pipe_setprio() {
  static_assert(P >= 0 && P <= 3, "s_setprio takes 0..3");
  asm volatile("s_setprio %0" : : "n"(P) : "memory");
}

// a value every lane holds alike, moved to scalar registers (a uniform double in vector registers costs two per lane for nothing)
__device__ __forceinline__ double uniform_f64(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)(b & 0xffffffffLL)), hi = __builtin_amdgcn_readfirstlane((unsigned int)((unsigned long long)b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ bool uniform_flag(bool f) { return __builtin_amdgcn_readfirstlane(f ? 1 : 0) != 0; }

// slices of workgroup b: XCD b & 7 keeps the contiguous eighth of the rows it has in every other FEM kernel (SliceWalk); its
// n_blocks/8 workgroups share that slab as evenly as whole slices allow.  Host and device use the same function.
__host__ __device__ inline void pipe_slices(int n_slices, int n_blocks, int b, int* first, int* count) {
  const int xcd = b & 7, j = b >> 3, per = n_blocks >> 3;
  const int chunk = (n_slices + 7) >> 3;
  const int lo = xcd * chunk;
  int len = n_slices - lo;
  len = len < 0 ? 0 : (len > chunk ? chunk : len);
  const int base = len / per, rem = len - base * per;
  *first = lo + j * base + (j < rem ? j : rem);
  *count = base + (j < rem ? 1 : 0);
}

// ... or, where the slices of a mesh differ much in width (hull nodes of a Delaunay mesh: 59 slots against 19 on average), from a table
// the host has balanced by SLOTS (pcg_pipe_plan.h pipe_deal_by_slots): a CU's product takes as long as the slots it streams, whoever streams them --
// the workgroups of the hull took 18 us per product against 7.5 on average with an equal number of slices each (profiles/r05_delaunay_phase_table.txt).
// wg_first: n_blocks + 1 first slices, ascending inside every XCD's share; nullptr: the formula above.
__host__ __device__ inline void pipe_deal(const int* wg_first, int n_slices, int n_blocks, int b, int* first, int* count) {
  if (wg_first) { *first = wg_first[b]; *count = wg_first[n_blocks + 1 + b]; }
  else pipe_slices(n_slices, n_blocks, b, first, count);
}

// The workgroups whose rows the columns of a slice lie in: a bit mask over the (at most kPipeMaxBlocks = 256) workgroups, 8 words per
// slice.  EXACT, where a column range per slice (rounds 2-3) gave a superset: one element that joins two distant nodes (a sliver on the hull of a Delaunay
// mesh, a cut that was closed again) widens the range of its slice to "everyone" but adds ONE producer to the exact list.
__global__ __launch_bounds__(kBlock) void k_slice_producers(int n_slices, int n_owned, const int* __restrict__ slice_off, const int* __restrict__ colidx,
                                                            const int* __restrict__ slice_owner, unsigned int* __restrict__ out) {
  const int s = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= n_slices) return;
  const int row = s * 64 + lane;
  unsigned int m[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (row < n_owned) {
    // four slots at a time, their columns and then their owners in flight together (one slot after the other was a chain of two dependent
    // loads per slot: 38-44 us of every re-sync at 1.1M tets)
    const int k1 = slice_off[s + 1];
    for (int k0 = slice_off[s]; k0 < k1; k0 += 4) {
      int c[4], o[4];
#pragma unroll
      for (int j = 0; j < 4; j++) c[j] = k0 + j < k1 ? colidx[(size_t)(k0 + j) * 64 + lane] : n_owned;
#pragma unroll
      for (int j = 0; j < 4; j++) o[j] = c[j] < n_owned ? slice_owner[c[j] >> 6] : -1;  // (>= n_owned: a shard's halo column, the proxies' business)
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (o[j] >= 0) {
#pragma unroll
          for (int i = 0; i < 8; i++) m[i] |= (o[j] >> 5) == i ? 1u << (o[j] & 31) : 0u;
        }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m[i] |= __shfl_xor(m[i], off, 64);
    if (lane == 0) out[(size_t)s * 8 + i] = m[i];
  }
}

// owner[slice] = the workgroup pipe_slices gives it to (a thread per workgroup)
__global__ __launch_bounds__(kBlock) void k_slice_owner(int n_slices, int nb, const int* __restrict__ wg_first, int* __restrict__ owner) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= nb) return;
  int first, count;
  pipe_deal(wg_first, n_slices, nb, b, &first, &count);
  for (int k = 0; k < count; k++) owner[first + k] = b;
}

// The producer list of every workgroup from the masks of its slices (a thread per workgroup; round 4: on the device, the host loop
// with its download and three uploads was 0.2 ms of every re-sync): prod[b][0..cnt[b]) ascending, cnt[b] = -1 (poll everyone) beyond
// kPipeMaxProducers, far[b] = a producer sits on another XCD, stats[0] = longest list, stats[1] = some workgroup polls everyone.
__global__ __launch_bounds__(kBlock) void k_wg_producers(int n_slices, int nb, const int* __restrict__ wg_first, const unsigned int* __restrict__ mask, int poll_all,
                                                         int* __restrict__ prod, int* __restrict__ cnt, int* __restrict__ far, int* __restrict__ stats) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= nb) return;
  int first, count;
  pipe_deal(wg_first, n_slices, nb, b, &first, &count);
  unsigned int m[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  for (int k = 0; k < count; k++)
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] |= mask[(size_t)(first + k) * 8 + i];
#pragma unroll
  for (int i = 0; i < 8; i++)
    if ((b >> 5) == i) m[i] &= ~(1u << (b & 31));
  int n = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) n += __popc(m[i]);
  int* mine = prod + (size_t)b * kPipeMaxProducers;
  if (n > kPipeMaxProducers || poll_all) {
    for (int k = 0; k < kPipeMaxProducers; k++) mine[k] = -1;
    cnt[b] = -1; far[b] = 1;
    atomicOr(&stats[1], 1);
    return;
  }
  int k = 0, f = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    unsigned int w = m[i];
    while (w) {
      const int o = 32 * i + __ffs((int)w) - 1;
      w &= w - 1u;
      mine[k++] = o;
      if ((o & 7) != (b & 7)) f = 1;
    }
  }
  for (; k < kPipeMaxProducers; k++) mine[k] = -1;
  cnt[b] = n; far[b] = f;
  atomicMax(&stats[0], n);
}

// The LDS window of every workgroup (pcg_pipe_mirror.h), a workgroup of the plan per persistent workgroup, a wavefront per slice:
// wave_out[b][w] = (a | m << 8 | p << 16, first wavefront-slot of the plain layers, byte offset of the mirror table, register slots: mir_reg_slots of
// `regs`); addr_out[slice][k][64] = the
// LDS word address of mirror layer k's block to read transposed (the partner's plain block or a pool entry); pool_src[b][e] = the index in `vals` of
// the lane's own block that pool entry e holds; wg_out[b] = (pool's first LDS word, entries); stats += (mirror layers, pool entries), min= plain layers,
// stats[3] += register slots.
// A workgroup whose window would not keep more slots on chip than the plain share gets the plain kernel's layout (no mirrors, no pool).
__global__ __launch_bounds__(64 * kMirWaves) void k_pipe_mirror_plan(int n_slices, int n_owned, const int* __restrict__ slice_off, const int* __restrict__ colidx,
                                                                   const int* __restrict__ wg_first, int klt, int c16i, int regs, int4* __restrict__ wave_out,
                                                                   unsigned short* __restrict__ addr_out, int* __restrict__ pool_src, int2* __restrict__ wg_out,
                                                                   int* __restrict__ stats) {
  const bool c16 = c16i != 0;
  __shared__ MirWave mw[kMirWaves];
  __shared__ int cnt[kMirWaves];
  __shared__ int ok;
  const int b = blockIdx.x, nb = gridDim.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int first, count;
  pipe_deal(wg_first, n_slices, nb, b, &first, &count);
  count = min(count, kMirWaves);
  const int lo = first * 64, hi = min((first + count) * 64, n_owned);
  if (w < count) {  // the diagonal slot most lanes have, and the layers below it whose columns are lower rows of this workgroup
    const int sl = first + w, width = slice_off[sl + 1] - slice_off[sl];
    const int dk = mir_lane_diag(slice_off, colidx, sl, lane, n_owned);
    int d = -1, best = 0;
    for (int k = 0; k < width; k++) {
      const int c = __popcll(__ballot(dk == k));
      if (c > best) { best = c; d = k; }
    }
    int m = 0;
    if (d >= 0)
      for (; m < kMirMax && d - 1 - m >= 0; m++)
        if (__popcll(__ballot(mir_lane_lower(slice_off, colidx, sl, d - 1 - m, lane, lo, hi))) < kMirLanes) break;
    if (lane == 0) { mw[w].d = d; mw[w].m = m; mw[w].width = width; }
  }
  __syncthreads();
  if (threadIdx.x == 0) ok = count > 0 && mir_wg_layout(mw, count, klt, c16, 0, false) ? 1 : 0;
  __syncthreads();
  // the lanes without a resident partner block, twice: with the least plain share; then with the plain layers the pool leaves room for (more
  // partner slots resident: never more lanes)
  for (int pass = 0; pass < 2; pass++) {
    if (ok && w < count) {
      int e = 0;
      for (int k = 0; k < mw[w].m; k++) e += __popcll(__ballot(mir_lane_addr(slice_off, colidx, first, mw, w, k, lane, lo, hi, c16) < 0));
      if (lane == 0) cnt[w] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0 && ok) {
      int E = 0;
      for (int v = 0; v < count; v++) E += cnt[v];
      if (pass == 0) ok = E <= kMirPoolMax && mir_wg_layout(mw, count, klt, c16, E, true) ? 1 : 0;
      else ok = mir_wg_gains(mw, count, klt, c16) ? 1 : 0;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (!ok) mir_wg_plain(mw, count, klt, c16);
    int E = 0, layers = 0, fewest = 1 << 30, held = 0;
    for (int v = 0; v < count; v++) {
      const int e = ok ? cnt[v] : 0;
      cnt[v] = E;  // (exclusive prefix: the first pool entry of slice v)
      E += e; layers += mw[v].m; fewest = min(fewest, mw[v].p); held += mir_reg_slots(mw[v], regs);
    }
    if (held > 0) atomicAdd(&stats[3], held);
    wg_out[b] = make_int2(mir_pool_at(mw, count, c16) / 4, E);
    atomicAdd(&stats[0], layers); atomicAdd(&stats[1], E);
    if (count > 0) atomicMin(&stats[2], fewest);
  }
  __syncthreads();
  if (w < count) {
    const int sl = first + w, pool_at = mir_pool_at(mw, count, c16) / 4;
    int e = cnt[w];
    for (int k = 0; k < mw[w].m; k++) {
      int addr = mir_lane_addr(slice_off, colidx, first, mw, w, k, lane, lo, hi, c16);
      const unsigned long long miss = __ballot(addr < 0);
      if (addr < 0) {
        const int idx = e + __popcll(miss & ((1ULL << lane) - 1ULL));
        pool_src[(size_t)b * kMirPoolMax + idx] = (slice_off[sl] + mw[w].a + k) * 9 * 64 + lane;
        addr = pool_at + (idx >> 6) * 9 * 64 + (idx & 63);
      }
      e += __popcll(miss);
      addr_out[((size_t)sl * kMirMax + k) * 64 + lane] = (unsigned short)addr;
    }
  }
  if (w < kMirWaves && lane == 0)
    wave_out[(size_t)b * kMirWaves + w] = w < count ? make_int4(mw[w].a | mw[w].m << 8 | mw[w].p << 16, mw[w].at, mw[w].tab, mir_reg_slots(mw[w], regs)) : make_int4(0, 0, 0, 0);
}

// One wavefront's share of the collection of all workgroups' posted sums of sequence number `sums`: lane `l0` of `stride` takes workgroups
// l0, l0 + stride, ...; adds their two values to t0s / t1s in that order (the callers fix the order of the rest).  Bounded by the wall clock.
// SERVE_PRIO (the service wavefront of a PRIO = 3 kernel, which enters at priority 1): a record that is not there yet is polled at priority 0.
template <bool SERVE_PRIO = false>
__device__ __forceinline__ void pipe_collect_posts(const PipeArgs& pa, unsigned int sums, int nb, int lane, int stride, int l0, long long t0, long long t_limit, bool& failed,
                                                   double& t0s, double& t1s) {
  const unsigned long long* post = pa.post + (size_t)(sums & 1u) * nb * 4;
  for (int b = l0; b - lane < nb && !failed; b += stride) {  // wave-uniform trip count
    const bool mine = b < nb;
    uint4 q4[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    for (;;) {
      bool ok = true;
      if (mine) {  // the record's four granules in two 16-byte requests (each granule is one 8-byte store of its writer)
        asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(q4[0]), "=&v"(q4[1]) : "v"(post + (size_t)b * 4) : "memory");
        ok = q4[0].y == sums && q4[0].w == sums && q4[1].y == sums && q4[1].w == sums;
      }
      if (__ballot(!ok) == 0ULL) break;
      if constexpr (SERVE_PRIO) pipe_setprio<0>();  // from here on a spin
      if (ld_sc1_u32(pa.error) != 0u || wall_clock64() - t0 > t_limit) { failed = true; break; }
      __builtin_amdgcn_s_sleep(1);
    }
    if constexpr (SERVE_PRIO) pipe_setprio<1>();
    if (mine && !failed) {
      t0s += __longlong_as_double((long long)(((unsigned long long)q4[0].x << 32) | (unsigned long long)q4[0].z));
      t1s += __longlong_as_double((long long)(((unsigned long long)q4[1].x << 32) | (unsigned long long)q4[1].z));
    }
  }
}

// How many cache lines the gathers of a slot touch, planes against node-by-node storage of the gathered vector (sampled: every `step`-th
// slice, all its slots; a wavefront per slot).  out[0] += distinct 128-byte lines of one plane (x 3 planes = the lines a slot fetches),
// out[1] += distinct lines of the 24-byte records, out[2] += 1.
__global__ __launch_bounds__(256) void k_gather_lines(int n_slices, int step, const int* __restrict__ slice_off, const int* __restrict__ colidx,
                                                      unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_waves = (int)((gridDim.x * blockDim.x) >> 6);
  unsigned long long planes = 0, records = 0, slots = 0;
  for (int s = wave * step; s < n_slices; s += n_waves * step) {
    for (int slot = slice_off[s]; slot < slice_off[s + 1]; slot++) {
      const unsigned int col = (unsigned int)colidx[(size_t)slot * 64 + lane];
      const unsigned int kp = col >> 4, k0 = (col * 24u) >> 7, k1 = (col * 24u + 23u) >> 7;
      bool first_p = true, first_0 = true, first_1 = k1 != k0;
      for (int l = 0; l < 64; l++) {  // (is there an earlier lane with the same line?)
        const unsigned int op = __builtin_amdgcn_readlane(kp, l), o0 = __builtin_amdgcn_readlane(k0, l), o1 = __builtin_amdgcn_readlane(k1, l);
        if (l < lane) {
          first_p = first_p && op != kp;
          first_0 = first_0 && o0 != k0 && o1 != k0;
          first_1 = first_1 && o0 != k1 && o1 != k1;
        }
      }
      planes += __popcll(__ballot(first_p));
      records += __popcll(__ballot(first_0)) + __popcll(__ballot(first_1));
      slots++;
    }
  }
  if (lane == 0 && slots) { atomicAdd(out, planes); atomicAdd(out + 1, records); atomicAdd(out + 2, slots); }
}

}  // namespace fb
#include "pcg_shard_box.hip.h"
namespace fb {

// the kernel itself: pcg_pipe_kernel.h, once as it always was and once with register slots
}  // namespace fb
#define FB_PIPE_KERNEL k_pcg_pipe
#define FB_PIPE_KERNEL_ATTR
#define FB_PIPE_KERNEL_HOLDS false
#include "pcg_pipe_kernel.h"
#undef FB_PIPE_KERNEL
#undef FB_PIPE_KERNEL_ATTR
#undef FB_PIPE_KERNEL_HOLDS
#define FB_PIPE_KERNEL k_pcg_pipe_regs
#define FB_PIPE_KERNEL_ATTR __attribute__((amdgpu_num_vgpr(FB_PIPE_REGS_VGPR_PAIRS)))
#define FB_PIPE_KERNEL_HOLDS true
#include "pcg_pipe_kernel.h"
#undef FB_PIPE_KERNEL
#undef FB_PIPE_KERNEL_ATTR
#undef FB_PIPE_KERNEL_HOLDS
