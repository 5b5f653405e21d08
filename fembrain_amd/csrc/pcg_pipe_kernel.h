// The kernel of pcg_pipe.hip.h, which includes this text TWICE: as k_pcg_pipe (REGS = 0: every instantiation there was before the register slots,
// unchanged) and as k_pcg_pipe_regs (REGS = 2 or 3), the same template under a function attribute that a template parameter cannot set: the
// compiler is held to 138 vector registers there (amdgpu_num_vgpr counts in pairs on this architecture), and the 30 above them, which the
// workgroup's 168-register allocation contains anyway, keep matrix values for the launch (pcg_pipe_regs.hip.h).  No include guard.
//   FB_PIPE_KERNEL        the kernel's name
//   FB_PIPE_KERNEL_ATTR   its function attribute, or nothing
//   FB_PIPE_KERNEL_HOLDS  true: the instantiations with REGS > 0, false: those with REGS = 0
namespace fb {

// WMAX: wavefronts per workgroup the instantiation is bounded for (512 registers per lane and SIMD are shared by
// ceil(WMAX / 4) wavefronts).  LDS-resident part of the matrix: the first slots of every slice (9 values + the column id per lane)
// are loaded into LDS ONCE per launch -- the matrix does not change during a solve; slots beyond are streamed every product as in
// k_spmv.  The CU's LDS holds pipe_lds_slots() = 62 / 65 wavefront-slots beside the sync buffers; a workgroup deals them
// to its `count` live wavefronts, count-th part each and the remainder one more for the first ones (11 slices: 5 slots each and a
// sixth for seven of them; 10 slices: 6 each), at most KLT per wavefront (the unroll bound of the LDS loop).
// The product's schedule in the LDS-window instantiations (WMAX = 12, KLT = 6 or 7: kMir below), all in slot order: the low part of the diagonal
// block (C++), the slots in front of the window streamed (pcg_pipe_stream.hip.h: loads 13..25 deep), the ON-CHIP RUN -- mirror layers, then
// plain LDS layers -- hand-scheduled with the gathers four slots ahead (pcg_pipe_onchip.hip.h; the C++ loop it replaced waited for each slot's
// three gathers in turn: 4.1-4.6 of the product's 10 us at 1M tets, profiles/r07_onchip_phase_before.txt), the slots behind the window
// streamed.  Every other instantiation keeps the C++ loop over its LDS slots.
// TIMING: the development build with per-phase clocks (FEMBRAIN_PERSIST_TIMING=1); in the LDS-window instantiations the product phase is
// also clocked at its two seams (first streamed part | on-chip run | second streamed part).
// SHARD: the kernel of a sharded handle (pcg_shard_box.hip.h; "k_pcg_pipe_shard<WMAX,KLT>" in fb_fem_pcg_path): the slices come from the
// plan's deal (sa.wg_range), the last wavefront is the spare one (sums, counters, proxy copies), rows a neighbour rank gathers are also
// stored into its box, the sums go through the rank level; 32-bit column words, write-through stores.  sa is not read otherwise.
// BJ (FB_PCG_BLOCK_JACOBI, opt-in and not part of the reference): the preconditioner is the inverse of the row's 3x3 diagonal block
// instead of 1/diag -- `invdiag` then points at 9 doubles per row (symmetric: 6 are loaded).  The Jacobi instantiations do not change.
// HELP: the instantiation with helper wavefronts (PipeArgs::tasks).  A template parameter, not a run-time test: with the helpers' second
// copy of the streamed product compiled in, the kernel of the headline mesh -- which has none -- ran 3 % slower (16.2 against 15.7 us per
// iteration on one box, tools/ab_r4 in round 5); with HELP = false nothing of it is there.
// AHEAD: the run-ahead form of a launch with a service wavefront (header, "Run-ahead form"); the host picks it per launch (fem_persist.hip), so
// the instantiations without it are what they were.
// REGS (2 or 3; 0: none): up to that many streamed slots of every slice, those next to the LDS window, keep their values in registers above the compiler's cap for the launch and
// run with the on-chip run (pcg_pipe_regs.hip.h; how many a slice has is the plan's word, PipeArgs::mirror).  Only for the run-ahead LDS-window
// instantiations; the temporaries of the hand-written loops are then v64..v99, which is what leaves the registers.
// PRIO (0: none, and nothing of it in the kernel; 1 progress, 2 static, 3 progress + service wavefront): wavefront priority through the product
// (header of pcg_pipe.hip.h, "Priority 0 before every wait").  The register-slot kernels and the TIMING (12, 6) run-ahead kernel only.
template <typename MT, bool C16, int WMAX, int KLT, bool TIMING, bool SHARD, bool BJ = false, bool HELP = false, bool XYZ = false, bool AHEAD = false, int REGS = 0,
          int PRIO = 0>
__global__ __launch_bounds__(64 * WMAX) FB_PIPE_KERNEL_ATTR void FB_PIPE_KERNEL(SellView sv, const MT* __restrict__ vals, const MT* __restrict__ dlo,
                                                        const double* __restrict__ invdiag, const double* __restrict__ bvec, double* __restrict__ xg,
                                                        double* __restrict__ rg, double* __restrict__ wg, double* __restrict__ zg,
                                                        double* __restrict__ sg, double* __restrict__ pg, CGState* __restrict__ st, PipeArgs pa,
                                                        ShardArgs sa) {
  static_assert(!SHARD || (!C16 && !TIMING), "a shard's columns are 32-bit local ids; the phase clocks are built for the unsharded kernel");
  static_assert(!BJ || (!SHARD && !TIMING), "block-Jacobi is for unsharded handles");
  static_assert(!HELP || (!SHARD && !BJ), "helper wavefronts: unsharded handles, the Jacobi preconditioner");
  static_assert(!AHEAD || (!SHARD && !HELP), "run-ahead: unsharded handles without helper wavefronts (add_helpers needs the barrier)");
  static_assert((REGS > 0) == FB_PIPE_KERNEL_HOLDS, "register slots: k_pcg_pipe_regs, and only there");
  static_assert(REGS == 0 || (AHEAD && !TIMING && !BJ && !XYZ && WMAX == 12 && (KLT == 6 || KLT == 7) && REGS <= kPipeRegsMax),
                "register slots: the run-ahead LDS-window instantiations");
  static_assert(PRIO >= 0 && PRIO <= 3 && (PRIO == 0 || (AHEAD && !BJ && !XYZ && WMAX == 12 && (REGS > 0 || (TIMING && KLT == 6)))),
                "wavefront priority: the register-slot kernels and the TIMING (12, 6) run-ahead kernel");
  constexpr bool kProgress = PRIO == 1 || PRIO == 3;
  static_assert(sizeof(MT) == 4, "k_pcg_pipe keeps part of the matrix in LDS as fp32 words and streams the rest as fp32");
  extern __shared__ double lds[];  // the request is padded so that one workgroup fills a CU
  double* wsum = lds;                          // [2][16] wave sums
  double* gath = lds + 32;                     // [2][kPipeMaxBlocks] all workgroups' sums
  double* bc = gath + 2 * kPipeMaxBlocks;      // [0..1] totals, [2] a wait failed (sweep), [3] a wait failed (product), [4] a sum poller gave up
  unsigned int* const tot_seq = (unsigned int*)(bc + 6);  // (AHEAD) the `sums` number whose totals bc[0..2] hold, released by the service wavefront
  const int n_waves = blockDim.x >> 6, nb = gridDim.x;
  if (pa.start == 0 && st->done) return;  // grid-uniform: written by an earlier launch
  if (threadIdx.x == 0) bc[4] = 0.0;      // set by a sum poller that gave up (read after the next barrier)
  if constexpr (AHEAD) {
    if (threadIdx.x == 0) *tot_seq = pa.seqs[1];  // no totals of this launch yet (the first product's barriers lie before the first wait for them)
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int first, count;
  if constexpr (SHARD) { first = sa.wg_range[blockIdx.x].x; count = sa.wg_range[blockIdx.x].y; }
  else pipe_deal(pa.wg_first, sv.n_slices, nb, blockIdx.x, &first, &count);
  const bool spare = SHARD && wv == n_waves - 1;  // a shard's spare wavefront: sums, counters, proxy copies (it owns no slice)
  const bool live = wv < count && !spare;         // wave-uniform
  const int sl = first + wv;
  const int row = sl * 64 + lane;
  const bool rvalid = live && row < sv.n_owned;
  const size_t dof = 3 * (size_t)(rvalid ? row : 0);
  int so = 0, width = 0;
  if (live) { so = sv.slice_off[sl]; width = sv.slice_off[sl + 1] - so; }
  so = __builtin_amdgcn_readfirstlane(so); width = __builtin_amdgcn_readfirstlane(width);  // wave-uniform: scalar registers
  const MT* v = vals + (size_t)so * 9 * 64 + lane;
  const int* ci = sv.colidx + (size_t)so * 64 + lane;
  const short* cd = C16 ? sv.coldelta + (size_t)so * 64 + lane : nullptr;
  // low part of the diagonal block (symmetric: 6 planes) and 1/diag, fixed for the solve
  MT m00 = 0, m01 = 0, m02 = 0, m11 = 0, m12 = 0, m22 = 0;
  double iv[BJ ? 6 : 3] = {0};  // 1/diag, or (BJ) the inverse diagonal block: 00 01 02 11 12 22
  int send_beg = 0, send_end = 0;  // (SHARD) this row's entries of the send lists
  if (rvalid) {
    const MT* l = dlo + (size_t)sl * 9 * 64 + lane;
    m00 = l[0 * 64]; m01 = l[1 * 64]; m02 = l[2 * 64]; m11 = l[4 * 64]; m12 = l[5 * 64]; m22 = l[8 * 64];
    if constexpr (BJ) {
      const double* B = invdiag + 3 * dof;
      iv[0] = B[0]; iv[1] = B[1]; iv[2] = B[2]; iv[3] = B[4]; iv[4] = B[5]; iv[5] = B[8];
    } else {
#pragma unroll
      for (int a = 0; a < 3; a++) iv[a] = invdiag[dof + a];
    }
    if constexpr (SHARD) { send_beg = sa.row_send_off[row]; send_end = sa.row_send_off[row + 1]; }
  }
  // LDS-resident part of the matrix: the first KL slots of this wave's slice, [klt_w][10][64] words (9 values + the column id)
  // (HELP: how many and where is the plan's decision, PipeArgs::tasks -- a slice of 27 slots among slices of 15 keeps 17 of them here, so
  // that every wavefront of the workgroup streams about the same number: an iteration ends with the slowest wavefront)
  int klt_w, lres_at;
  // the LDS window (PipeArgs::mirror, pcg_pipe_mirror.h): slots [mir_a, mir_a + mir_m) are read from LDS as the transposes of other rows'
  // blocks, [kp, kp + klt_w) are the plain resident ones, the rest is streamed.  Without a window: kp = 0, the first klt_w slots.
  constexpr bool kMir = !HELP && !SHARD && !BJ && !XYZ && WMAX == 12 && (KLT == 6 || KLT == 7);
  int mir_a = 0, mir_m = 0, mir_tab = 0;
  int reg_r = 0;  // (REGS) register slots of this slice
  if constexpr (HELP) {
    const int4 tk = pa.tasks[(size_t)blockIdx.x * kPipeTaskStride + wv];
    klt_w = __builtin_amdgcn_readfirstlane(live ? tk.x : 0);
    lres_at = __builtin_amdgcn_readfirstlane(live ? tk.y : 0);
  } else {
    constexpr int kSlots = pipe_lds_slots(C16);
    const int lbase = min(KLT, kSlots / max(count, 1)), lrem = lbase < KLT ? min(count, kSlots - lbase * count) : 0;  // workgroup-uniform
    klt_w = __builtin_amdgcn_readfirstlane(live ? lbase + (wv < lrem ? 1 : 0) : 0);
    lres_at = wv * lbase + min(wv, lrem);
    if constexpr (kMir) {
      if (pa.mirror) {
        const int4 mt = live ? pa.mirror[(size_t)blockIdx.x * kPipeMaxWaves + wv] : make_int4(0, 0, 0, 0);
        klt_w = __builtin_amdgcn_readfirstlane((mt.x >> 16) & 0xff);
        lres_at = __builtin_amdgcn_readfirstlane(mt.y);
        mir_a = __builtin_amdgcn_readfirstlane(mt.x & 0xff);
        mir_m = __builtin_amdgcn_readfirstlane((mt.x >> 8) & 0xff);
        mir_tab = __builtin_amdgcn_readfirstlane(mt.z);
        if constexpr (REGS > 0) reg_r = __builtin_amdgcn_readfirstlane(min(mt.w, REGS));
      }
    }
  }
  const int kp = mir_a + mir_m, k_after = kp + klt_w;  // first plain slot, first slot streamed after the window
  const int KL = min(klt_w, width - kp);
  // the register slots (pcg_pipe_regs.hip.h): reg_b behind the window, [k_after, k_behind), the others in front of it, [n_front, mir_a); filled here,
  // at the head of every launch.  Without REGS: n_front = mir_a, k_behind = k_after.
  const int reg_b = REGS > 0 ? min(reg_r, max(width - k_after, 0)) : 0, reg_f = REGS > 0 ? min(reg_r - reg_b, mir_a) : 0;
  const int n_front = mir_a - reg_f, k_behind = k_after + reg_b;
  auto reg_slot = [&](int q) { return q < reg_f ? so + n_front + q : so + k_after + (q - reg_f); };  // register layer q's slot of the matrix
  if constexpr (REGS > 0) {
    const int reg_n = reg_f + reg_b;
    auto voff = [&](int q) { return ((unsigned int)reg_slot(q) * 9u * 64u + (unsigned int)lane) * (unsigned int)sizeof(float); };
    auto goff = [&](int q) -> unsigned int {  // the column's byte offset in a plane, as the loops form it from the column word
      if (q >= reg_n) return 0u;
      const size_t at = (size_t)reg_slot(q) * 64 + lane;
      return (C16 ? (unsigned int)(row + (int)sv.coldelta[at]) : (unsigned int)sv.colidx[at]) << 3;
    };
    pipe_regs_fill(reg_n, voff(0), voff(1), voff(2), goff(0), goff(1), goff(2), (const float*)vals);
  }
  // this wavefront's part: C16 [klt_w][9][64] value words, then [klt_w][64] column differences (halfwords); else [klt_w][10][64] words, the tenth the column
  constexpr int kValWords = C16 ? 9 : 10;
  char* lwave = (char*)(lds + kPipeSyncDoubles) + (size_t)lres_at * pipe_slot_bytes(C16);
  unsigned int* lres = (unsigned int*)lwave + lane;
  short* lcd = (short*)(lwave + (size_t)klt_w * 9 * 256) + lane;  // (C16)
  auto lds_col = [&](int k) -> unsigned int {
    if constexpr (C16) return (unsigned int)(row + (int)lcd[k * 64]);
    else return lres[(k * 10 + 9) * 64];
  };
  if (sizeof(MT) == 4) {
    for (int k = 0; k < KL; k++) {
      const MT* vk = v + (size_t)(kp + k) * 9 * 64;
#pragma unroll
      for (int j = 0; j < 9; j++) lres[(k * kValWords + j) * 64] = __float_as_uint((float)vk[j * 64]);
      if constexpr (C16) lcd[k * 64] = cd[(size_t)(kp + k) * 64];
      else lres[(k * 10 + 9) * 64] = (unsigned int)ci[(size_t)(kp + k) * 64];
    }
  }
  if constexpr (kMir) {
    if (pa.mirror) {
      // the mirror tables: per lane and layer the column and the LDS word of the block to read transposed
      unsigned int* lmt = (unsigned int*)((char*)(lds + kPipeSyncDoubles) + mir_tab) + lane;
      const unsigned short* ma = pa.mir_addr + (size_t)(live ? sl : 0) * kMirMax * 64 + lane;
      for (int k = 0; k < mir_m; k++) {
        const unsigned int addr = ma[k * 64];
        if constexpr (C16) lmt[k * 64] = addr << 16 | (unsigned short)cd[(size_t)(mir_a + k) * 64];
        else { lmt[k * 96] = (unsigned int)ci[(size_t)(mir_a + k) * 64]; ((unsigned short*)(lmt - lane + k * 96 + 64))[lane] = (unsigned short)addr; }
      }
      // the pool: blocks whose transposes are not resident elsewhere, stored transposed (value 3a + b of the block at word (3b + a) x 64)
      const int2 pw = pa.mir_wg[blockIdx.x];
      unsigned int* lmat = (unsigned int*)(lds + kPipeSyncDoubles);
      for (int e = threadIdx.x; e < pw.y; e += blockDim.x) {
        const MT* src = vals + pa.mir_pool[(size_t)blockIdx.x * kMirPoolMax + e];
        unsigned int* pe = lmat + pw.x + (e >> 6) * 9 * 64 + (e & 63);
#pragma unroll
        for (int j = 0; j < 9; j++) pe[(3 * (j % 3) + j / 3) * 64] = __float_as_uint((float)src[j * 64]);
      }
    }
  }
  // this wavefront's task (helpers, see PipeArgs): the owner of a slice streams its slots up to own_k1 and adds the partial sums of the
  // helpers in help_mask; a helper streams [hk0, hk1) of slice help_sl for the rows of that slice
  // (every value below is wave-uniform and made so explicitly, outside any branch: scalar registers.  Without HELP they are constants and the
  // kernel is the round-4 one.)
  double* ypart = (double*)((char*)(lds + kPipeSyncDoubles) + (size_t)(pipe_lds_slots(C16) - pipe_help_slots(C16)) * pipe_slot_bytes(C16));  // [helper][3][64]
  int own_k1 = width, help_sl = -1, hk0 = 0, hk1 = 0, help_idx = 0, help_so = 0;
  unsigned int help_mask = 0u;
  if constexpr (HELP) {
    const int4 tk = pa.tasks[(size_t)blockIdx.x * kPipeTaskStride + wv];
    const bool helper = !live && !spare && tk.x >= 0;
    own_k1 = __builtin_amdgcn_readfirstlane(live ? tk.z : width);
    help_mask = (unsigned int)__builtin_amdgcn_readfirstlane(live ? tk.w : 0);
    help_sl = __builtin_amdgcn_readfirstlane(helper ? first + tk.x : -1);
    hk0 = __builtin_amdgcn_readfirstlane(helper ? tk.y : 0); hk1 = __builtin_amdgcn_readfirstlane(helper ? tk.z : 0);
    help_idx = __builtin_amdgcn_readfirstlane(helper ? tk.w : 0);
    help_so = __builtin_amdgcn_readfirstlane(sv.slice_off[help_sl < 0 ? 0 : help_sl]);
  }
  // the producers of this workgroup's columns: one per lane of wavefront 0
  const int n_prod = pa.prod_count[blockIdx.x];
  int my_prod = -1;
  if (wv == 0 && n_prod >= 0 && lane < n_prod) my_prod = pa.producers[(size_t)blockIdx.x * kPipeMaxProducers + lane];

  unsigned int send_mask = 0u;  // (SHARD) workgroup-uniform: the ranks this workgroup has rows to send to
  ShardBoxLayout BL = {};
  if constexpr (SHARD) { send_mask = sa.wg_send_mask[blockIdx.x]; BL = shard_box_layout(sa.halo_cap); }
  unsigned int pub = pa.seqs[0], sums = pa.seqs[1];  // grid-uniform: written by the previous launch
  const long long t_limit = pa.timeout_ticks;
  bool failed = false;
  long long tm[TIMING ? 7 : 1] = {0}, tprev = TIMING ? wall_clock64() : 0;  // (TIMING: the phase clocks cost 14 registers per lane)
  // (TIMING) tm[5], tm[6]: of the product phase, the first streamed part and the on-chip run; the rest of tm[2] is the second streamed part
  auto seam = [&](int k, long long& t) { if (TIMING) { const long long u = wall_clock64(); tm[k] += u - t; t = u; } };
  auto lap = [&](int k) { if (TIMING) { const long long t = wall_clock64(); tm[k] += t - tprev; tprev = t; } };

  // Stores of the next product's input vector into the plane buffer of the next publish number (512 contiguous bytes per wave
  // and plane).  Write-through (sc1) where a workgroup of ANOTHER XCD gathers these rows; a workgroup all of whose consumers
  // share its XCD (= its L2) may store plainly (pa.plain_local): the line then stays in that L2, the store is acknowledged
  // there, and the consumers -- their L1 invalidated -- read it from there.  Which workgroups share an XCD is NOT the launch's to
  // promise (blockIdx & 7 is the observed round-robin deal, good for speed only; a CU-masked stream deals otherwise): every
  // workgroup announces the XCC id the hardware reports, its first publish of a launch goes through, and it stores plainly from
  // the second on only if all its producers (= its consumers: A is symmetric) announced the same id (checked in product()).
  const bool plain_cand = !SHARD && pa.plain_local != 0 && pa.prod_xcd[blockIdx.x] == 0;  // workgroup-uniform
  bool through = true, xcc_known = false;
  unsigned int my_xcc = 0u;
  if constexpr (!SHARD) {
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(my_xcc));
    if (threadIdx.x == 0) st_sc1_u32(pa.xcc + blockIdx.x, ((pub + 1u) << 4) | my_xcc);  // (visible before this workgroup's first flag: product() drains before it flags)
  }
  // XYZ: the published vector lies node by node (x, y, z side by side) instead of in three planes -- for irregular meshes, whose gathers
  // of a slot touch 64 different cache lines per plane: one line per lane instead of three (pcg_pipe_stream.hip.h).  606k-tet Delaunay
  // probe 18.6 -> 16.4 us per iteration; the cube after a cut, whose columns are mostly consecutive, 19.4 -> 20.6 (each of the three loads
  // of a slot then touches 12 lines instead of 4), so setup_persist decides from the columns (k_gather_lines).
  static_assert(!XYZ || HELP, "the node-by-node vector comes with the table-driven instantiation");
  const size_t xs = XYZ ? 1 : pa.n_pad, cs = XYZ ? 3 : 1;  // strides of a component and of a column in the published vector
  auto publish = [&](const double* vin) {
    pub++;
    double* pl = pa.planes + (size_t)(pub & 1u) * 3 * pa.n_pad;
    if (rvalid) {
      if (XYZ && through) {
        st_sc1_xyz(pl + 3 * (size_t)row, vin[0], vin[1], vin[2]);
      } else if (through) {
#pragma unroll
        for (int a = 0; a < 3; a++) st_sc1_f64(pl + a * xs + cs * (size_t)row, vin[a]);
      } else {
#pragma unroll
        for (int a = 0; a < 3; a++) pl[a * xs + cs * (size_t)row] = vin[a];
      }
      if constexpr (SHARD) shard_send_row(sa, BL, pub, send_beg, send_end, vin);
    }
  };
  // y = A vin for the vector published last: drain the stores, flag, wait for the producers of this workgroup's columns,
  // multiply.  post_sums: the two wave sums in wsum[.][wv] are this iteration's local parts of gamma and delta -- posted with
  // the flag, read after the product.
  auto product = [&](const double* vin, double* y, bool post_sums, bool late_acquire) {
    double* pl = pa.planes + (size_t)(pub & 1u) * 3 * pa.n_pad;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    lap(0);  // publish, drained
    if (post_sums) sums++;
    if (REGS == 0 && wv != 0 && live && pa.prefetch_slots > 0 && (mir_a > 0 || own_k1 > k_after)) {
      // idle until wavefront 0 has seen the neighbours' flags: the first streamed slots' values go to L2 meanwhile (measured at 1M
      // tets, us per iteration with 0 / 2 / 3 / 4 slots: 17.15 / 16.25 / 16.1 / 16.05; the same during the drain of the publish
      // stores instead delays the flag and loses: 16.85).  With an LDS window: those of the first streamed part, [0, mir_a).
      int so_k = so + (mir_a > 0 ? 0 : k_after);
      asm volatile("" : "+s"(so_k));  // (opaque, as for the streamed loop below)
      pipe_prefetch_values(min(pa.prefetch_slots, mir_a > 0 ? mir_a : own_k1 - k_after), ((unsigned int)so_k * 9u * 64u + (unsigned int)lane) * (unsigned int)sizeof(float), vals);
    }
    if constexpr (REGS > 0) {  // the same with register slots: what is still streamed, [0, n_front) or from k_behind on -- never a register slot
      if (wv != 0 && live && pa.prefetch_slots > 0 && (n_front > 0 || own_k1 > k_behind)) {
        int so_k = so + (n_front > 0 ? 0 : k_behind);
        asm volatile("" : "+s"(so_k));
        pipe_prefetch_values_low(min(pa.prefetch_slots, n_front > 0 ? n_front : own_k1 - k_behind), ((unsigned int)so_k * 9u * 64u + (unsigned int)lane) * (unsigned int)sizeof(float), vals);
      }
    }
    if constexpr (SHARD) {
      if (spare) shard_service_product(sa, BL, pa, pub, pl, nb, lane, send_mask, t_limit, bc, failed);
    }
    if (wv == 0) {
      if (lane == 0) st_sc1_u32(pa.flags + blockIdx.x, pub);
      if (post_sums && lane < 2) {  // workgroup sums in wave order, posted as two tagged halves each
        double t = 0.0;
        for (int w = 0; w < n_waves; w++) t += wsum[lane * 16 + w];
        const unsigned long long bits = (unsigned long long)__double_as_longlong(t), tag = (unsigned long long)sums << 32;
        unsigned long long* post = pa.post + ((size_t)(sums & 1u) * nb + blockIdx.x) * 4 + 2 * lane;
        st_sc1_u64(post, (bits >> 32) | tag);
        st_sc1_u64(post + 1, (bits & 0xffffffffULL) | tag);
      }
      // Every wave of this workgroup is past its last gather from the buffer published now (two products ago) and none loads
      // from the planes before the barrier below: drop this CU's L1 lines NOW (asynchronous), the poll runs meanwhile.  That early
      // form rests on the sums: every workgroup has posted this iteration's sums, i.e. finished the product before the previous one, so
      // no CU of this XCD pulls a line of this buffer's previous contents into the shared L2 any more.  Products that do not follow a
      // sums sweep (the first of a launch, the exact-residual pair, the iteration after them) have no such guarantee about a sibling
      // CU two products behind -- they take the guide's order, acquire AFTER the poll.
      if (!late_acquire) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const long long t0 = wall_clock64();
      if (n_prod >= 0) {
        for (;;) {
          bool ok = true;
          if (my_prod >= 0) ok = (int)(ld_sc1_u32(pa.flags + my_prod) - pub) >= 0;
          if (__ballot(!ok) == 0ULL) break;
          if (ld_sc1_u32(pa.error) != 0u || wall_clock64() - t0 > t_limit) { failed = true; break; }
          __builtin_amdgcn_s_sleep(1);
        }
      } else if constexpr (SHARD) {
        shard_poll_all(sa, pa, pub, nb, lane, t0, t_limit, failed);
      } else {
        for (int b = 4 * lane; b - 4 * lane < nb && !failed; b += 256) {  // four flags per lane in one 16-byte request
          for (;;) {
            bool ok = true;
            if (b < nb) {
              const uint4 f = ld_sc1_u128(pa.flags + b);
              ok = (int)(f.x - pub) >= 0 && (b + 1 >= nb || (int)(f.y - pub) >= 0) && (b + 2 >= nb || (int)(f.z - pub) >= 0) && (b + 3 >= nb || (int)(f.w - pub) >= 0);
            }
            if (__ballot(!ok) == 0ULL) break;
            if (ld_sc1_u32(pa.error) != 0u || wall_clock64() - t0 > t_limit) { failed = true; break; }
            __builtin_amdgcn_s_sleep(1);
          }
        }
      }
      if (failed && lane == 0) st_sc1_u32(pa.error, 1u);
      if (late_acquire) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      if (plain_cand && !xcc_known && !failed) {  // first product of the launch: the producers' flags are in, so are their XCC ids
        const bool same = my_prod < 0 || ld_sc1_u32(pa.xcc + my_prod) == ((pub << 4) | my_xcc);
        const bool all_same = __ballot(!same) == 0ULL;
        if (lane == 0) bc[5] = all_same ? 1.0 : 0.0;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) bc[3] = (failed || ld_sc1_u32(pa.error) != 0u) ? 1.0 : 0.0;  // one lane decides for the whole workgroup
    }
    __syncthreads();
    lap(1);  // flag + wait for the producers + acquire
    if (uniform_flag(bc[3] != 0.0 || (SHARD && bc[4] != 0.0))) { failed = true; return; }
    if (plain_cand && !xcc_known) { through = !uniform_flag(bc[5] != 0.0); xcc_known = true; }
    // (PRIO) behind the second barrier: a slice wavefront starts its product at 3 (progress), the youngest of every SIMD runs it at 1 (static)
    if constexpr (kProgress) { if (uniform_flag(live)) pipe_setprio<3>(); }
    if constexpr (PRIO == 2) { if (uniform_flag(live && wv >= 8)) pipe_setprio<1>(); }
    // the low part of the diagonal block times the own entry first: vin is not needed beyond this point
    double y0 = 0, y1 = 0, y2 = 0;
    if (rvalid) {
      MT u00 = m00, u01 = m01, u02 = m02, u11 = m11, u12 = m12, u22 = m22;  // kept in storage type: without the (empty) asm the
      asm volatile("" : "+v"(u00), "+v"(u01), "+v"(u02), "+v"(u11), "+v"(u12), "+v"(u22));  // compiler hoists the conversions and keeps 12 registers
      const double l00 = (double)u00, l01 = (double)u01, l02 = (double)u02, l11 = (double)u11, l12 = (double)u12, l22 = (double)u22;
      y0 = l00 * vin[0] + l01 * vin[1] + l02 * vin[2];
      y1 = l01 * vin[0] + l11 * vin[1] + l12 * vin[2];
      y2 = l02 * vin[0] + l12 * vin[1] + l22 * vin[2];
    }
    long long tseam = tprev;
    if (live) {
      if constexpr (kMir) {
        // the LDS window in slot order: the slots in front of it streamed, then the mirror layers (the same mul / mul / add / mul / add / add
        // per row as everywhere: the sum of a row runs over the same slots in the same order with the same values as without a window)
        if (REGS == 0 && mir_a > 0) {
          int so_k = so;
          asm volatile("" : "+s"(so_k));  // (opaque, as below)
          pipe_stream_slots<C16, XYZ>(mir_a, ((unsigned int)so_k * 9u * 64u + (unsigned int)lane) * (unsigned int)sizeof(float),
                                      ((unsigned int)so_k * 64u + (unsigned int)lane) * (unsigned int)(C16 ? sizeof(short) : sizeof(int)), vals,
                                      C16 ? (const void*)sv.coldelta : (const void*)sv.colidx, pl, pl + xs, pl + 2 * xs, row, y0, y1, y2);
        }
        if constexpr (REGS > 0) {  // (register slots: what is left of it, over the low temporaries)
          if (n_front > 0) {
            int so_k = so;
            asm volatile("" : "+s"(so_k));
            pipe_stream_slots_low<C16>(n_front, ((unsigned int)so_k * 9u * 64u + (unsigned int)lane) * (unsigned int)sizeof(float),
                                       ((unsigned int)so_k * 64u + (unsigned int)lane) * (unsigned int)(C16 ? sizeof(short) : sizeof(int)), vals,
                                       C16 ? (const void*)sv.coldelta : (const void*)sv.colidx, pl, pl + xs, pl + 2 * xs, row, y0, y1, y2);
          }
        }
        if constexpr (kProgress) pipe_setprio<2>();  // the seam into the on-chip run
        seam(5, tseam);
        // the on-chip run, m mirror layers and then KL plain ones: hand-scheduled, the gathers four slots ahead (pcg_pipe_onchip.hip.h)
        const char* lbase = (const char*)(lds + kPipeSyncDoubles);
        if constexpr (REGS > 0) {  // ... with the register layers at both ends of it (pcg_pipe_regs.hip.h)
          pipe_onchip_slots_regs<C16, kProgress>(reg_f, mir_m, max(KL, 0), reg_b, (const unsigned int*)(lbase + mir_tab) + lane, (const unsigned short*)(lbase + mir_tab) + lane, lres, lcd,
                                      lbase, pl, pl + xs, pl + 2 * xs, row, y0, y1, y2);
        } else
        pipe_onchip_slots<C16, kProgress>(mir_m, max(KL, 0), (const unsigned int*)(lbase + mir_tab) + lane, (const unsigned short*)(lbase + mir_tab) + lane, lres, lcd, lbase, pl, pl + xs,
                               pl + 2 * xs, row, y0, y1, y2);
        if constexpr (kProgress) pipe_setprio<0>();  // the seam into the streamed rest (a run that ended in register layers is there already)
      }
      if (sizeof(MT) == 4 && KLT >= 16) {
        // whole slices in LDS, five wavefronts per CU: registers to spare, so ALL gathers of the product are in flight before the first
        // multiplication (the loop below waits for each slot's three gathers in turn: 5.5 us for the slowest wavefronts at 105k tets, whose
        // columns come from another XCD's rows, against 2.2 on average -- profiles/r05_small_mesh_phase_table.txt)
        double gx[KLT][3];
#pragma unroll
        for (int k = 0; k < KLT; k++) {
          const unsigned int col = k < KL ? lds_col(k) : 0u;
          const double* xp = pl + cs * (size_t)col;
          gx[k][0] = k < KL ? xp[0] : 0.0; gx[k][1] = k < KL ? xp[xs] : 0.0; gx[k][2] = k < KL ? xp[2 * xs] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < KLT; k++) if (k < KL) {
          const unsigned int* lk = lres + (size_t)k * kValWords * 64;
          const double x0 = gx[k][0], x1 = gx[k][1], x2 = gx[k][2];
          y0 += (double)__uint_as_float(lk[0 * 64]) * x0 + (double)__uint_as_float(lk[1 * 64]) * x1 + (double)__uint_as_float(lk[2 * 64]) * x2;
          y1 += (double)__uint_as_float(lk[3 * 64]) * x0 + (double)__uint_as_float(lk[4 * 64]) * x1 + (double)__uint_as_float(lk[5 * 64]) * x2;
          y2 += (double)__uint_as_float(lk[6 * 64]) * x0 + (double)__uint_as_float(lk[7 * 64]) * x1 + (double)__uint_as_float(lk[8 * 64]) * x2;
        }
      } else if (sizeof(MT) == 4 && !kMir) {
#pragma unroll
        for (int k = 0; k < KLT; k++) if (k < KL) {  // LDS-resident slots
          const unsigned int* lk = lres + (size_t)k * kValWords * 64;
          const double* xp = pl + cs * (size_t)lds_col(k);
          const double x0 = xp[0], x1 = xp[xs], x2 = xp[2 * xs];
          y0 += (double)__uint_as_float(lk[0 * 64]) * x0 + (double)__uint_as_float(lk[1 * 64]) * x1 + (double)__uint_as_float(lk[2 * 64]) * x2;
          y1 += (double)__uint_as_float(lk[3 * 64]) * x0 + (double)__uint_as_float(lk[4 * 64]) * x1 + (double)__uint_as_float(lk[5 * 64]) * x2;
          y2 += (double)__uint_as_float(lk[6 * 64]) * x0 + (double)__uint_as_float(lk[7 * 64]) * x1 + (double)__uint_as_float(lk[8 * 64]) * x2;
        }
        if constexpr (HELP) {  // (a wide slice's share may be longer than the unroll bound: further groups of KLT, the gathers of a group in flight together)
          for (int kb = KLT; kb < KL; kb += KLT) {
            double gx[KLT][3];
#pragma unroll
            for (int j = 0; j < KLT; j++) {
              const int k = min(kb + j, KL - 1);  // (past the end: the last slot again, not used)
              const double* xp = pl + cs * (size_t)lds_col(k);
              gx[j][0] = xp[0]; gx[j][1] = xp[xs]; gx[j][2] = xp[2 * xs];
            }
#pragma unroll
            for (int j = 0; j < KLT; j++) if (kb + j < KL) {
              const unsigned int* lk = lres + (size_t)(kb + j) * kValWords * 64;
              const double x0 = gx[j][0], x1 = gx[j][1], x2 = gx[j][2];
              y0 += (double)__uint_as_float(lk[0 * 64]) * x0 + (double)__uint_as_float(lk[1 * 64]) * x1 + (double)__uint_as_float(lk[2 * 64]) * x2;
              y1 += (double)__uint_as_float(lk[3 * 64]) * x0 + (double)__uint_as_float(lk[4 * 64]) * x1 + (double)__uint_as_float(lk[5 * 64]) * x2;
              y2 += (double)__uint_as_float(lk[6 * 64]) * x0 + (double)__uint_as_float(lk[7 * 64]) * x1 + (double)__uint_as_float(lk[8 * 64]) * x2;
            }
          }
        }
      }
      if constexpr (kMir) {
        if (TIMING) asm volatile("" : "+v"(y0), "+v"(y1), "+v"(y2));  // (the clock is read behind the sums, not beside them)
        seam(6, tseam);
      }
      // the streamed slots: hand-pipelined loads (pcg_pipe_stream.hip.h); those from own_k1 on are a helper's
      const int n_str = own_k1 - k_after;
      if (REGS == 0 && n_str > 0) {
        int so_k = so + k_after;
        asm volatile("" : "+s"(so_k));  // opaque: keeps the two offsets below from being hoisted out of the solver loop into live registers
        pipe_stream_slots<C16, XYZ>(n_str, ((unsigned int)so_k * 9u * 64u + (unsigned int)lane) * (unsigned int)sizeof(float),
                               ((unsigned int)so_k * 64u + (unsigned int)lane) * (unsigned int)(C16 ? sizeof(short) : sizeof(int)), vals,
                               C16 ? (const void*)sv.coldelta : (const void*)sv.colidx, pl, pl + xs, pl + 2 * xs, row, y0, y1, y2);
      }
      if constexpr (REGS > 0) {  // (register slots: from k_behind on, over the low temporaries)
        if (own_k1 > k_behind) {
          int so_k = so + k_behind;
          asm volatile("" : "+s"(so_k));
          pipe_stream_slots_low<C16>(own_k1 - k_behind, ((unsigned int)so_k * 9u * 64u + (unsigned int)lane) * (unsigned int)sizeof(float),
                                     ((unsigned int)so_k * 64u + (unsigned int)lane) * (unsigned int)(C16 ? sizeof(short) : sizeof(int)), vals,
                                     C16 ? (const void*)sv.coldelta : (const void*)sv.colidx, pl, pl + xs, pl + 2 * xs, row, y0, y1, y2);
        }
      }
    }
    if constexpr (HELP) if (help_sl >= 0) {  // a helper: its share of another wavefront's slice, handed over through LDS (the owner adds it after the next barrier)
      double h0 = 0, h1 = 0, h2 = 0;
      int so_k = help_so + hk0;
      asm volatile("" : "+s"(so_k));
      if (hk1 > hk0)  // (the stream loads its first slots unconditionally: never with none)
      pipe_stream_slots<C16, XYZ>(hk1 - hk0, ((unsigned int)so_k * 9u * 64u + (unsigned int)lane) * (unsigned int)sizeof(float),
                             ((unsigned int)so_k * 64u + (unsigned int)lane) * (unsigned int)(C16 ? sizeof(short) : sizeof(int)), vals,
                             C16 ? (const void*)sv.coldelta : (const void*)sv.colidx, pl, pl + xs, pl + 2 * xs, help_sl * 64 + lane, h0, h1, h2);
      double* hp = ypart + (size_t)help_idx * 3 * 64 + lane;
      hp[0] = h0; hp[64] = h1; hp[128] = h2;
    }
    if constexpr (PRIO != 0) pipe_setprio<0>();  // every wavefront, whatever it held: what follows are waits, recurrences and exits
    y[0] = y0; y[1] = y1; y[2] = y2;
    lap(2);  // product
  };
  // the helpers' partial sums of this wavefront's slice, in the order of their numbers (after a workgroup barrier that follows the product)
  auto add_helpers = [&](double* y) {
    unsigned int m = help_mask;
    while (m) {
      const int hi = __ffs((int)m) - 1;
      m &= m - 1u;
      const double* hp = ypart + (size_t)hi * 3 * 64 + lane;
      y[0] += hp[0]; y[1] += hp[64]; y[2] += hp[128];
    }
  };

  // this row's vectors stay here for the whole solve
  double xr[3] = {0, 0, 0}, rr[3] = {0, 0, 0}, wr[3] = {0, 0, 0}, zr[3] = {0, 0, 0}, sr[3] = {0, 0, 0}, pr[3] = {0, 0, 0};
  double rho0 = 0.0, eps2 = pa.eps2, gamma_old = 1.0, alpha_old = 1.0;
  int iter = 0, max_iter = pa.max_iter;
  // One product per trip of the loop below (ONE copy of the product's code): what is multiplied and what becomes of the result
  // depends on the phase.  WARM_X / REFRESH_X: y = A x, r = b - y (CGSolver.cpp:131-136 / :159-166); INIT_W / REFRESH_W:
  // w = A (r / diag); ITER: an iteration.
  enum { PH_WARM_X = 0, PH_INIT_W = 1, PH_ITER = 2, PH_REFRESH_X = 3, PH_REFRESH_W = 4 };
  int phase = PH_ITER;
  bool fresh = pa.start != 0;  // the next iteration is the first of a solve (beta = 0)
  if (pa.start == 0) {
    if (rvalid) {
#pragma unroll
      for (int a = 0; a < 3; a++) { xr[a] = xg[dof + a]; rr[a] = rg[dof + a]; wr[a] = wg[dof + a]; zr[a] = zg[dof + a]; sr[a] = sg[dof + a]; pr[a] = pg[dof + a]; }
    }
    rho0 = uniform_f64(st->rho0); eps2 = uniform_f64(st->eps2); iter = st->iter; max_iter = st->max_iter;
    gamma_old = uniform_f64(pa.pstate[0]); alpha_old = uniform_f64(pa.pstate[1]);
  } else if (pa.start == 2) {
    if (rvalid) {
#pragma unroll
      for (int a = 0; a < 3; a++) xr[a] = xg[dof + a];
    }
    phase = PH_WARM_X;
  } else {
    if (rvalid) {  // x = 0: r = b
#pragma unroll
      for (int a = 0; a < 3; a++) rr[a] = bvec[dof + a];
    }
    phase = PH_INIT_W;
  }

  // out = M^-1 v: v / diag, or (BJ) the inverse diagonal block times v
  auto precond = [&](const double* vv, double* out) {
    if constexpr (BJ) {
      out[0] = iv[0] * vv[0] + iv[1] * vv[1] + iv[2] * vv[2];
      out[1] = iv[1] * vv[0] + iv[3] * vv[1] + iv[4] * vv[2];
      out[2] = iv[2] * vv[0] + iv[4] * vv[1] + iv[5] * vv[2];
    } else {
#pragma unroll
      for (int a = 0; a < 3; a++) out[a] = iv[a] * vv[a];
    }
  };
  bool done = false, published = false;  // published: the stores of the next product's input are on their way already
  bool unsettled = true;                 // the next product does not follow a sums sweep of this launch: acquire after the poll
  double gamma = 0.0;
  int it_done = 0;
  while (!failed) {
    if (phase == PH_ITER && it_done >= pa.n_iters) break;  // a launch is cut between iterations only
    double vin[3];
    if (phase == PH_WARM_X || phase == PH_REFRESH_X) {
#pragma unroll
      for (int a = 0; a < 3; a++) vin[a] = xr[a];
    } else if (phase == PH_ITER) {
      precond(wr, vin);  // m = w / diag
    } else {
      precond(rr, vin);
    }
    if (!published) publish(vin);
    published = false;
    if (phase == PH_ITER) {
      // local parts of gamma = r . u and delta = w . u (u = r / diag), while the stores drain
      double u[3];
      precond(rr, u);
      double a0 = rr[0] * u[0] + rr[1] * u[1] + rr[2] * u[2];
      double a1 = wr[0] * u[0] + wr[1] * u[1] + wr[2] * u[2];
      a0 = wave_sum(a0); a1 = wave_sum(a1);
      int wvo = wv;
      asm volatile("" : "+v"(wvo));  // opaque: the LDS address is formed here instead of living in a register through the solve
      if (lane == 0) { wsum[wvo] = a0; wsum[16 + wvo] = a1; }
    }
    double y[3];
    product(vin, y, phase == PH_ITER, phase != PH_ITER || unsettled);
    unsettled = phase != PH_ITER;  // (an iteration's sums sweep settles the next product's early acquire)
    if (failed) break;
    if constexpr (HELP) if (phase != PH_ITER) {  // (an iteration's sweep of the sums has barriers of its own: the partial sums are added behind them)
      __syncthreads();
      add_helpers(y);
    }
    if (phase == PH_WARM_X || phase == PH_REFRESH_X) {
      unsigned int d3 = 3u * (unsigned int)(rvalid ? row : 0);
      asm volatile("" : "+v"(d3));  // opaque: the address of b is formed here, not kept in two registers through the whole solve
#pragma unroll
      for (int a = 0; a < 3; a++) rr[a] = rvalid ? bvec[d3 + a] - y[a] : 0.0;
      phase = phase == PH_WARM_X ? PH_INIT_W : PH_REFRESH_W;
      continue;
    }
    if (phase != PH_ITER) {
#pragma unroll
      for (int a = 0; a < 3; a++) wr[a] = y[a];
      phase = PH_ITER;
      continue;
    }
    // ---- all workgroups' sums (posted before their products: they are there) ----
    if constexpr (SHARD) {
      if (spare) shard_rank_sums(sa, BL, pa, sums, nb, lane, t_limit, bc, failed);
      __syncthreads();
    } else if (AHEAD || pa.service) {
      // A workgroup with a wavefront to spare (fewer slices than the instantiation's wavefronts) has its LAST wavefront -- no
      // slice, it idles through the product -- collect the sums meanwhile: same order of additions as below, so the same bits;
      // the others find the totals behind ONE barrier, or (AHEAD, the header's run-ahead form) each behind its own wait for their number.
      if (wv == n_waves - 1) {
        if constexpr (PRIO == 3) pipe_setprio<1>();  // the youngest wavefront of its SIMD: its collection at 1, a poll of a missing record at 0, 0 behind the hand-over
        const long long t0 = wall_clock64();
        double t0s = 0, t1s = 0;
        pipe_collect_posts<PRIO == 3>(pa, sums, nb, lane, 64, lane, t0, t_limit, failed, t0s, t1s);
        failed = uniform_flag(failed);
        if (failed && lane == 0) st_sc1_u32(pa.error, 1u);
        t0s = wave_sum(t0s); t1s = wave_sum(t1s);
        if (lane == 0) {
          bc[0] = t0s; bc[1] = t1s; bc[2] = (failed || ld_sc1_u32(pa.error) != 0u) ? 1.0 : 0.0;
          if constexpr (AHEAD) __hip_atomic_store(tot_seq, sums, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);  // totals or failure: always handed over
        }
        if constexpr (PRIO == 3) pipe_setprio<0>();
      }
      if constexpr (AHEAD) {
        while ((unsigned int)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(tot_seq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) != sums) __builtin_amdgcn_s_sleep(1);
      } else {
        __syncthreads();
      }
    } else {
      const int pollers = min(n_waves, 4);
      if (wv < pollers) {
        const long long t0 = wall_clock64();
        const unsigned long long* post = pa.post + (size_t)(sums & 1u) * nb * 4;
        for (int b = wv * 64 + lane; b - lane < nb && !failed; b += pollers * 64) {  // wave-uniform trip count
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
            if (ld_sc1_u32(pa.error) != 0u || wall_clock64() - t0 > t_limit) { failed = true; break; }
            __builtin_amdgcn_s_sleep(1);
          }
          if (mine && !failed) {
            gath[b] = __longlong_as_double((long long)(((unsigned long long)q4[0].x << 32) | (unsigned long long)q4[0].z));
            gath[kPipeMaxBlocks + b] = __longlong_as_double((long long)(((unsigned long long)q4[1].x << 32) | (unsigned long long)q4[1].z));
          }
        }
        if (failed && lane == 0) { st_sc1_u32(pa.error, 1u); bc[4] = 1.0; }
      }
      __syncthreads();
      if (wv == 0) {  // fixed order: lane l adds workgroups l, l + 64, ...; then the wave tree -- the same bits in every workgroup
        double t0s = 0, t1s = 0;
        int l0 = lane;
        asm volatile("" : "+v"(l0));  // (opaque, as above)
        for (int b = l0; b < nb; b += 64) { t0s += gath[b]; t1s += gath[kPipeMaxBlocks + b]; }
        t0s = wave_sum(t0s); t1s = wave_sum(t1s);
        if (lane == 0) { bc[0] = t0s; bc[1] = t1s; bc[2] = (bc[4] != 0.0 || ld_sc1_u32(pa.error) != 0u) ? 1.0 : 0.0; }
      }
      __syncthreads();
    }
    lap(3);  // sweep of the sums (AHEAD: this wavefront's own wait for the totals)
    if (uniform_flag(bc[2] != 0.0)) { failed = true; break; }  // a wait timed out somewhere: every workgroup leaves within one phase
    if constexpr (HELP) add_helpers(y);  // (every path of the sweep ends in a workgroup barrier: the helpers' sums of this product are in LDS)
    gamma = uniform_f64(bc[0]);
    const double delta = uniform_f64(bc[1]);
    if (fresh) rho0 = gamma;
    // the while-condition of CGSolver.cpp:147 at the head of the iteration; gamma is bitwise the same in every workgroup
    if (!(gamma > eps2 * rho0) || iter >= max_iter) { done = true; break; }
    double alpha, beta;
    if (fresh) { beta = 0.0; alpha = gamma / delta; }
    else { beta = gamma / gamma_old; alpha = gamma / (delta - beta * gamma / alpha_old); }
    fresh = false;
    // ---- recurrences, in registers (y = n = A m) ----
    iter++;
    it_done++;
    gamma_old = gamma; alpha_old = alpha;
    const bool refresh = iter % 30 == 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      zr[a] = y[a] + beta * zr[a];
      sr[a] = wr[a] + beta * sr[a];
    }
    if (!refresh) {
      // w first: the next product's input m = w / diag leaves now, the rest of the recurrences runs while its stores drain.
      // (Every workgroup has posted this iteration's sums, i.e. finished the product before this one: the buffer is free.)
      double m[3];
#pragma unroll
      for (int a = 0; a < 3; a++) wr[a] = wr[a] - alpha * zr[a];
      precond(wr, m);
      publish(m);
      published = true;
    }
    if constexpr (BJ) {
      double ur[3];
      precond(rr, ur);
#pragma unroll
      for (int a = 0; a < 3; a++) pr[a] = ur[a] + beta * pr[a];
    } else {
#pragma unroll
      for (int a = 0; a < 3; a++) pr[a] = iv[a] * rr[a] + beta * pr[a];
    }
#pragma unroll
    for (int a = 0; a < 3; a++) xr[a] = xr[a] + alpha * pr[a];
    if (refresh) {
      phase = PH_REFRESH_X;  // exact residual (CGSolver.cpp:159-166), and the w that goes with it: two more products
    } else {
#pragma unroll
      for (int a = 0; a < 3; a++) rr[a] = rr[a] - alpha * sr[a];
    }
    lap(4);  // recurrences
  }
  if (TIMING && lane == 0) {
    unsigned long long* tw = (unsigned long long*)pa.timing + ((size_t)blockIdx.x * kPipeMaxWaves + wv) * kPipeTimingSlots;
    for (int k = 0; k < 5; k++) atomicAdd(tw + k, (unsigned long long)tm[k]);
    atomicAdd(tw + 5, (unsigned long long)it_done);
    atomicAdd(tw + 6, (unsigned long long)tm[5]); atomicAdd(tw + 7, (unsigned long long)tm[6]);
  }
  if (failed) return;  // nothing written back: the host re-solves from the vectors it handed over
  // The iteration cap ended the solve: x is left in pg and the start vector stays -- the host checks the iterate's true residual and
  // either takes it or has the two-launch solver repeat the solve from the same start (pcg_solve_pipe)
  const bool capped = done && gamma > eps2 * rho0;
  if (rvalid) {
    unsigned int dof = 3u * (unsigned int)row;
    asm volatile("" : "+v"(dof));  // (formed here: see the exact-residual phase)
    if (capped) {
#pragma unroll
      for (int a = 0; a < 3; a++) pg[dof + a] = xr[a];
    } else {
#pragma unroll
      for (int a = 0; a < 3; a++) xg[dof + a] = xr[a];
      if (!done) {  // the launch was cut (test knob): the next one continues from here
#pragma unroll
        for (int a = 0; a < 3; a++) { rg[dof + a] = rr[a]; wg[dof + a] = wr[a]; zg[dof + a] = zr[a]; sg[dof + a] = sr[a]; pg[dof + a] = pr[a]; }
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->rho0 = rho0; st->eps2 = eps2; st->max_iter = max_iter;
    st->iter = iter;
    st->rho[iter & 1] = done ? gamma : gamma_old;  // what the host's convergence test reads (CGSolver.cpp:189)
    st->done = done ? 1 : 0;
    pa.pstate[0] = gamma_old; pa.pstate[1] = alpha_old;
    // (a shard's launch cut after a pre-publish takes the publish back: its rows are in the planes and the boxes, but no counter was raised
    // for it, and the next launch publishes the same values under the same number)
    pa.seqs[0] = (SHARD && published) ? pub - 1u : pub; pa.seqs[1] = sums;
  }
}


}  // namespace fb
