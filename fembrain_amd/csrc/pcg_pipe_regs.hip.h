// Register slots of k_pcg_pipe's LDS-window instantiations (k_pcg_pipe_regs, the REGS template parameter: 2 or 3): up to REGS streamed slot layers
// of a slice whose nine fp32 values per lane -- and the lane's gather offset of the layer's column -- stay in REGISTERS for a whole launch instead
// of being streamed in every product.
//
// Why there is room.  A 12-wavefront workgroup allocates 168 vector registers per lane (occupancy 3) whatever it uses.  The solver's state and
// the 36 temporaries of the hand-written loops need 138 when the temporaries sit low (v64..v99: pcg_pipe_temps.h with FBP_TEMPS_LOW); at
// v120..v155 the compiler reports 168 only because the highest temporary is v155.  So the kernel is compiled under a cap of 138 registers
// (pcg_pipe_kernel.h: a function attribute) and v138..v167 are this file's: 3 layers x (9 values + 1 offset), 84 KB per CU over 11 slices --
// half as much again as the LDS window.  (Accumulation registers were the first plan.  The vector ALU cannot read them as operands, and this
// compiler gives a kernel that names one HALF of its budget, 84 registers here, as vector registers: it then spills the solver's state into
// them.  Plain registers above a cap have neither problem.)
//
// Which slots.  Those next to the LDS window, so that the on-chip run (pcg_pipe_onchip.hip.h) only becomes longer and no pipeline is filled or
// drained for them: of a slice's window [a, a + m + p) and its r = min(REGS, streamed slots) register slots, nb = min(r, slots behind the window)
// follow the plain layers and nf = r - nb precede the mirror layers.  The product in slot order:
//     streamed [0, a - nf) | register [a - nf, a) | mirror [a, a + m) | plain [a + m, a + m + p) | register, nb of them | streamed, the rest
// Behind the window first: the cube's slices stream 2-3 slots there, and with them in registers the second stream -- its fill and its drain --
// mostly disappears.  A register layer in the four-gather-set rotation differs from a plain LDS layer in where its operands come from: the nine
// values are operands of the conversions where the plain layer has its ds_reads, and the gathers take their address register as it is.
// Arithmetic: FBP_ROW itself -- every row sum keeps its bits.
// Fill.  pipe_regs_fill at the head of EVERY launch: the matrix changes between solves and a solve may be cut into several launches.
// Safety.  The compiler cannot touch v138 and above under the cap (it calls them reserved, and says so once per fill -- the clobbers are there all
// the same: they are what makes the kernel's register count reach v167); these instantiations spill nothing, use no scratch and keep occupancy 3,
// and no operand from v138 on appears outside this file's text (profiles/r09_regs_kernel_registers.txt).  The operands of the run are as few as
// they are on purpose: the kernel sits at its cap, and two scalar operands more made the compiler spill 30 registers of solver state.
#pragma once
#include "pcg_pipe_onchip.hip.h"
// from here on the temporaries of the FBP_ / FBO_ text are v64..v99
#define FBP_TEMPS_LOW
#include "pcg_pipe_temps.h"

namespace fb {

constexpr int kPipeRegsMax = 3;      // register slots of a slice at most
constexpr int kPipeRegsFirst = 138;  // the first register of this file: v138..v164 the values, v165..v167 the gather offsets; the compiler's end below it
#define FB_PIPE_REGS_VGPR_PAIRS 69   // = kPipeRegsFirst / 2: amdgpu_num_vgpr counts the unified registers of gfx90a and later in pairs
static_assert(2 * FB_PIPE_REGS_VGPR_PAIRS == kPipeRegsFirst && kPipeRegsFirst + 10 * kPipeRegsMax == 168, "the register slots fill the allocation of occupancy 3");

// clang-format off
#define FBR_SET0 "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145", "v146"
#define FBR_SET1 "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155"
#define FBR_SET2 "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164"
#define FBR_OFF0 "v165"
#define FBR_OFF1 "v166"
#define FBR_OFF2 "v167"
// the nine values of a layer into its registers (FBP_LOADV's addresses), and its gather offset
#define FBR_FILL(off, r0, r1, r2, r3, r4, r5, r6, r7, r8)                  \
  "s_nop 4\n\t"                                                            \
  "global_load_dword " r0 ", %[voff], %[svals]\n\t"                        \
  "global_load_dword " r1 ", %[voff], %[svals] offset:256\n\t"             \
  "global_load_dword " r2 ", %[voff], %[svals] offset:512\n\t"             \
  "global_load_dword " r3 ", %[voff], %[svals] offset:768\n\t"             \
  "global_load_dword " r4 ", %[voff], %[svals] offset:1024\n\t"            \
  "global_load_dword " r5 ", %[voff], %[svals] offset:1280\n\t"            \
  "global_load_dword " r6 ", %[voff], %[svals] offset:1536\n\t"            \
  "global_load_dword " r7 ", %[voff], %[svals] offset:1792\n\t"            \
  "global_load_dword " r8 ", %[voff], %[svals] offset:2048\n\t"            \
  "v_mov_b32_e32 " off ", %[goff]\n\t"
#define FBR_FILL_(off, SET) FBR_FILL(off, SET)
// a register layer's block: FBP_ROW with the held values as its operands
#define FBR_COMPUTE(x0, x1, x2, r0, r1, r2, r3, r4, r5, r6, r7, r8)                                    \
  FBP_ROW("%[y0]", r0, r1, r2, x0, x1, x2)                                                             \
  FBP_ROW("%[y1]", r3, r4, r5, x0, x1, x2)                                                             \
  FBP_ROW("%[y2]", r6, r7, r8, x0, x1, x2)
#define FBR_COMPUTE_(x0, x1, x2, SET) FBR_COMPUTE(x0, x1, x2, SET)
#define FBR_GATHER(x0, x1, x2, off)                                        \
  "global_load_dwordx2 " x0 ", " off ", %[spl0]\n\t"                       \
  "global_load_dwordx2 " x1 ", " off ", %[spl1]\n\t"                       \
  "global_load_dwordx2 " x2 ", " off ", %[spl2]\n\t"
// register layer number q (0, 1, 2: the order of the fill; a scalar counter, Q2 = the text for layer 2 or nothing): TEXT0 / TEXT1 / TEXT2, then q + 1
#define FBR_BY_LAYER(T, J, q, TEXT0, TEXT1, TEXT2)                         \
  "s_cmp_lt_i32 " q ", 1\n\t"                                              \
  "s_cbranch_scc0 .Lfbr_" T "1" J "_%=\n\t"                                \
  TEXT0                                                                    \
  "s_branch .Lfbr_" T "d" J "_%=\n"                                        \
  ".Lfbr_" T "1" J "_%=:\n\t"                                              \
  "s_cmp_lt_i32 " q ", 2\n\t"                                              \
  "s_cbranch_scc0 .Lfbr_" T "2" J "_%=\n\t"                                \
  TEXT1                                                                    \
  "s_branch .Lfbr_" T "d" J "_%=\n"                                        \
  ".Lfbr_" T "2" J "_%=:\n\t"                                              \
  TEXT2                                                                    \
  ".Lfbr_" T "d" J "_%=:\n\t"                                              \
  "s_add_i32 " q ", " q ", 1\n\t"
#define FBR_COMPUTE_REG(J, x0, x1, x2) \
  FBR_BY_LAYER("q", J, "%[qc]", FBR_COMPUTE_(x0, x1, x2, FBR_SET0), FBR_COMPUTE_(x0, x1, x2, FBR_SET1), FBR_COMPUTE_(x0, x1, x2, FBR_SET2))
#define FBR_ISSUE_REG(J, x0, x1, x2) \
  FBR_BY_LAYER("g", J, "%[qi]", FBR_GATHER(x0, x1, x2, FBR_OFF0), FBR_GATHER(x0, x1, x2, FBR_OFF1), FBR_GATHER(x0, x1, x2, FBR_OFF2))
// the next layer not yet issued (ni of them left), into set J: fi register layers, mi mirror layers, pi plain layers, then register layers again
#define FBR_ISSUE(J, ISSUE_MIR, ISSUE_PLAIN, x0, x1, x2, A)                \
  "s_cmp_lt_i32 %[ni], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbr_id" J "_%=\n\t"                                    \
  "s_sub_i32 %[ni], %[ni], 1\n\t"                                          \
  "s_cmp_lt_i32 %[fi], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbr_im" J "_%=\n\t"                                    \
  "s_sub_i32 %[fi], %[fi], 1\n\t"                                          \
  "s_branch .Lfbr_ir" J "_%=\n"                                            \
  ".Lfbr_im" J "_%=:\n\t"                                                  \
  "s_cmp_lt_i32 %[mi], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbr_ip" J "_%=\n\t"                                    \
  ISSUE_MIR(x0, x1, x2, A)                                                 \
  "s_sub_i32 %[mi], %[mi], 1\n\t"                                          \
  "s_branch .Lfbr_ix" J "_%=\n"                                            \
  ".Lfbr_ip" J "_%=:\n\t"                                                  \
  "s_cmp_lt_i32 %[pi], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbr_ir" J "_%=\n\t"                                    \
  ISSUE_PLAIN(x0, x1, x2, A)                                               \
  "s_sub_i32 %[pi], %[pi], 1\n\t"                                          \
  "s_branch .Lfbr_ix" J "_%=\n"                                            \
  ".Lfbr_ir" J "_%=:\n\t"                                                  \
  FBR_ISSUE_REG(J, x0, x1, x2)                                             \
  ".Lfbr_ix" J "_%=:\n\t"                                                  \
  "s_add_i32 %[fl], %[fl], 1\n"                                            \
  ".Lfbr_id" J "_%=:\n\t"
// one slot from set J (nc left to compute: fc register layers, mc mirror layers, pc plain layers, then register layers), then the slot four behind it
// (priority by progress, FBR_BODYP: PP = the step at the head of a plain layer's path, as FBO_SLOTP's; BL / BACK = where a register layer BEHIND the
// window goes and the step in front of it -- "cr" and nothing without the form: the text of the parent's loop)
#define FBR_BACK_NONE(J)
#define FBR_BACK_PRIO(J) ".Lfbr_cb" J "_%=:\n\t" "s_setprio 0\n\t"
#define FBR_SLOTP(J, PP, BL, BACK, ISSUE_MIR, ISSUE_PLAIN, x0, x1, x2, A)  \
  "s_cmp_lt_i32 %[nc], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbr_end_%=\n\t"                                        \
  "s_sub_i32 %[nc], %[nc], 1\n\t"                                          \
  "s_sub_i32 %[fl], %[fl], 1\n\t"                                          \
  "s_cmp_lt_i32 %[fc], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbr_cm" J "_%=\n\t"                                    \
  "s_sub_i32 %[fc], %[fc], 1\n\t"                                          \
  "s_branch .Lfbr_cr" J "_%=\n"                                            \
  ".Lfbr_cm" J "_%=:\n\t"                                                  \
  "s_cmp_lt_i32 %[mc], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbr_cp" J "_%=\n\t"                                    \
  "s_sub_i32 %[mc], %[mc], 1\n\t"                                          \
  FBO_FIRST_MIR(A)                                                         \
  FBO_WAITVM("m" J)                                                        \
  FBO_COMPUTE_MIR(x0, x1, x2, A)                                           \
  "s_branch .Lfbr_ci" J "_%=\n"                                            \
  ".Lfbr_cp" J "_%=:\n\t"                                                  \
  "s_cmp_lt_i32 %[pc], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbr_" BL J "_%=\n\t"                                   \
  "s_sub_i32 %[pc], %[pc], 1\n\t"                                          \
  PP                                                                       \
  FBO_FIRST_PLAIN(A)                                                       \
  FBO_WAITVM("p" J)                                                        \
  FBO_COMPUTE_PLAIN(x0, x1, x2, A)                                         \
  "s_branch .Lfbr_ci" J "_%=\n"                                            \
  BACK(J)                                                                  \
  ".Lfbr_cr" J "_%=:\n\t"                                                  \
  FBO_WAITVM("r" J)                                                        \
  FBR_COMPUTE_REG(J, x0, x1, x2)                                           \
  ".Lfbr_ci" J "_%=:\n\t"                                                  \
  FBR_ISSUE(J, ISSUE_MIR, ISSUE_PLAIN, x0, x1, x2, A)
#define FBR_ISSUE_(J, ISSUE_MIR, ISSUE_PLAIN, SET) FBR_ISSUE(J, ISSUE_MIR, ISSUE_PLAIN, SET)
#define FBR_SLOT_(J, PP, BL, BACK, ISSUE_MIR, ISSUE_PLAIN, SET) FBR_SLOTP(J, PP, BL, BACK, ISSUE_MIR, ISSUE_PLAIN, SET)
// Priority by progress (round 10): the run is entered at priority 2 (register layers in front, mirror layers), steps to 1 at the head of the plain
// layers' path and to 0 in front of the register layers behind the window -- the same scalar instruction again for every layer of the kind, the
// run being one rotating loop (FBO_PRIO_PLAIN).  A kind without layers is stepped over with its path.
#define FBR_BODY(ISSUE_MIR, ISSUE_PLAIN) FBR_BODYP(ISSUE_MIR, ISSUE_PLAIN, "", "cr", FBR_BACK_NONE)
#define FBR_BODY_PRIO(ISSUE_MIR, ISSUE_PLAIN) FBR_BODYP(ISSUE_MIR, ISSUE_PLAIN, FBO_PRIO_PLAIN, "cb", FBR_BACK_PRIO)
#define FBR_BODYP(ISSUE_MIR, ISSUE_PLAIN, PP, BL, BACK)                                                         \
  /* scalar operands fresh from v_readfirstlane, read by vector memory instructions: 5 wait states (see FBP_BODYG) */ \
  "s_nop 4\n\t"                                                                                                 \
  "s_mov_b32 %[fl], 0\n\t"                                                                                      \
  "s_mov_b32 %[qc], 0\n\t"                                                                                      \
  "s_mov_b32 %[qi], 0\n\t"                                                                                      \
  /* prologue: the first four slots' gathers (fewer: what there is) */                                          \
  FBR_ISSUE_("a", ISSUE_MIR, ISSUE_PLAIN, FBO_SET0)                                                             \
  FBR_ISSUE_("b", ISSUE_MIR, ISSUE_PLAIN, FBO_SET1)                                                             \
  FBR_ISSUE_("c", ISSUE_MIR, ISSUE_PLAIN, FBO_SET2)                                                             \
  FBR_ISSUE_("d", ISSUE_MIR, ISSUE_PLAIN, FBO_SET3)                                                             \
  ".Lfbr_loop_%=:\n\t"                                                                                          \
  FBR_SLOT_("0", PP, BL, BACK, ISSUE_MIR, ISSUE_PLAIN, FBO_SET0)                                                \
  FBR_SLOT_("1", PP, BL, BACK, ISSUE_MIR, ISSUE_PLAIN, FBO_SET1)                                                \
  FBR_SLOT_("2", PP, BL, BACK, ISSUE_MIR, ISSUE_PLAIN, FBO_SET2)                                                \
  FBR_SLOT_("3", PP, BL, BACK, ISSUE_MIR, ISSUE_PLAIN, FBO_SET3)                                                \
  "s_branch .Lfbr_loop_%=\n"                                                                                    \
  ".Lfbr_end_%=:\n\t"
// clang-format on

// The fill: register layer q (0 <= q < r <= 3, wave-uniform) = the nine values at byte offset voff_q (the lane's, from `vals`) and goff_q, the byte
// offset of the layer's column in a plane of the gathered vector; waited for.  All lanes active.  The clobbers are what makes the kernel's
// register count include these registers -- all 30, whatever r is.
__device__ __forceinline__ void pipe_regs_fill(int r, unsigned int voff0, unsigned int voff1, unsigned int voff2, unsigned int goff0, unsigned int goff1,
                                               unsigned int goff2, const float* vals) {
  vals = scalar_ptr(vals);
  r = __builtin_amdgcn_readfirstlane(r);
  if (r > 0) asm volatile(FBR_FILL_(FBR_OFF0, FBR_SET0) : : [voff] "v"(voff0), [goff] "v"(goff0), [svals] "s"(vals) : "memory", FBR_OFF0, FBR_SET0);
  if (r > 1) asm volatile(FBR_FILL_(FBR_OFF1, FBR_SET1) : : [voff] "v"(voff1), [goff] "v"(goff1), [svals] "s"(vals) : "memory", FBR_OFF1, FBR_SET1);
  if (r > 2) asm volatile(FBR_FILL_(FBR_OFF2, FBR_SET2) : : [voff] "v"(voff2), [goff] "v"(goff2), [svals] "s"(vals) : "memory", FBR_OFF2, FBR_SET2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// pipe_prefetch_values and pipe_stream_slots (planes) over the low temporaries: the same text, expanded here
__device__ __forceinline__ void pipe_prefetch_values_low(int n, unsigned int voff, const float* vals) {
  vals = scalar_ptr(vals);
  n = __builtin_amdgcn_readfirstlane(n);
  asm volatile("s_nop 4\n\t"
               "s_cmp_lt_i32 %[n], 1\n\t"
               "s_cbranch_scc1 .Lfbp_pf_end_%=\n\t"
               FBP_LOADV(FBV_120, FBV_121, FBV_122, FBV_123, FBV_124, FBV_125, FBV_126, FBV_127, FBV_128)
               "s_cmp_lt_i32 %[n], 2\n\t"
               "s_cbranch_scc1 .Lfbp_pf_wait_%=\n\t"
               FBP_LOADV(FBV_129, FBV_130, FBV_131, FBV_132, FBV_133, FBV_134, FBV_135, FBV_136, FBV_137)
               "s_cmp_lt_i32 %[n], 3\n\t"
               "s_cbranch_scc1 .Lfbp_pf_wait_%=\n\t"
               FBP_LOADV(FBV_138, FBV_139, FBV_140, FBV_141, FBV_142, FBV_143, FBV_144, FBV_145, FBV_146)
               "s_cmp_lt_i32 %[n], 4\n\t"
               "s_cbranch_scc1 .Lfbp_pf_wait_%=\n\t"
               FBP_LOADV(FBV_147, FBV_148, FBV_149, FBV_150, FBV_151, FBV_152, FBV_153, FBV_154, FBV_155)
               ".Lfbp_pf_wait_%=:\n\t"
               "s_waitcnt vmcnt(0)\n"
               ".Lfbp_pf_end_%=:\n\t"
               : [voff] "+v"(voff)
               : [n] "s"(n), [svals] "s"(vals)
               : FBP_CLOBBERS);
}

template <bool C16>
__device__ __forceinline__ void pipe_stream_slots_low(int n, unsigned int voff, unsigned int coff, const float* vals, const void* cols, const double* pl0,
                                                      const double* pl1, const double* pl2, int row, double& y0, double& y1, double& y2) {
  vals = scalar_ptr(vals); cols = scalar_ptr(cols); pl0 = scalar_ptr(pl0); pl1 = scalar_ptr(pl1); pl2 = scalar_ptr(pl2);
  n = __builtin_amdgcn_readfirstlane(n);
  if (C16) {
    asm volatile(FBP_BODY(FBP_LOADC16, FBP_GOFF16)
                 : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [voff] "+v"(voff), [coff] "+v"(coff), [n] "+s"(n)
                 : [svals] "s"(vals), [scols] "s"(cols), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2), [row] "v"(row)
                 : FBP_CLOBBERS);
  } else {
    asm volatile(FBP_BODY(FBP_LOADC32, FBP_GOFF32)
                 : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [voff] "+v"(voff), [coff] "+v"(coff), [n] "+s"(n)
                 : [svals] "s"(vals), [scols] "s"(cols), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2), [row] "v"(row)
                 : FBP_CLOBBERS);
  }
}

// The on-chip run with register layers: nf register layers, m mirror layers, kl plain layers, nb register layers (all wave-uniform, any may be 0;
// nf + nb <= 3), accumulated into y0, y1, y2 in that order.  The register layers are numbered in that order, as pipe_regs_fill filled them.
// The rest as pipe_onchip_slots.
// PRIO: with the priority steps of FBR_BODY_PRIO (the caller enters at priority 2 and sets 0 behind the run whatever it held).
template <bool C16, bool PRIO = false>
__device__ __forceinline__ void pipe_onchip_slots_regs(int nf, int m, int kl, int nb, const void* lmt, const void* lmt2, const void* lres, const void* lcd,
                                                       const void* lmat, const double* pl0, const double* pl1, const double* pl2, int row, double& y0, double& y1,
                                                       double& y2) {
  pl0 = scalar_ptr(pl0); pl1 = scalar_ptr(pl1); pl2 = scalar_ptr(pl2);
  int fi = __builtin_amdgcn_readfirstlane(nf), mi = __builtin_amdgcn_readfirstlane(m), pi = __builtin_amdgcn_readfirstlane(kl);
  int ni = fi + mi + pi + __builtin_amdgcn_readfirstlane(nb), fc = fi, mc = mi, pc = pi, nc = ni, fl, qc, qi;
  const unsigned int almat = __builtin_amdgcn_readfirstlane(lds_byte_address(lmat));
  unsigned int almt = lds_byte_address(lmt), ares = lds_byte_address(lres);
  if constexpr (C16) {
    unsigned int acd = lds_byte_address(lcd);
    if constexpr (PRIO)
      asm volatile(FBR_BODY_PRIO(FBO_ISSUE_MIR16, FBO_ISSUE_PLAIN16)
                   : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [lmt] "+v"(almt), [lres] "+v"(ares), [lcd] "+v"(acd), [fi] "+s"(fi), [mi] "+s"(mi), [pi] "+s"(pi),
                     [ni] "+s"(ni), [fc] "+s"(fc), [mc] "+s"(mc), [pc] "+s"(pc), [nc] "+s"(nc), [fl] "=&s"(fl), [qc] "=&s"(qc), [qi] "=&s"(qi)
                   : [lmat] "s"(almat), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2), [row] "v"(row)
                   : FBP_CLOBBERS);
    else
    asm volatile(FBR_BODY(FBO_ISSUE_MIR16, FBO_ISSUE_PLAIN16)
                 : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [lmt] "+v"(almt), [lres] "+v"(ares), [lcd] "+v"(acd), [fi] "+s"(fi), [mi] "+s"(mi), [pi] "+s"(pi),
                   [ni] "+s"(ni), [fc] "+s"(fc), [mc] "+s"(mc), [pc] "+s"(pc), [nc] "+s"(nc), [fl] "=&s"(fl), [qc] "=&s"(qc), [qi] "=&s"(qi)
                 : [lmat] "s"(almat), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2), [row] "v"(row)
                 : FBP_CLOBBERS);
  } else {
    unsigned int almt2 = lds_byte_address(lmt2);
    if constexpr (PRIO)
      asm volatile(FBR_BODY_PRIO(FBO_ISSUE_MIR32, FBO_ISSUE_PLAIN32)
                   : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [lmt] "+v"(almt), [lmt2] "+v"(almt2), [lres] "+v"(ares), [fi] "+s"(fi), [mi] "+s"(mi), [pi] "+s"(pi),
                     [ni] "+s"(ni), [fc] "+s"(fc), [mc] "+s"(mc), [pc] "+s"(pc), [nc] "+s"(nc), [fl] "=&s"(fl), [qc] "=&s"(qc), [qi] "=&s"(qi)
                   : [lmat] "s"(almat), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2)
                   : FBP_CLOBBERS);
    else
    asm volatile(FBR_BODY(FBO_ISSUE_MIR32, FBO_ISSUE_PLAIN32)
                 : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [lmt] "+v"(almt), [lmt2] "+v"(almt2), [lres] "+v"(ares), [fi] "+s"(fi), [mi] "+s"(mi), [pi] "+s"(pi),
                   [ni] "+s"(ni), [fc] "+s"(fc), [mc] "+s"(mc), [pc] "+s"(pc), [nc] "+s"(nc), [fl] "=&s"(fl), [qc] "=&s"(qc), [qi] "=&s"(qi)
                 : [lmat] "s"(almat), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2)
                 : FBP_CLOBBERS);
  }
}

}  // namespace fb
