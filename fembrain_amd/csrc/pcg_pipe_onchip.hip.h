// The on-chip run of a row product of k_pcg_pipe's LDS-window instantiations ((12, 6) and (12, 7)), written in gfx950 assembly:
// y += sum over "m mirror layers, then kl plain layers" of (3x3 fp32 block from LDS) x (gathered fp64 3-vector), lane = row, in slot order.
//
// Why assembly.  The compiler turns the C++ loops over these slots into one basic block per slot: column word from LDS, lgkmcnt(0), three
// gathers, vmcnt(2) / (1) / (0), 27 fp64 operations, branch -- nothing of slot k+1 is in flight while slot k waits, so a wavefront pays one
// exposed round trip to L2 or the Infinity Cache for each of its ~8.6 on-chip slots.  At the 168-register budget of a 12-wavefront
// workgroup there is no room for the compiler to do better (pcg_pipe_stream.hip.h has the same story for the streamed slots).  Here:
//   G(k+4) the three gathers of slot k+4                    issued when slot k has been computed (its registers are free then)
//   M(k)   27 fp64 operations of slot k, row by row         when G(k) has landed; three younger slots' gathers (9 loads) stay in flight
// Four gather sets (6 registers each) rotate; vector memory returns in order, so "G(k) has landed" is s_waitcnt vmcnt(3 x younger slots in
// flight): 9 in the middle of a run, 6 / 3 / 0 for the last slots (and for runs shorter than the pipeline) -- no load is issued past the run.
// The matrix values come from LDS one block row (3 words) at a time into the same three registers: the next row's ds_read is issued as soon as the
// conversions have consumed the previous words, so its latency runs under the row's remaining multiplications and additions.  A slot's first
// row is read before the wait for its gathers.  A mirror layer reads word (3b + a) x 64 of the partner's block where a plain layer reads word
// 3a + b of its own: only the offsets of the ds_reads differ.
// Arithmetic: FBP_ROW's sequence (cvt, cvt, mul, mul, add, cvt, mul, add, add) -- what the compiler emits for
//     y_a += (double)v[3a] * x0 + (double)v[3a+1] * x1 + (double)v[3a+2] * x2        (-ffp-contract=off)
// so the sums have the bits of the C++ loops they replace (tests/test_pipe_onchip_gpu.py holds them against recorded ones).
// Registers: the stream's 36 temporaries v120..v155 (FBP_CLOBBERS): v120-v123 the row's two fp64 temporaries (v122 also the byte offset of a
// gather, between rows), v124-v147 the four gather sets, v148-v151 the LDS byte address of each set's block, v152-v154 a block row's words.
#pragma once
#include "pcg_pipe_stream.hip.h"

namespace fb {

// clang-format off
// one block row: the words are in v152, v153, v154; NEXT_AB / NEXT_C read the next row's into them as soon as they are consumed
#define FBO_ROW(y, x0, x1, x2, NEXT_AB, NEXT_C)                            \
  "s_waitcnt lgkmcnt(0)\n\t"                                               \
  "v_cvt_f64_f32_e32 " FBV_120_121 ", " FBV_152 "\n\t"                                 \
  "v_cvt_f64_f32_e32 " FBV_122_123 ", " FBV_153 "\n\t"                                 \
  NEXT_AB                                                                  \
  "v_mul_f64 " FBV_120_121 ", " x0 ", " FBV_120_121 "\n\t"                           \
  "v_mul_f64 " FBV_122_123 ", " x1 ", " FBV_122_123 "\n\t"                           \
  "v_add_f64 " FBV_120_121 ", " FBV_120_121 ", " FBV_122_123 "\n\t"                       \
  "v_cvt_f64_f32_e32 " FBV_122_123 ", " FBV_154 "\n\t"                                 \
  NEXT_C                                                                   \
  "v_mul_f64 " FBV_122_123 ", " x2 ", " FBV_122_123 "\n\t"                           \
  "v_add_f64 " FBV_120_121 ", " FBV_120_121 ", " FBV_122_123 "\n\t"                       \
  "v_add_f64 " y ", " y ", " FBV_120_121 "\n\t"
// words o0, o1 (x 256 bytes) and o2 (bytes) of the block at LDS address A
#define FBO_READ_AB(A, o0, o1) "ds_read2st64_b32 " FBV_152_153 ", " A " offset0:" o0 " offset1:" o1 "\n\t"
#define FBO_READ_C(A, o2) "ds_read_b32 " FBV_154 ", " A " offset:" o2 "\n\t"
// a plain layer: row a of the block is words 3a, 3a + 1, 3a + 2
#define FBO_COMPUTE_PLAIN(x0, x1, x2, A)                                                               \
  FBO_ROW("%[y0]", x0, x1, x2, FBO_READ_AB(A, "3", "4"), FBO_READ_C(A, "1280"))                        \
  FBO_ROW("%[y1]", x0, x1, x2, FBO_READ_AB(A, "6", "7"), FBO_READ_C(A, "2048"))                        \
  FBO_ROW("%[y2]", x0, x1, x2,,)
#define FBO_FIRST_PLAIN(A) FBO_READ_AB(A, "0", "1") FBO_READ_C(A, "512")
// a mirror layer: row a of the block is words a, a + 3, a + 6 of the partner's (the transpose)
#define FBO_COMPUTE_MIR(x0, x1, x2, A)                                                                 \
  FBO_ROW("%[y0]", x0, x1, x2, FBO_READ_AB(A, "1", "4"), FBO_READ_C(A, "1792"))                        \
  FBO_ROW("%[y1]", x0, x1, x2, FBO_READ_AB(A, "2", "5"), FBO_READ_C(A, "2048"))                        \
  FBO_ROW("%[y2]", x0, x1, x2,,)
#define FBO_FIRST_MIR(A) FBO_READ_AB(A, "0", "3") FBO_READ_C(A, "1536")
#define FBO_GATHER(x0, x1, x2)                                             \
  "global_load_dwordx2 " x0 ", " FBV_122 ", %[spl0]\n\t"                          \
  "global_load_dwordx2 " x1 ", " FBV_122 ", %[spl1]\n\t"                          \
  "global_load_dwordx2 " x2 ", " FBV_122 ", %[spl2]\n\t"
// The next layer's column and block address, then its gathers.  16-bit columns: a mirror layer's table word is (LDS word of the block) << 16 |
// (column - row), a plain layer's column difference is a halfword behind the wavefront's values.  32-bit columns: the mirror table is 384 bytes
// per layer (64 columns, then 64 halfword addresses), a plain layer's column is the tenth word of its slot.
#define FBO_ISSUE_MIR16(x0, x1, x2, A)                                     \
  "ds_read_b32 " A ", %[lmt]\n\t"                                          \
  "v_add_u32_e32 %[lmt], 0x100, %[lmt]\n\t"                                \
  "s_waitcnt lgkmcnt(0)\n\t"                                               \
  "v_bfe_i32 " FBV_122 ", " A ", 0, 16\n\t"                                       \
  "v_add_u32_e32 " FBV_122 ", %[row], " FBV_122 "\n\t"                                   \
  "v_lshlrev_b32_e32 " FBV_122 ", 3, " FBV_122 "\n\t"                                    \
  FBO_GATHER(x0, x1, x2)                                                   \
  "v_lshrrev_b32_e32 " A ", 16, " A "\n\t"                                 \
  "v_lshl_add_u32 " A ", " A ", 2, %[lmat]\n\t"
#define FBO_ISSUE_PLAIN16(x0, x1, x2, A)                                   \
  "ds_read_i16 " FBV_122 ", %[lcd]\n\t"                                           \
  "v_add_u32_e32 %[lcd], 0x80, %[lcd]\n\t"                                 \
  "v_mov_b32_e32 " A ", %[lres]\n\t"                                       \
  "v_add_u32_e32 %[lres], 0x900, %[lres]\n\t"                              \
  "s_waitcnt lgkmcnt(0)\n\t"                                               \
  "v_add_u32_e32 " FBV_122 ", %[row], " FBV_122 "\n\t"                                   \
  "v_lshlrev_b32_e32 " FBV_122 ", 3, " FBV_122 "\n\t"                                    \
  FBO_GATHER(x0, x1, x2)
#define FBO_ISSUE_MIR32(x0, x1, x2, A)                                     \
  "ds_read_b32 " FBV_122 ", %[lmt]\n\t"                                           \
  "ds_read_u16 " A ", %[lmt2] offset:256\n\t"                              \
  "v_add_u32_e32 %[lmt], 0x180, %[lmt]\n\t"                                \
  "v_add_u32_e32 %[lmt2], 0x180, %[lmt2]\n\t"                              \
  "s_waitcnt lgkmcnt(0)\n\t"                                               \
  "v_lshlrev_b32_e32 " FBV_122 ", 3, " FBV_122 "\n\t"                                    \
  FBO_GATHER(x0, x1, x2)                                                   \
  "v_lshl_add_u32 " A ", " A ", 2, %[lmat]\n\t"
#define FBO_ISSUE_PLAIN32(x0, x1, x2, A)                                   \
  "ds_read_b32 " FBV_122 ", %[lres] offset:2304\n\t"                              \
  "v_mov_b32_e32 " A ", %[lres]\n\t"                                       \
  "v_add_u32_e32 %[lres], 0xa00, %[lres]\n\t"                              \
  "s_waitcnt lgkmcnt(0)\n\t"                                               \
  "v_lshlrev_b32_e32 " FBV_122 ", 3, " FBV_122 "\n\t"                                    \
  FBO_GATHER(x0, x1, x2)
// the next layer not yet issued, if there is one, into set J: mirror layers first (mi of them left), then plain ones (pi left); fl = slots in flight
#define FBO_ISSUE(J, ISSUE_MIR, ISSUE_PLAIN, x0, x1, x2, A)                \
  "s_cmp_lt_i32 %[mi], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbo_ip" J "_%=\n\t"                                    \
  ISSUE_MIR(x0, x1, x2, A)                                                 \
  "s_sub_i32 %[mi], %[mi], 1\n\t"                                          \
  "s_add_i32 %[fl], %[fl], 1\n\t"                                          \
  "s_branch .Lfbo_id" J "_%=\n"                                            \
  ".Lfbo_ip" J "_%=:\n\t"                                                  \
  "s_cmp_lt_i32 %[pi], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbo_id" J "_%=\n\t"                                    \
  ISSUE_PLAIN(x0, x1, x2, A)                                               \
  "s_sub_i32 %[pi], %[pi], 1\n\t"                                          \
  "s_add_i32 %[fl], %[fl], 1\n"                                            \
  ".Lfbo_id" J "_%=:\n\t"
// the gathers of the oldest slot in flight have landed: fl younger slots' (3 loads each, at most 3 slots) may still fly
#define FBO_WAITVM(J)                                                      \
  "s_cmp_lt_i32 %[fl], 3\n\t"                                              \
  "s_cbranch_scc1 .Lfbo_w2" J "_%=\n\t"                                    \
  "s_waitcnt vmcnt(9)\n\t"                                                 \
  "s_branch .Lfbo_wd" J "_%=\n"                                            \
  ".Lfbo_w2" J "_%=:\n\t"                                                  \
  "s_cmp_lt_i32 %[fl], 2\n\t"                                              \
  "s_cbranch_scc1 .Lfbo_w1" J "_%=\n\t"                                    \
  "s_waitcnt vmcnt(6)\n\t"                                                 \
  "s_branch .Lfbo_wd" J "_%=\n"                                            \
  ".Lfbo_w1" J "_%=:\n\t"                                                  \
  "s_cmp_lt_i32 %[fl], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbo_w0" J "_%=\n\t"                                    \
  "s_waitcnt vmcnt(3)\n\t"                                                 \
  "s_branch .Lfbo_wd" J "_%=\n"                                            \
  ".Lfbo_w0" J "_%=:\n\t"                                                  \
  "s_waitcnt vmcnt(0)\n"                                                   \
  ".Lfbo_wd" J "_%=:\n\t"
// one slot from set J (nc slots left to compute, the first mc of them mirror layers), then the slot four behind it into the same set
// (PP: text at the head of a plain layer's path -- nothing, or the priority step of the seam into the plain layers, FBO_PRIO_PLAIN)
#define FBO_SLOTP(J, PP, ISSUE_MIR, ISSUE_PLAIN, x0, x1, x2, A)            \
  "s_cmp_lt_i32 %[nc], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbo_end_%=\n\t"                                        \
  "s_sub_i32 %[nc], %[nc], 1\n\t"                                          \
  "s_sub_i32 %[fl], %[fl], 1\n\t"                                          \
  "s_cmp_lt_i32 %[mc], 1\n\t"                                              \
  "s_cbranch_scc1 .Lfbo_cp" J "_%=\n\t"                                    \
  "s_sub_i32 %[mc], %[mc], 1\n\t"                                          \
  FBO_FIRST_MIR(A)                                                         \
  FBO_WAITVM("m" J)                                                        \
  FBO_COMPUTE_MIR(x0, x1, x2, A)                                           \
  "s_branch .Lfbo_ci" J "_%=\n"                                            \
  ".Lfbo_cp" J "_%=:\n\t"                                                  \
  PP                                                                       \
  FBO_FIRST_PLAIN(A)                                                       \
  FBO_WAITVM("p" J)                                                        \
  FBO_COMPUTE_PLAIN(x0, x1, x2, A)                                         \
  ".Lfbo_ci" J "_%=:\n\t"                                                  \
  FBO_ISSUE(J, ISSUE_MIR, ISSUE_PLAIN, x0, x1, x2, A)
#define FBO_SET0 FBV_124_125, FBV_126_127, FBV_128_129, FBV_148
#define FBO_SET1 FBV_130_131, FBV_132_133, FBV_134_135, FBV_149
#define FBO_SET2 FBV_136_137, FBV_138_139, FBV_140_141, FBV_150
#define FBO_SET3 FBV_142_143, FBV_144_145, FBV_146_147, FBV_151
#define FBO_ISSUE_(J, ISSUE_MIR, ISSUE_PLAIN, SET) FBO_ISSUE(J, ISSUE_MIR, ISSUE_PLAIN, SET)
#define FBO_SLOT_(J, PP, ISSUE_MIR, ISSUE_PLAIN, SET) FBO_SLOTP(J, PP, ISSUE_MIR, ISSUE_PLAIN, SET)
// Priority by progress (round 10, the PRIO instantiations of pcg_pipe_kernel.h): the wavefront steps its priority down to 1 where its on-chip run
// passes from the mirror layers to the plain ones.  The run is ONE rotating loop over both kinds, so the step stands at the head of the plain
// layers' path and is executed again by every plain layer: one scalar instruction without an operand, the same priority again.
#define FBO_PRIO_PLAIN "s_setprio 1\n\t"
#define FBO_BODY(ISSUE_MIR, ISSUE_PLAIN) FBO_BODYP(ISSUE_MIR, ISSUE_PLAIN, "")
#define FBO_BODYP(ISSUE_MIR, ISSUE_PLAIN, PP)                                                                   \
  /* scalar operands fresh from v_readfirstlane, read by vector memory instructions: 5 wait states (see FBP_BODYG) */ \
  "s_nop 4\n\t"                                                                                                 \
  "s_mov_b32 %[fl], 0\n\t"                                                                                      \
  /* prologue: the first four slots' gathers (fewer: what there is) */                                          \
  FBO_ISSUE_("a", ISSUE_MIR, ISSUE_PLAIN, FBO_SET0)                                                             \
  FBO_ISSUE_("b", ISSUE_MIR, ISSUE_PLAIN, FBO_SET1)                                                             \
  FBO_ISSUE_("c", ISSUE_MIR, ISSUE_PLAIN, FBO_SET2)                                                             \
  FBO_ISSUE_("d", ISSUE_MIR, ISSUE_PLAIN, FBO_SET3)                                                             \
  ".Lfbo_loop_%=:\n\t"                                                                                          \
  FBO_SLOT_("0", PP, ISSUE_MIR, ISSUE_PLAIN, FBO_SET0)                                                          \
  FBO_SLOT_("1", PP, ISSUE_MIR, ISSUE_PLAIN, FBO_SET1)                                                          \
  FBO_SLOT_("2", PP, ISSUE_MIR, ISSUE_PLAIN, FBO_SET2)                                                          \
  FBO_SLOT_("3", PP, ISSUE_MIR, ISSUE_PLAIN, FBO_SET3)                                                          \
  "s_branch .Lfbo_loop_%=\n"                                                                                    \
  ".Lfbo_end_%=:\n\t"
// clang-format on

// the byte address in LDS of a pointer into the workgroup's dynamic shared memory
__device__ __forceinline__ unsigned int lds_byte_address(const void* p) {
  return (unsigned int)(unsigned long long)(__attribute__((address_space(3))) const void*)p;
}

// m >= 0 mirror layers, then kl >= 0 plain layers (both wave-uniform, both may be 0), accumulated into y0, y1, y2 in that order.
// lmt: the lane's word of the first mirror layer's table (C16: (block's LDS word) << 16 | column - row, 256 bytes per layer; else the column,
// 384 bytes per layer, and lmt2 + 256 the lane's halfword of the block's LDS word); lres: the lane's first word of the first plain layer
// (9 x 256 bytes per layer and, C16, lcd: the lane's halfword of its column - row; else 10 x 256 bytes, the tenth word the column);
// lmat: the LDS byte address the mirror tables' block words count from; pl0..2: the planes of the gathered vector.  All 64 lanes active.
template <bool C16, bool PRIO = false>
__device__ __forceinline__ void pipe_onchip_slots(int m, int kl, const void* lmt, const void* lmt2, const void* lres, const void* lcd, const void* lmat,
                                                  const double* pl0, const double* pl1, const double* pl2, int row, double& y0, double& y1, double& y2) {
  pl0 = scalar_ptr(pl0); pl1 = scalar_ptr(pl1); pl2 = scalar_ptr(pl2);
  int mi = __builtin_amdgcn_readfirstlane(m), pi = __builtin_amdgcn_readfirstlane(kl), mc = mi, nc = mi + pi, fl;
  const unsigned int almat = __builtin_amdgcn_readfirstlane(lds_byte_address(lmat));
  unsigned int almt = lds_byte_address(lmt), ares = lds_byte_address(lres);
  if constexpr (C16) {
    unsigned int acd = lds_byte_address(lcd);
    if constexpr (PRIO)
      asm volatile(FBO_BODYP(FBO_ISSUE_MIR16, FBO_ISSUE_PLAIN16, FBO_PRIO_PLAIN)
                   : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [lmt] "+v"(almt), [lres] "+v"(ares), [lcd] "+v"(acd), [mi] "+s"(mi), [pi] "+s"(pi),
                     [mc] "+s"(mc), [nc] "+s"(nc), [fl] "=&s"(fl)
                   : [lmat] "s"(almat), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2), [row] "v"(row)
                   : FBP_CLOBBERS);
    else
    asm volatile(FBO_BODY(FBO_ISSUE_MIR16, FBO_ISSUE_PLAIN16)
                 : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [lmt] "+v"(almt), [lres] "+v"(ares), [lcd] "+v"(acd), [mi] "+s"(mi), [pi] "+s"(pi),
                   [mc] "+s"(mc), [nc] "+s"(nc), [fl] "=&s"(fl)
                 : [lmat] "s"(almat), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2), [row] "v"(row)
                 : FBP_CLOBBERS);
  } else {
    unsigned int almt2 = lds_byte_address(lmt2);
    if constexpr (PRIO)
      asm volatile(FBO_BODYP(FBO_ISSUE_MIR32, FBO_ISSUE_PLAIN32, FBO_PRIO_PLAIN)
                   : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [lmt] "+v"(almt), [lmt2] "+v"(almt2), [lres] "+v"(ares), [mi] "+s"(mi), [pi] "+s"(pi),
                     [mc] "+s"(mc), [nc] "+s"(nc), [fl] "=&s"(fl)
                   : [lmat] "s"(almat), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2)
                   : FBP_CLOBBERS);
    else
    asm volatile(FBO_BODY(FBO_ISSUE_MIR32, FBO_ISSUE_PLAIN32)
                 : [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [lmt] "+v"(almt), [lmt2] "+v"(almt2), [lres] "+v"(ares), [mi] "+s"(mi), [pi] "+s"(pi),
                   [mc] "+s"(mc), [nc] "+s"(nc), [fl] "=&s"(fl)
                 : [lmat] "s"(almat), [spl0] "s"(pl0), [spl1] "s"(pl1), [spl2] "s"(pl2)
                 : FBP_CLOBBERS);
  }
}

}  // namespace fb
