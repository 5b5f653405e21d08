// The LDS window of the persistent solver's one-row kernel (k_pcg_pipe, (12, 6) and (12, 7)): which slot layers of a slice are kept in LDS, and
// which of them are read as the transpose of another row's block instead of being stored again.  Host and device use the same functions
// (fem_persist.hip: k_pipe_mirror_plan; plan_api.cpp: the host model the CPU suite checks).
//
// A = A^T bitwise, and a workgroup owns a contiguous run of slices: where a row's block (r, c) has its column in a row of
// the SAME workgroup below it (the -1, -55, -56 neighbours of the cube), the block (c, r) = (r, c)^T is one of that row's upper blocks, which the
// workgroup keeps in LDS anyway.  Per slice, a contiguous window [a, a + m + p) of slots is LDS-resident:
//   [a, a + m)       MIRROR layers: no values, a word per lane -- the column and the LDS word address of the block to read transposed: the
//                    partner row's plain block, or (partner block not resident, padding lane, ...) an entry of the workgroup's POOL, which the
//                    kernel fills at launch from `vals` and stores transposed, so that every lane of the layer reads the same nine offsets;
//   [a + m, a + m + p)  PLAIN layers: 9 values + the column word, as before.
// Slots [0, a) and [a + m + p, width) are streamed.  The product runs in slot order (dlo, stream, mirror, plain, stream): the same sum over the
// same values in the same order as the kernel without mirrors -- bit for bit.
// LDS of a workgroup, from the start of the matrix region: the plain slots of its slices (wavefront-slots of pipe_slot_bytes, in wavefront
// order) | the mirror tables (kMirTabBytes per layer, wavefront order) | the pool (groups of 64 entries, [9][64] words each).
#pragma once

namespace fb {

constexpr int kMirMax = 4;          // mirror layers of a slice at most (the unroll bound of the kernel's loop)
constexpr int kMirLanes = 56;       // a layer qualifies where at least this many of its 64 lanes have a lower column of the same workgroup
constexpr int kMirPoolMax = 1024;   // pool entries of a workgroup at most (more: that workgroup keeps no mirrors)
constexpr int kMirWaves = 12;       // slices per workgroup the table has room for (kPipeMaxWaves)
constexpr int mir_slot_bytes(bool c16) { return c16 ? 9 * 256 + 128 : 10 * 256; }  // = pipe_slot_bytes
constexpr int mir_lds_slots(bool c16) { return c16 ? 65 : 62; }                    // = pipe_lds_slots
constexpr int mir_tab_bytes(bool c16) { return c16 ? 256 : 384; }  // per mirror layer: [64] (address << 16 | 16-bit column difference), or [64] columns, [64] 16-bit addresses
constexpr int kMirGroupBytes = 9 * 256;

struct MirWave {
  int a, m, p;  // window start, mirror layers, plain layers
  int at;       // first wavefront-slot of the plain layers
  int tab;      // byte offset of the mirror table
  int d;        // (planning) the diagonal slot most lanes have, -1: none
  int width;    // (planning) slots of the slice
};

// the slot of this lane's diagonal block, -1: none (padding row)
__host__ __device__ inline int mir_lane_diag(const int* slice_off, const int* colidx, int sl, int lane, int n_owned) {
  const int row = sl * 64 + lane;
  if (row >= n_owned) return -1;
  for (int k = slice_off[sl]; k < slice_off[sl + 1]; k++)
    if (colidx[(size_t)k * 64 + lane] == row) return k - slice_off[sl];
  return -1;
}

// does this lane's block at slot k (of the slice) have a column of the workgroup's rows [lo, hi) below its own row?
__host__ __device__ inline bool mir_lane_lower(const int* slice_off, const int* colidx, int sl, int k, int lane, int lo, int hi) {
  const int row = sl * 64 + lane;
  const int c = colidx[(size_t)(slice_off[sl] + k) * 64 + lane];
  return row < hi && c >= lo && c < row;
}

// the LDS word address (from the matrix region) of the block (c, row) = the transpose of this lane's block at mirror layer k, or -1: not
// resident (the lane takes a pool entry).  lo = first row of the workgroup, hi = its end (<= n_owned); mw = the workgroup's plan.
__host__ __device__ inline int mir_lane_addr(const int* slice_off, const int* colidx, int first, const MirWave* mw, int w, int k, int lane, int lo, int hi,
                                             bool c16) {
  const int sl = first + w, row = sl * 64 + lane;
  const int c = colidx[(size_t)(slice_off[sl] + mw[w].a + k) * 64 + lane];
  if (!(row < hi && c >= lo && c < row)) return -1;
  const int w2 = (c >> 6) - first, l2 = c & 63;
  const MirWave& q = mw[w2];
  const int k0 = q.a + q.m, n = q.p < q.width - k0 ? q.p : q.width - k0;  // the partner's resident plain slots
  const int s0 = slice_off[first + w2] + k0;
  for (int j = 0; j < n; j++)
    if (colidx[(size_t)(s0 + j) * 64 + l2] == row) return q.at * (mir_slot_bytes(c16) / 4) + j * (c16 ? 9 : 10) * 64 + l2;
  return -1;
}

// The workgroup's layout from the slices' diagonal slots and mirror candidates (mw[w].d, .m, .width set): every slice keeps `share` plain
// layers (the plain kernel's least share) and its m mirror layers below the diagonal; the LDS that is left after a pool of `pool` entries
// becomes more plain layers (grow), one per slice in wavefront order, at most klt each.  Returns false where nothing fits.
__host__ __device__ inline bool mir_wg_layout(MirWave* mw, int count, int klt, bool c16, int pool, bool grow) {
  const int total = mir_lds_slots(c16) * mir_slot_bytes(c16);
  int share = mir_lds_slots(c16) / (count > 0 ? count : 1);  // (at most 6: what fb_fem_persist_info reports for 9-12 slices per CU)
  share = share < klt ? share : klt;
  share = share < 6 ? share : 6;
  int used = 0;
  for (int w = 0; w < count; w++) {
    if (mw[w].m > 0) mw[w].a = mw[w].d - mw[w].m;
    else { mw[w].a = 0; mw[w].m = 0; }
    mw[w].p = share;
    used += share * mir_slot_bytes(c16) + mw[w].m * mir_tab_bytes(c16);
  }
  const int pool_bytes = (pool + 63) / 64 * kMirGroupBytes;
  // no room for all of them: the lowest mirror layers of the last slices go back to the stream first
  for (int w = count - 1; w >= 0 && used + pool_bytes > total; w--)
    while (mw[w].m > 0 && used + pool_bytes > total) { mw[w].m--; mw[w].a++; used -= mir_tab_bytes(c16); }
  if (used + pool_bytes > total) return false;
  int extra = grow ? (total - used - pool_bytes) / mir_slot_bytes(c16) : 0;
  for (bool grew = true; extra > 0 && grew;) {
    grew = false;
    for (int w = 0; w < count && extra > 0; w++)
      if (mw[w].p < klt) { mw[w].p++; extra--; grew = true; }
  }
  int at = 0, tab = 0;
  for (int w = 0; w < count; w++) { mw[w].at = at; at += mw[w].p; }
  tab = at * mir_slot_bytes(c16);
  for (int w = 0; w < count; w++) { mw[w].tab = tab; tab += mw[w].m * mir_tab_bytes(c16); }
  return true;
}

// Register slots of a slice (pcg_pipe_regs.hip.h): of `regs` (what the instantiation holds and FEMBRAIN_PIPE_REGS allows) as many as the slice streams.
// mir_reg_split: nb of them follow the plain layers -- as many as there are slots behind the window --, the other nf precede the mirror layers, so
// streamed [0, a - nf) | register | mirror [a, a + m) | plain [a + m, a + m + p) | register | streamed [a + m + p + nb, width) partition the slice in slot order.
__host__ __device__ inline int mir_reg_slots(const MirWave& w, int regs) {
  const int behind = w.width - (w.a + w.m + w.p) > 0 ? w.width - (w.a + w.m + w.p) : 0, streamed = w.a + behind;
  return regs < streamed ? (regs > 0 ? regs : 0) : streamed;
}
__host__ __device__ inline void mir_reg_split(const MirWave& w, int r, int* nf, int* nb) {
  const int behind = w.width - (w.a + w.m + w.p) > 0 ? w.width - (w.a + w.m + w.p) : 0;
  *nb = r < behind ? r : behind;
  *nf = r - *nb < w.a ? r - *nb : w.a;
}

// byte offset of the pool (after the plain layers and the mirror tables)
__host__ __device__ inline int mir_pool_at(const MirWave* mw, int count, bool c16) {
  int b = 0;
  for (int w = 0; w < count; w++) b += mw[w].p * mir_slot_bytes(c16) + mw[w].m * mir_tab_bytes(c16);
  return b;
}

// slots of the slices the window keeps on chip, against the plain kernel's share (klt_w of k_pcg_pipe): mirrors only where they add some
__host__ __device__ inline bool mir_wg_gains(const MirWave* mw, int count, int klt, bool c16) {
  const int kSlots = mir_lds_slots(c16);
  const int lbase = (klt < kSlots / (count > 0 ? count : 1)) ? klt : kSlots / (count > 0 ? count : 1);
  const int lrem = lbase < klt ? (count < kSlots - lbase * count ? count : kSlots - lbase * count) : 0;
  int before = 0, after = 0;
  for (int w = 0; w < count; w++) {
    const int kw = lbase + (w < lrem ? 1 : 0);
    before += kw < mw[w].width ? kw : mw[w].width;
    const int rest = mw[w].width - mw[w].a - mw[w].m;
    after += mw[w].m + (mw[w].p < rest ? mw[w].p : (rest > 0 ? rest : 0));
  }
  return after > before;
}

// the plain kernel's layout (no mirrors): what a workgroup whose mirrors do not pay keeps
__host__ __device__ inline void mir_wg_plain(MirWave* mw, int count, int klt, bool c16) {
  const int kSlots = mir_lds_slots(c16);
  const int lbase = (klt < kSlots / (count > 0 ? count : 1)) ? klt : kSlots / (count > 0 ? count : 1);
  const int lrem = lbase < klt ? (count < kSlots - lbase * count ? count : kSlots - lbase * count) : 0;
  for (int w = 0; w < count; w++) {
    mw[w].a = 0; mw[w].m = 0; mw[w].p = lbase + (w < lrem ? 1 : 0);
    mw[w].at = w * lbase + (w < lrem ? w : lrem);
    mw[w].tab = 0;
  }
}

}  // namespace fb
