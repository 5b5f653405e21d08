// C-ABI of the FEM hot path (include/fembrain_hip.h): assembly, the solvers, the per-step driver and the inspection entry points.
// Kernels live in fem_device.hip.h, the host-side plan in fem_plan.cpp, the handle's life cycle (build, re-sync, cut) in fem_build.hip.
#include <cfloat>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "fem_device.hip.h"
#include "fem_handle.h"

using namespace fb;

namespace {

size_t mt_size(const fb_fem_s* h) { return h->f64 ? sizeof(double) : sizeof(float); }


__global__ __launch_bounds__(kBlock) void k_widen_positions(long long n, const float* __restrict__ in, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

// (ZeroBatch, fem_handle.h)
struct ZeroList { unsigned int* p[kZeroMax]; unsigned long long end[kZeroMax]; unsigned int tail_words[kZeroMax]; int n; };  // end: running total of 16-byte chunks
__global__ __launch_bounds__(kBlock) void k_zero_many(ZeroList z, unsigned long long total_chunks) {
  for (unsigned long long c = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; c < total_chunks; c += (unsigned long long)gridDim.x * kBlock) {
    int b = 0;
    while (c >= z.end[b]) b++;
    const unsigned long long local = c - (b ? z.end[b - 1] : 0ULL);
    if (c + 1 == z.end[b] && z.tail_words[b]) {  // the buffer's last chunk holds fewer than four words: the fill never leaves the buffer
      for (unsigned int k = 0; k < z.tail_words[b]; k++) z.p[b][4 * local + k] = 0u;
    } else {
      reinterpret_cast<uint4*>(z.p[b])[local] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}
}  // namespace
namespace fb {
void ZeroBatch::add(void* ptr, size_t bytes) {
  if (!ptr || !bytes || rc != FB_OK) return;
  if (bytes & 3) {  // (not a whole number of words: the runtime's fill)
    if (hipMemsetAsync(ptr, 0, bytes, s) != hipSuccess) rc = fail(FB_EDEVICE, "hipMemsetAsync failed");
    return;
  }
  if (n == kZeroMax) flush();
  const unsigned long long chunks = (bytes + 15) / 16, before = n ? end[n - 1] : 0ULL;
  p[n] = static_cast<unsigned int*>(ptr);
  end[n] = before + chunks;
  tail_words[n] = (unsigned int)((bytes & 15) / 4);
  n++;
}
int ZeroBatch::flush() {
  if (rc != FB_OK) return rc;
  if (n == 0) return FB_OK;
  ZeroList z;
  memcpy(z.p, p, sizeof p); memcpy(z.end, end, sizeof end); memcpy(z.tail_words, tail_words, sizeof tail_words);
  z.n = n;
  const unsigned long long total = end[n - 1];
  const unsigned int blocks = (unsigned int)std::min<unsigned long long>((total + kBlock - 1) / kBlock, 256ULL * 16);
  hipLaunchKernelGGL(k_zero_many, dim3(blocks), dim3(kBlock), 0, s, z, total);
  if (hipGetLastError() != hipSuccess) rc = fail(FB_EDEVICE, "k_zero_many failed to launch");
  n = 0;
  return rc;
}

int widen_positions(hipStream_t s, long long n, const float* in, double* out) {
  hipLaunchKernelGGL(k_widen_positions, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n, in, out);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

// slack of this handle's allocations (common.h): a quarter for a mesh that will be cut, or what reserve_nodes / reserve_elements ask for
int handle_slack(const fb_fem_s* h, int n_nodes, int n_tets) {
  if (!h->prm.expect_cuts) return 2;
  double f = 0.25;
  if (h->prm.reserve_nodes > n_nodes && n_nodes > 0) f = std::max(f, (double)h->prm.reserve_nodes / n_nodes - 1.0);
  if (h->prm.reserve_elements > n_tets && n_tets > 0) f = std::max(f, (double)h->prm.reserve_elements / n_tets - 1.0);
  return std::max(2, std::min(32, (int)std::ceil(f * 16.0)));
}

// FB_RENUMBER_* of this handle: fb_fem_params.renumber unless FEMBRAIN_RENUMBER=0/1 says otherwise; a sharded handle renumbers on request only
int renumber_mode(const fb_fem_s* h) {
  if (const char* e = getenv("FEMBRAIN_RENUMBER")) return atoi(e) != 0 ? FB_RENUMBER_ON : FB_RENUMBER_OFF;
  if (h->prm.renumber == 0 && h->shard_auto_on) return FB_RENUMBER_ON;  // (a sharded handle under AUTO whose ranks voted for it)
  // a mesh that will be cut: the nodes a cut appends make any caller order wide, so the internal order is chosen at creation and the
  // first fb_fem_resync_delta merges its nodes into it instead of sending the mesh through the full builder
  if (h->prm.renumber == 0 && h->prm.expect_cuts && h->plan.n_ranks <= 1 && !h->comm) return FB_RENUMBER_ON;
  return h->prm.renumber > 0 ? FB_RENUMBER_ON : (h->prm.renumber < 0 ? FB_RENUMBER_OFF : FB_RENUMBER_AUTO);
}

int upload_masks(fb_fem_s* h) {
  const FemPlan& P = h->plan;
  FB_TRY(h->dofmask.upload(P.dofmask, h->stream));
  std::vector<uint8_t> nm((size_t)P.n_local);
  for (int l = 0; l < P.n_local; l++) nm[l] = (uint8_t)((P.dofmask[3 * (size_t)l] ? 1 : 0) | (P.dofmask[3 * (size_t)l + 1] ? 2 : 0) | (P.dofmask[3 * (size_t)l + 2] ? 4 : 0));
  return h->nodemask.upload(nm, h->stream);
}

// (the plan builders ask for spmv_c16 before upload_plan asks for all of it: a dozen getenv calls per plan build, twice)
HostKnobs read_host_knobs() {
  HostKnobs k;
  const char *ak = getenv("FEMBRAIN_ASM_KERNEL"), *per_cu = getenv("FEMBRAIN_ASM_PER_CU"), *wide_grid = getenv("FEMBRAIN_ASM_WIDE_GRID");
  const char *nt = getenv("FEMBRAIN_SPMV_NT"), *c16 = getenv("FEMBRAIN_SPMV_C16");
  k.asm_rows = ak && !strcmp(ak, "rows"), k.asm_tets1 = ak && !strcmp(ak, "tets1");
  if (per_cu) k.asm_per_cu = std::max(1, atoi(per_cu));
  if (wide_grid) k.asm_wide_grid = std::max(1, atoi(wide_grid));
  k.asm_wide_rows = getenv("FEMBRAIN_ASM_WIDE_ROWS") != nullptr;
  k.asm_profile = getenv("FEMBRAIN_ASM_PROFILE") != nullptr;
  if (nt) k.spmv_nt = atoi(nt) != 0 ? 1 : 0;
  k.spmv_c16 = !(c16 && atoi(c16) == 0);
  k.verbose = getenv("FEMBRAIN_TIMING") != nullptr;
  return k;
}
}  // namespace fb
namespace {

// ---- the SpMV's instantiations, all of them: what selects one, and its address ----
// f64: storage of the matrix values; mode 0..3 (k_spmv); split: wavefronts per slice, 0 = k_spmv, 2 | 4 = k_spmv_split (which has neither NT
// nor C16); xch 2: the halo refresh and the sums' post in the kernel (MODE 3 only); c16: 0 | 1 | 2 as fb_fem_s::c16
struct SpmvKernel { bool f64; int mode, split, xch; bool nt; int c16; const void* fn; };
#define FB_K_SPMV(MT, MODE, XCH, NT, C16) {std::is_same<MT, double>::value, MODE, 0, XCH, NT, C16, (const void*)k_spmv<MT, MODE, XCH, NT, C16>}
#define FB_K_SPLIT(MT, MODE, SPLIT, XCH) {std::is_same<MT, double>::value, MODE, SPLIT, XCH, false, 0, (const void*)k_spmv_split<MT, MODE, SPLIT, XCH>}
#define FB_K_SPMV_FORMS(MT, MODE, XCH)                                                                                           \
  FB_K_SPMV(MT, MODE, XCH, false, 0), FB_K_SPMV(MT, MODE, XCH, false, 1), FB_K_SPMV(MT, MODE, XCH, false, 2), FB_K_SPMV(MT, MODE, XCH, true, 0), \
      FB_K_SPMV(MT, MODE, XCH, true, 1), FB_K_SPMV(MT, MODE, XCH, true, 2), FB_K_SPLIT(MT, MODE, 2, XCH), FB_K_SPLIT(MT, MODE, 4, XCH)
#define FB_K_SPMV_MODES(MT) FB_K_SPMV_FORMS(MT, 0, 0), FB_K_SPMV_FORMS(MT, 1, 0), FB_K_SPMV_FORMS(MT, 2, 0), FB_K_SPMV_FORMS(MT, 3, 0), FB_K_SPMV_FORMS(MT, 3, 2)
const SpmvKernel kSpmvKernels[] = {FB_K_SPMV_MODES(float), FB_K_SPMV_MODES(double)};
#undef FB_K_SPMV_MODES
#undef FB_K_SPMV_FORMS
#undef FB_K_SPLIT
#undef FB_K_SPMV
static_assert(sizeof kSpmvKernels / sizeof kSpmvKernels[0] == 80, "60 k_spmv and 20 k_spmv_split");
// spmv() fills one argument array for all of them
typedef void (*SpmvSignature)(SellView, const double*, const double*, const double*, double*, const double*, const double*, double*, CGState*, int, P2PArgs);
static_assert(std::is_same<decltype(&k_spmv<double, 3, 2, true, 1>), SpmvSignature>::value && std::is_same<decltype(&k_spmv_split<double, 0, 4, 0>), SpmvSignature>::value, "spmv()");

// The rows this plan launches, one per MODE and the XCH = 2 one (fb_fem_set_exchange_mode may ask for it on any sharded handle later),
// stored in the handle.  A combination that was not built is refused here.
int resolve_spmv_kernels(fb_fem_s* h) {
  auto find = [h](int mode, int xch) -> const void* {
    for (const SpmvKernel& k : kSpmvKernels)
      if (k.f64 == h->f64 && k.mode == mode && k.xch == xch && k.split == h->split && (h->split || (k.nt == h->spmv_nt && k.c16 == h->c16))) return k.fn;
    return nullptr;
  };
  bool all = true;
  for (int mode = 0; mode < 4; mode++) all = (h->spmv_fn[mode] = find(mode, 0)) != nullptr && all;
  all = (h->spmv_xch_fn = find(3, 2)) != nullptr && all;
  if (!all) return fail(FB_EINVAL, "no SpMV kernel was built for %s values, %d wavefronts per slice, column words of form %d", h->f64 ? "fp64" : "fp32", h->split, h->c16);
  return FB_OK;
}

// ---- the assembly families' instantiations, all of them ----
enum AsmFamily { kFamWarp, kFamTets, kFamTetsSt, kFamRows, kFamWide, kFamMass, kFamK0 };
// f64: storage of the records and the matrix values; tangent: the exact tangent's terms (kcorr present); newmark: qacc passed; mat: the
// handle has an element map.  false where a family has no such parameter
struct AsmKernel { AsmFamily family; bool f64, tangent, newmark, mat; const void* fn; };
constexpr int kAsmG = 2;  // k_assemble_tets: list rows whose records are in flight per lane (measured at 1M tets, fp32: 224 us with 4, 209 with 2, 211 with 1)
#define FB_K_WARP(MT, TANGENT, MAT) {kFamWarp, std::is_same<MT, double>::value, TANGENT, false, MAT, (const void*)k_tet_warp<MT, TANGENT, MAT>}
#define FB_K_TETS(MT, TANGENT, NEWMARK, MAT) {kFamTets, std::is_same<MT, double>::value, TANGENT, NEWMARK, MAT, (const void*)k_assemble_tets<MT, kAsmG, TANGENT, NEWMARK, MAT>}
#define FB_K_SLOTS(FAMILY, KERNEL, MT, MAT) {FAMILY, std::is_same<MT, double>::value, false, false, MAT, (const void*)KERNEL<MT, MAT>}
#define FB_K_TETS_ST(NEWMARK, MAT) {kFamTetsSt, false, false, NEWMARK, MAT, (const void*)k_assemble_tets_st<NEWMARK, MAT>}
#define FB_K_BY_STORAGE(MT, MAT)                                                                                                              \
  FB_K_WARP(MT, false, MAT), FB_K_WARP(MT, true, MAT), FB_K_TETS(MT, false, false, MAT), FB_K_TETS(MT, false, true, MAT), FB_K_TETS(MT, true, false, MAT), \
      FB_K_TETS(MT, true, true, MAT), FB_K_SLOTS(kFamRows, k_assemble_rows, MT, MAT), FB_K_SLOTS(kFamWide, k_assemble_wide, MT, MAT)
#define FB_K_BY_MAT(MAT)                                                                                          \
  FB_K_BY_STORAGE(float, MAT), FB_K_BY_STORAGE(double, MAT), FB_K_TETS_ST(false, MAT), FB_K_TETS_ST(true, MAT),   \
      {kFamMass, false, false, false, MAT, (const void*)k_mass_blocks<float, MAT>}, {kFamK0, false, false, false, MAT, (const void*)k_element_K0_mfma<MAT>}
// (the material-aware ones first, as the code named them before there was a table: the compiler emits the kernels in this order, and its
// output for k_assemble_tets_st is the same instruction for instruction only in that one)
const AsmKernel kAsmKernels[] = {FB_K_BY_MAT(true), FB_K_BY_MAT(false)};
#undef FB_K_BY_MAT
#undef FB_K_BY_STORAGE
#undef FB_K_TETS_ST
#undef FB_K_SLOTS
#undef FB_K_TETS
#undef FB_K_WARP
static_assert(sizeof kAsmKernels / sizeof kAsmKernels[0] == 40, "8 k_tet_warp, 16 k_assemble_tets, 4 each of _tets_st / _rows / _wide, 2 each of k_mass_blocks / k_element_K0_mfma");
// the launches below fill one argument array per family: its order is the kernel's parameter list, pinned here
template <typename... P> using KernelOf = void (*)(P...);
typedef const uint32_t* CU32;
static_assert(std::is_same<decltype(&k_tet_warp<double, true, true>), KernelOf<int, const int4*, const double*, const double*, const double*, double*, double*, double*, double, double, int,
                                                                               double*, const uint8_t*, const double*>>::value, "launch_warp");
static_assert(std::is_same<decltype(&k_assemble_tets<double, kAsmG, true, true, true>), KernelOf<SellView, const int*, CU32, CU32, const double*, const double*, AsmOut<double>, AsmParams,
                                                                                                 const double*, int, unsigned long long*>>::value, "launch_rows, element-major");
static_assert(std::is_same<decltype(&k_assemble_tets_st<true, true>), KernelOf<SellView, const int*, CU32, CU32, const float*, const double*, AsmOut<float>, AsmParams, int,
                                                                               unsigned long long*>>::value, "launch_rows, staged");
static_assert(std::is_same<decltype(&k_assemble_rows<double, true>), KernelOf<SellView, const int*, const int*, CU32, const double*, const double*, AsmOut<double>, AsmParams, const double*,
                                                                              int>>::value, "launch_asm_rows");
static_assert(std::is_same<decltype(&k_assemble_wide<double, true>), KernelOf<SellView, const int*, int, int, double*, const int*, const int*, CU32, const double*, const double*,
                                                                              AsmOut<double>, AsmParams, const double*>>::value, "launch_asm_wide");
static_assert(std::is_same<decltype(&k_mass_blocks<float, true>), KernelOf<SellView, const int*, CU32, CU32, const float*, double, int, double*, const uint8_t*, const double*>>::value,
              "launch_rows, mass entries");
static_assert(std::is_same<decltype(&k_element_K0_mfma<true>), KernelOf<int, int, const double*, double, double, double*, double*, const double*, const int4*, const uint8_t*,
                                                                        const double*>>::value, "launch_element_K0");

size_t mass_blocks_lds(const fb_fem_s* h) { return (size_t)(kBlock / 64) * h->asm_max_width * 64 * sizeof(double); }

// The rows a plan launches, stored in the handle, and the dynamic-LDS size of those that have one (beyond 64 KB an attribute of the function, set
// before the launch on the handle's device).  For every plan (upload_plan) and when a handle gets its element map later (mat).  Both values of
// NEWMARK: a Newmark handle assembles without qacc too (fb_fem_assemble, fb_fem_mass).  The handle keeps what it had if anything fails.
int resolve_asm_kernels(fb_fem_s* h, bool mat) {
  const bool tangent = h->kcorr.p != nullptr;
  bool all = true;
  auto find = [&](AsmFamily family, bool f64, bool tg, bool newmark) -> const void* {
    for (const AsmKernel& k : kAsmKernels)
      if (k.family == family && k.f64 == f64 && k.tangent == tg && k.newmark == newmark && k.mat == mat) return k.fn;
    all = false;
    return nullptr;
  };
  AsmKernels K;
  K.warp = find(kFamWarp, h->f64, tangent, false);
  K.rows = find(kFamRows, h->f64, false, false);
  K.wide = find(kFamWide, h->f64, false, false);
  K.k0 = find(kFamK0, false, false, false);
  for (int nm = 0; nm < 2; nm++) {
    if (h->asm_tets) K.tets[nm] = find(kFamTets, h->f64, tangent, nm != 0);
    if (h->asm_staged) K.tets_st[nm] = find(kFamTetsSt, false, false, nm != 0);  // (an element-major plan with fp32 records and the plain tangent)
  }
  if (h->asm_staged) K.mass = find(kFamMass, false, false, false);
  if (!all) return fail(FB_EINVAL, "no assembly kernel was built for %s records%s%s", h->f64 ? "fp64" : "fp32", tangent ? ", exact tangent" : "", mat ? ", element map" : "");
  for (int nm = 0; nm < 2; nm++) {
    if (K.tets[nm]) FB_HIP(hipFuncSetAttribute(K.tets[nm], hipFuncAttributeMaxDynamicSharedMemorySize, h->asm_lds));
    if (K.tets_st[nm]) FB_HIP(hipFuncSetAttribute(K.tets_st[nm], hipFuncAttributeMaxDynamicSharedMemorySize, h->asm_lds_st));
  }
  if (K.mass) FB_HIP(hipFuncSetAttribute(K.mass, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mass_blocks_lds(h)));
  h->asm_k = K;
  return FB_OK;
}

}  // namespace
namespace fb {
int upload_plan(fb_fem_s* h, const double* xyz_global, const float* xyz_device, const double* xyz_device64) {
  const FemPlan& P = h->plan;
  hipStream_t s = h->stream;
  const HostKnobs kn = h->knobs = read_host_knobs();
  if (!h->device_plan) {  // (the device builder has put the tets and the plan arrays in place already)
    std::vector<int4> t4(P.n_tets);
    for (int e = 0; e < P.n_tets; e++) t4[e] = make_int4(P.tets[4 * (size_t)e], P.tets[4 * (size_t)e + 1], P.tets[4 * (size_t)e + 2], P.tets[4 * (size_t)e + 3]);
    FB_TRY(h->tets.upload(t4, s));
    FB_TRY(h->slice_off.upload(P.slice_off, s));
    FB_TRY(h->colidx.upload(P.colidx, s));
    FB_TRY(h->slot_coff.upload(P.slot_coff, s));
    FB_TRY(h->slot_ccnt.upload(P.slot_ccnt, s));
    FB_TRY(h->contrib.upload(P.contrib.data(), P.contrib.size(), s));
  }
  if (h->x0_ready) {
    // (renumbered: gathered into the internal order by build_plan_on_device)
  } else if (xyz_device64) {  // (fb_fem_resync_delta: the caller-order positions, already on this device)
    FB_TRY(h->x0.alloc((size_t)3 * P.n_local));
    FB_HIP(hipMemcpyAsync(h->x0.p, xyz_device64, sizeof(double) * 3 * (size_t)P.n_local, hipMemcpyDeviceToDevice, s));
  } else if (xyz_device) {  // mesh handed over on the device (fb_fem_create_from_poly): float positions widened in place
    FB_TRY(h->x0.alloc((size_t)3 * P.n_local));
    FB_TRY(widen_positions(s, 3LL * P.n_local, xyz_device, h->x0.p));
  } else {
    if (P.n_ranks == 1) {  // identity numbering
      FB_TRY(h->x0.upload(xyz_global, (size_t)3 * P.n_local, s));
    } else {
      std::vector<double>& x0 = h->x0_stage;
      x0.resize((size_t)3 * P.n_local);
      const bool mapped = !h->l2c.empty();  // (renumbered: the owned nodes are a range of the INTERNAL order, anywhere in the caller's)
      if (!mapped) memcpy(x0.data(), xyz_global + 3 * (size_t)P.node_lo, sizeof(double) * 3 * (size_t)P.n_owned);  // owned nodes are a contiguous global range
      for (int l = mapped ? 0 : P.n_owned; l < P.n_local; l++)
        for (int k = 0; k < 3; k++) x0[3 * (size_t)l + k] = xyz_global[3 * (size_t)(mapped ? h->l2c[l] : P.local2global[l]) + k];
      FB_TRY(h->x0.upload(x0, s));
    }
  }
  FB_TRY(h->rest.alloc((size_t)16 * P.n_tets));
  FB_TRY(h->volf.alloc((size_t)std::max(1, P.n_tets)));
  FB_TRY(h->fe.alloc((size_t)12 * P.n_tets));
  FB_TRY(h->rec.alloc((size_t)16 * P.n_tets * mt_size(h)));
  if (h->prm.exact_tangent && !h->prm.linear) FB_TRY(h->kcorr.alloc((size_t)144 * P.n_tets * mt_size(h)));
  else h->kcorr.release();
  if (!h->masks_ready) FB_TRY(upload_masks(h));
  if (!P.send_local.empty()) FB_TRY(h->send_local.upload(P.send_local, s));
  FB_TRY(h->sendbuf.alloc(std::max<size_t>(1, (size_t)12 * P.send_local.size())));
  ZeroBatch zb(s);
  FB_TRY(h->vals.alloc((size_t)P.n_slots * 9 * 64 * mt_size(h)));
  zb.add(h->vals);
  FB_TRY(h->dlo.alloc((size_t)P.n_slices * 9 * 64 * mt_size(h)));
  zb.add(h->dlo);
  FB_TRY(h->mblk.alloc((size_t)P.n_slots * 64));
  zb.add(h->mblk);
  {
    // Element-major assembly where the accumulators of the widest slice fit the LDS of a CU (5 KB per slot: up to 32 slots);
    // FEMBRAIN_ASM_KERNEL=rows keeps the slot-major kernel (same result bit for bit, tests/test_fem_gpu.py)
    // (the widest slice the element-major kernels take, and how many are wider: those few go to the slot-major kernel -- one hub node
    // used to send the whole mesh there)
    int mw = 0, n_wide = 0, widest = 0;
    std::vector<int> wide;
    for (int sl = 0; sl < P.n_slices; sl++) {
      const int wsl = P.slice_off[sl + 1] - P.slice_off[sl];
      if (wsl > kIncMaxWidth) { n_wide++; widest = std::max(widest, wsl); wide.push_back(sl); } else mw = std::max(mw, wsl);
    }
    h->asm_wide = n_wide;
    h->asm_wide_slots = widest;
    h->asm_wide_grid = 0;
    if (n_wide > 0) {  // k_assemble_wide: one workgroup per wide slice while their scratch areas stay under 64 MB, fewer (each taking several) beyond
      const size_t area = (size_t)widest * kWideTerms * 64;  // doubles
      h->asm_wide_grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_wide, ((size_t)64 << 20) / (area * sizeof(double))));
      if (kn.asm_wide_grid) h->asm_wide_grid = std::min(h->asm_wide_grid, kn.asm_wide_grid);  // (tests: several slices per workgroup)
      FB_TRY(h->wide_list.upload(wide, s));
      FB_TRY(h->wide_scratch.alloc(area * (size_t)h->asm_wide_grid));
    }
    hipDeviceProp_t prop;
    FB_HIP(hipGetDeviceProperties(&prop, h->prm.device));
    const int lds_cu = (int)std::min<size_t>(std::max<size_t>(prop.maxSharedMemoryPerMultiProcessor, prop.sharedMemPerBlock), 160 * 1024);  // gfx950: 160 KB per CU
    h->asm_max_width = mw;
    h->asm_lds = (mw * 10 + kAsmExtra) * 64 * (int)sizeof(double);
    h->asm_tets = mw >= 2 && mw <= kIncMaxWidth && h->asm_lds <= lds_cu && h->asm_lds <= (int)prop.sharedMemPerBlock && !kn.asm_rows;
    if (h->asm_tets) {
      FB_TRY(build_incidence_device(s, P.n_slices, P.n_owned, h->slice_off.p, h->colidx.p, h->slot_coff.p, h->slot_ccnt.p, h->contrib.p, h->tets.p, h->inc_off,
                                    h->inc, h->inc_slot, h->plan_ws, P.n_ranks == 1));
      auto per_cu_of = [&](int lds) { return std::max(1, kn.asm_per_cu ? std::min(lds_cu / lds, kn.asm_per_cu) : lds_cu / lds); };  // (FEMBRAIN_ASM_PER_CU: development aid)
      const int per_cu = per_cu_of(h->asm_lds), cus = std::max(8, (prop.multiProcessorCount / 8) * 8), chunk = ceil_div(P.n_slices, 8);
      h->asm_grid = 8 * std::max(1, std::min(chunk, (cus / 8) * per_cu));
      if (kn.verbose) fprintf(stderr, "[fembrain] element-major assembly: %d workgroups, %d B of LDS each (%d per CU; device reports %zu / %zu)\n", h->asm_grid, h->asm_lds, per_cu, (size_t)prop.maxSharedMemoryPerMultiProcessor, (size_t)prop.sharedMemPerBlock);
      const bool tangent = h->prm.exact_tangent && !h->prm.linear;
      // fp32 records and the plain tangent: the staged form (one record fetch per row and element, mass entries precomputed);
      // FEMBRAIN_ASM_KERNEL=tets1 keeps the unstaged element-major kernel (same bits)
      h->asm_lds_st = (mw * 9 + kAsmExtra) * 64 * (int)sizeof(double) + kAsmStageDoubles * (int)sizeof(double);
      h->asm_staged = !h->f64 && !tangent && h->asm_lds_st <= lds_cu && h->asm_lds_st <= (int)prop.sharedMemPerBlock && !kn.asm_tets1;
      if (h->asm_staged) {
        const int per_cu_st = per_cu_of(h->asm_lds_st);
        h->asm_grid_st = 8 * std::max(1, std::min(chunk, (cus / 8) * per_cu_st));
        if (kn.verbose) fprintf(stderr, "[fembrain] staged element-major assembly: %d workgroups, %d B of LDS each (%d per CU)\n", h->asm_grid_st, h->asm_lds_st, per_cu_st);
      }
    } else {
      h->asm_staged = false;
      h->inc_off.release(); h->inc.release(); h->inc_slot.release();
    }
    FB_TRY(resolve_asm_kernels(h, h->mat_ids.p != nullptr));  // (with the LDS sizes above)
    h->mass_valid = false;
  }
  if (h->prm.pcg_variant == FB_PCG_BLOCK_JACOBI) {
    if (P.n_ranks > 1) return fail(FB_EINVAL, "FB_PCG_BLOCK_JACOBI is for unsharded handles");
    FB_TRY(h->invblk.alloc((size_t)9 * P.n_local));
  }
  const size_t nv = (size_t)3 * P.n_local + 2;  // spare doubles: the vector kernels walk owned rows in 16-byte pairs
  DevBuf<double>* vecs[] = {&h->q, &h->qvel, &h->fext, &h->fint, &h->rhs, &h->x, &h->r, &h->d, &h->Ad, &h->invdiag, &h->tmp};
  for (auto* v : vecs) {
    FB_TRY(v->alloc(nv));
    zb.add(*v);
  }
  DevBuf<double>* nvecs[] = {&h->qacc, &h->q1, &h->qvel1, &h->qacc1};
  for (auto* v : nvecs) {
    if (h->prm.integrator == FB_INTEGRATOR_NEWMARK) { FB_TRY(v->alloc(nv)); zb.add(*v); }
    else v->release();
  }
  FB_TRY(zb.flush());
  h->pcg_warm = false;
  const int chunk = ceil_div(P.n_slices, 8);
  const int per = std::max(1, std::min(kMaxPartials / 8, ceil_div(chunk, kWavesPerBlock)));
  h->grid = 8 * per;
  const int want = h->prm.spmv_kernel;
  if (want == FB_SPMV_SPLIT && 8 * ceil_div(chunk, 2) > kMaxPartials)
    return fail(FB_EINVAL, "split SpMV needs a mesh (or shard) of <= %d slices, this one has %d", 2 * kMaxPartials, P.n_slices);
  h->split = 0;
  if (want == FB_SPMV_SPLIT || want == 0) {
    if (8 * chunk <= kMaxPartials) h->split = 4;
    // two wavefronts per slice still pay up to ~1,700 slices (us per iteration, split vs rows: 17.5 / 18.1 at 1,158 slices,
    // 19.1 / 19.5 at 1,521, 23.1 / 22.1 at 1,954); an explicit FB_SPMV_SPLIT is honoured up to the partial-sum limit
    else if (8 * ceil_div(chunk, 2) <= kMaxPartials && (want == FB_SPMV_SPLIT || P.n_slices <= 1700)) h->split = 2;
  }
  h->sgrid = h->split == 4 ? 8 * chunk : (h->split == 2 ? 8 * ceil_div(chunk, 2) : h->grid);
  {
    // bytes one PCG iteration moves: matrix values + indices + the 12 vector streams of the two kernels
    const double iter_bytes = (double)P.n_slots * 64 * (9.0 * mt_size(h) + 4.0) + 12.0 * 24.0 * P.n_local;
    h->spmv_nt = kn.spmv_nt >= 0 ? kn.spmv_nt != 0 : iter_bytes > 384.0 * 1024 * 1024;  // measured: -2 % at 341 MB, +11 % at 469 MB, +15 % at 1.1 GB
  }
  // small meshes: one 16-byte pair per thread in the merged vector pass (8.9 vs 9.3 us per iteration at 105k tets; on the 1M-tet
  // mesh the extra blocks cost more in the partial-sum prologue than they save: 29.9 vs 29.1)
  h->vgrid = h->split == 4 ? 8 * std::max(1, ceil_div(chunk * 96, kBlock)) : h->grid;
  // Persistent solver: unsharded handles whose slices fit one wavefront each on the CUs of the device.  Opt-in by
  // fb_fem_params.pcg_variant = FB_PCG_PERSISTENT or FEMBRAIN_PCG_PERSIST=1 (=0 forces it off)
  FB_TRY(setup_persist(h));
  FB_TRY(h->part_a.alloc(3 * kMaxPartials));
  FB_TRY(h->part_b.alloc(kMaxPartials));
  FB_TRY(h->part_c.alloc(3 * kMaxPartials));
  FB_TRY(h->scal.alloc(8));
  FB_TRY(h->st.alloc(1));
  FB_TRY(h->st.zero(s));
  FB_TRY(h->counter.alloc(1));
  FB_TRY(resolve_spmv_kernels(h));  // (split, spmv_nt and c16 are final)
  if (!h->device_plan) FB_HIP(hipStreamSynchronize(s));  // (a device-built plan: the rest-state check that follows waits for all of it)
  h->system_valid = false;
  return FB_OK;
}


int launch_rest(fb_fem_s* h, int* first_flat) {
  h->mass_valid = false;  // (the rest volumes may change)
  const int nt = h->plan.n_tets;
  hipLaunchKernelGGL(k_tet_rest, dim3(ceil_div(nt, kBlock)), dim3(kBlock), 0, h->stream, nt, h->tets.p, h->x0.p, h->rest.p, first_flat, h->volf.p);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

// owned part of a device vector -> its range of a global-length host vector
int download_owned(fb_fem_s* h, const DevBuf<double>& src, double* g) {
  const FemPlan& P = h->plan;
  if (P.n_ranks == 1 && h->ren.active) {  // internal order -> caller order on the device, one contiguous copy out
    FB_TRY(h->io.reserve((size_t)3 * P.n_local));
    FB_TRY(gather_nodes(h->stream, P.n_local, 3, src.p, h->ren.d_new_of_old.p, h->io.p));
    return h->io.download(g, (size_t)3 * P.n_local, h->stream);
  }
  if (!h->l2c.empty()) {  // a renumbered shard: its owned nodes lie anywhere in the caller's order
    std::vector<double> loc((size_t)3 * P.n_owned);
    FB_TRY(src.download(loc.data(), loc.size(), h->stream));
    for (int l = 0; l < P.n_owned; l++)
      for (int k = 0; k < 3; k++) g[3 * (size_t)h->l2c[l] + k] = loc[3 * (size_t)l + k];
    return FB_OK;
  }
  return src.download(g + 3 * (size_t)P.node_lo, (size_t)3 * P.n_owned, h->stream);
}
}  // namespace fb
namespace {
// ---- per-element materials ----

inline void lame_of(double E, double nu, double* lambda, double* mu) {
  *lambda = (nu * E) / ((1 + nu) * (1 - 2 * nu));
  *mu = E / (2 * (1 + nu));
}

// the device table of n materials under the handle's force scaling: lambda | mu | rho/20, padded with entry 0
int upload_material_table(fb_fem_s* h, int n, const double* E, const double* nu, const double* rho) {
  std::vector<double> tab((size_t)3 * kMaxMaterials);
  for (int i = 0; i < kMaxMaterials; i++) {
    const int k = i < n ? i : 0;  // (padding: any byte indexes a valid material)
    lame_of(E[k] * h->force_scale, nu[k], &tab[i], &tab[kMaxMaterials + i]);
    tab[2 * kMaxMaterials + i] = rho[k] / 20.0;
  }
  return h->mat_tab.upload(tab, h->stream);
}

// lambda / mu of the handle (= material 0) and, where an element map exists, the device table.  rho_changed: the mass entries
// (k_mass_blocks) are to be formed again -- they do not depend on E or nu
int refresh_materials(fb_fem_s* h, bool rho_changed) {
  if (has_material_map(h)) FB_TRY(upload_material_table(h, (int)h->mat_E.size(), h->mat_E.data(), h->mat_nu.data(), h->mat_rho.data()));
  lame_of(h->prm.E * h->force_scale, h->prm.nu, &h->lambda, &h->mu);
  h->system_valid = false;
  if (rho_changed) h->mass_valid = false;
  return FB_OK;
}

inline void asm_materials(const fb_fem_s* h, AsmParams& ap) {
  ap.lambda = h->lambda; ap.mu = h->mu; ap.rho20 = h->prm.rho / 20.0;
  ap.mtab = has_material_map(h) ? h->mat_tab.p : nullptr;
}


// halo refresh of a per-node array (`width` doubles per node: 3 for vectors, 12 for PCG records); no-op when unsharded
__global__ __launch_bounds__(kBlock) void k_pack_nodes(int n, int width, const int* __restrict__ ids, const double* __restrict__ v,
                                                       double* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n * width) return;
  const int node = i / width, c = i - node * width;
  out[i] = v[(size_t)width * ids[node] + c];
}

int halo_exchange(fb_fem_s* h, double* vec, int width = 3) {
  if (!h->comm || h->comm->n_ranks == 1) return FB_OK;
  const FemPlan& P = h->plan;
  const int ns = (int)P.send_local.size();
  if (h->xch_mode >= FB_XCH_P2P)
    return p2p_halo(h->p2p, width, h->send_local.p, h->send_off_dev.p, P.n_local - P.n_owned, h->halo_off_dev.p, P.n_owned, vec, h->stream);
  if (ns > 0) {
    hipLaunchKernelGGL(k_pack_nodes, dim3(ceil_div(ns * width, kBlock)), dim3(kBlock), 0, h->stream, ns, width, h->send_local.p, vec, h->sendbuf.p);
    FB_HIP(hipGetLastError());
  }
  return comm_exchange_nodes(h->comm, h->sendbuf.p, P.send_off.data(), vec + (size_t)width * P.n_owned, P.halo_off.data(), width, h->stream);
}

int launch_warp(fb_fem_s* h, const double* u, double* rot) {
  int nt = h->plan.n_tets, linear = h->prm.linear != 0 ? 1 : 0;
  void* args[] = {&nt, &h->tets.p, &h->x0.p, &u, &h->rest.p, &h->rec.p, &h->fe.p, &rot, &h->lambda, &h->mu, &linear, &h->kcorr.p, &h->mat_ids.p, &h->mat_tab.p};
  FB_HIP(hipLaunchKernel(h->asm_k.warp, dim3(ceil_div(nt, kBlock)), dim3(kBlock), args, 0, h->stream));
  return FB_OK;
}

int launch_element_K0(fb_fem_s* h, int first, int n, double* K0, double* Minv) {
  void* args[] = {&first, &n, &h->rest.p, &h->lambda, &h->mu, &K0, &Minv, &h->x0.p, &h->tets.p, &h->mat_ids.p, &h->mat_tab.p};
  FB_HIP(hipLaunchKernel(h->asm_k.k0, dim3(ceil_div(n, kWavesPerBlock)), dim3(kBlock), args, 0, h->stream));
  return FB_OK;
}

// k_assemble_wide: the slices of wide_list, on stream s
template <typename MT>
int launch_asm_wide(fb_fem_s* h, hipStream_t s, AsmOut<MT> o, AsmParams ap) {
  SellView sv = sell_view(h);
  void* args[] = {&sv, &h->wide_list.p, &h->asm_wide, &h->asm_wide_slots, &h->wide_scratch.p, &h->slot_coff.p, &h->slot_ccnt.p, &h->contrib.p, &h->rec.p, &h->fe.p, &o, &ap, &h->kcorr.p};
  FB_HIP(hipLaunchKernel(h->asm_k.wide, dim3(h->asm_wide_grid), dim3(kWideBlock), args, 0, s));
  return FB_OK;
}

// k_assemble_rows: the slices at least min_width slots wide (0: all of them)
template <typename MT>
int launch_asm_rows(fb_fem_s* h, AsmOut<MT> o, AsmParams ap, int min_width) {
  SellView sv = sell_view(h);
  void* args[] = {&sv, &h->slot_coff.p, &h->slot_ccnt.p, &h->contrib.p, &h->rec.p, &h->fe.p, &o, &ap, &h->kcorr.p, &min_width};
  FB_HIP(hipLaunchKernel(h->asm_k.rows, dim3(h->grid), dim3(kBlock), args, 0, h->stream));
  return FB_OK;
}

// FEMBRAIN_ASM_PROFILE=1: where an element-major kernel's wavefronts spend their time (16 counters or null to `launch`; 100 MHz ticks summed over `grid` workgroups)
template <typename Launch>
int launch_profiled(fb_fem_s* h, const char* kernel, int grid, Launch launch) {
  unsigned long long* prof = nullptr;
  if (h->knobs.asm_profile) {
    FB_HIP(hipMalloc((void**)&prof, 16 * sizeof(unsigned long long)));
    FB_HIP(hipMemset(prof, 0, 16 * sizeof(unsigned long long)));
  }
  FB_HIP(launch(prof));
  if (prof) {
    FB_HIP(hipStreamSynchronize(h->stream));
    unsigned long long t[16];
    FB_HIP(hipMemcpy(t, prof, sizeof t, hipMemcpyDeviceToHost));
    for (int w = 0; w < 4; w++)
      fprintf(stderr, "[fembrain] %s wavefront %d: elements %.1f us, wait %.1f, algebra %.1f, wait %.1f (mean per workgroup)\n", kernel, w, t[4 * w] * 0.01 / grid,
              t[4 * w + 1] * 0.01 / grid, t[4 * w + 2] * 0.01 / grid, t[4 * w + 3] * 0.01 / grid);
    (void)hipFree(prof);
  }
  return FB_OK;
}

template <typename MT>
int launch_rows(fb_fem_s* h, AsmParams ap, const double* qvel, const double* fext, double* mblk_out, double* fint_out,
                double* rhs, double* invdiag, const double* qacc = nullptr) {
  const AsmKernels& K = h->asm_k;
  AsmOut<MT> o;
  o.dofmask = h->dofmask.p; o.nodemask = h->nodemask.p; o.qvel = qvel; o.fext = fext; o.qacc = qacc; o.vals = (MT*)h->vals.p; o.dlo = (MT*)h->dlo.p; o.mblk_out = mblk_out;
  o.fint_out = fint_out; o.rhs = rhs; o.invdiag = invdiag;
  o.res_all = nullptr;
  if (rhs && h->prm.integrator == FB_INTEGRATOR_NEWMARK && h->nm_max_newton > 1) {  // (kept between calls: alloc is a no-op while the size fits)
    FB_TRY(h->res_all.alloc((size_t)3 * h->plan.n_local + 2));
    o.res_all = h->res_all.p;
  }
  o.invblk = invdiag && h->prm.pcg_variant == FB_PCG_BLOCK_JACOBI ? h->invblk.p : nullptr;
  o.mblk_in = nullptr;
  // The few slices too wide for the element-major kernel (hub nodes, hull nodes of a Delaunay mesh): the slot-major kernel on those only,
  // on a stream of its own BESIDE the element-major launch -- one wavefront takes ~0.8 ms for a 59-slot slice (one latency-bound slot after
  // the other) while the element-major kernel does the other 1,300 slices of the 606k-tet probe in 0.19 ms; the two write disjoint slices.
  // (A CU-masked handle has no second stream with the same mask: the pass then follows in order.)
  const bool wide_pass = h->asm_tets && !mblk_out && h->asm_wide > 0;
  bool wide_beside = false;
  if (wide_pass) {
    if (!h->side && h->cu_limit == 0) {
      if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); h->side = nullptr; }
      for (auto& e : h->ev_side) if (h->side && !e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); }
    }
    wide_beside = h->side && h->ev_side[0] && h->ev_side[1] && !h->knobs.asm_wide_rows;
    if (wide_beside) {
      FB_HIP(hipEventRecord(h->ev_side[0], h->stream));  // (the records and element forces of this assembly are complete)
      FB_HIP(hipStreamWaitEvent(h->side, h->ev_side[0], 0));
      FB_TRY(launch_asm_wide(h, h->side, o, ap));
      FB_HIP(hipEventRecord(h->ev_side[1], h->side));
    }
  }
  SellView sv = sell_view(h);
  if (h->asm_tets && h->asm_staged && std::is_same<MT, float>::value && !h->kcorr.p && !mblk_out) {  // (never for MT = double: k_assemble_tets_st takes AsmOut<float>)
    if (!h->mass_valid) {  // once per rebuild of the rest data
      void* args[] = {&sv, &h->inc_off.p, &h->inc.p, &h->inc_slot.p, &h->volf.p, &ap.rho20, &h->asm_max_width, &h->mblk.p, &h->mat_ids.p, &ap.mtab};
      FB_HIP(hipLaunchKernel(K.mass, dim3(ceil_div(h->plan.n_slices, kBlock / 64)), dim3(kBlock), args, mass_blocks_lds(h), h->stream));
      h->mass_valid = true;
    }
    o.mblk_in = h->mblk.p;
    FB_TRY(launch_profiled(h, "k_assemble_tets_st", h->asm_grid_st, [&](unsigned long long* prof) {
      void* args[] = {&sv, &h->inc_off.p, &h->inc.p, &h->inc_slot.p, &h->rec.p, &h->fe.p, &o, &ap, &h->asm_max_width, &prof};
      return hipLaunchKernel(K.tets_st[qacc ? 1 : 0], dim3(h->asm_grid_st), dim3(kBlock), args, (size_t)h->asm_lds_st, h->stream);
    }));
  } else if (h->asm_tets && !mblk_out) {  // (the per-block mass read-back, fb_fem_mass, goes through the slot-major kernel)
    FB_TRY(launch_profiled(h, "k_assemble_tets", h->asm_grid, [&](unsigned long long* prof) {
      void* args[] = {&sv, &h->inc_off.p, &h->inc.p, &h->inc_slot.p, &h->rec.p, &h->fe.p, &o, &ap, &h->kcorr.p, &h->asm_max_width, &prof};
      return hipLaunchKernel(K.tets[qacc ? 1 : 0], dim3(h->asm_grid), dim3(kBlock), args, (size_t)h->asm_lds, h->stream);
    }));
  } else {
    FB_TRY(launch_asm_rows(h, o, ap, 0));
  }
  if (wide_pass && wide_beside) {
    FB_HIP(hipStreamWaitEvent(h->stream, h->ev_side[1], 0));
  } else if (wide_pass) {
    AsmOut<MT> ow = o;
    ow.mblk_in = nullptr;
    if (h->knobs.asm_wide_rows) FB_TRY(launch_asm_rows(h, ow, ap, h->asm_max_width));  // development aid: the one-wavefront-per-slice form (same bits)
    else FB_TRY(launch_asm_wide(h, h->stream, ow, ap));
  }
  return FB_OK;
}

}  // namespace
namespace fb {
// pass 1 + pass 2 of the system of the current state (Keff, rhs, invdiag)
int assemble_system(fb_fem_s* h) {
  const double hh = h->prm.timestep, cM = h->prm.damping_mass, cK = h->prm.damping_stiffness;
  FB_TRY(halo_exchange(h, h->q.p));
  FB_TRY(halo_exchange(h, h->qvel.p));
  AsmParams ap;
  asm_materials(h, ap);
  const double* qacc = nullptr;
  if (h->prm.integrator == FB_INTEGRATOR_NEWMARK) {
    // implicitNewmarkSparse.cpp:218-236: K_eff = K + alpha4 (cK K + cM M) + alpha1 M;  residual = -(M qaccel + (cK K + cM M) qvel + f_int - f_ext)
    const double a1 = 1.0 / (h->nm_beta * hh * hh), a4 = h->nm_gamma / (h->nm_beta * hh);
    FB_TRY(halo_exchange(h, h->qacc.p));
    ap.s_k = 1.0 + a4 * cK; ap.s_m = a4 * cM + a1;
    ap.g_k = cK; ap.g_m = cM; ap.g_a = 1.0; ap.rhs_scale = -1.0;
    qacc = h->qacc.p;
  } else {
    ap.s_k = hh * (hh + cK); ap.s_m = 1.0 + hh * cM;   // Keff = M + h D + h^2 K, D = cK K + cM M
    ap.g_k = hh + cK; ap.g_m = cM;                     // (h K + D) qvel
    ap.g_a = 0.0; ap.rhs_scale = -hh;
  }
  ap.apply_mask = 1;
  FB_TRY(launch_warp(h, h->q.p, nullptr));
  FB_TRY(h->f64 ? launch_rows<double>(h, ap, h->qvel.p, h->fext.p, nullptr, h->fint.p, h->rhs.p, h->invdiag.p, qacc)
                : launch_rows<float>(h, ap, h->qvel.p, h->fext.p, nullptr, h->fint.p, h->rhs.p, h->invdiag.p, qacc));
  h->system_valid = true;
  return FB_OK;
}

void drop_graph(fb_fem_s* h) {
  if (h->batch_graph) (void)hipGraphExecDestroy(h->batch_graph);
  h->batch_graph = nullptr;
  h->graph_rhs = nullptr;
}
}  // namespace fb
namespace {

// One SpMV launch in the plan's instantiation of MODE (k_spmv: 0 y = A x, 1 with d . q, 2 r = b - A x, 3 the three merged sums).  xch: MODE 3 of a
// sharded handle on the peer-to-peer transport, which also gathers the halo columns from the inbox and whose last block posts the sums (XCH = 2).
// Called thousands of times per solve and under stream capture: a kernel launch through the stored address and nothing else.
int spmv(fb_fem_s* h, int mode, const double* x, double* y, const double* b, double* partial, int parity, const P2PArgs* xch = nullptr) {
  SellView sv = sell_view(h);
  P2PArgs pa = xch ? *xch : P2PArgs();
  void* args[] = {&sv, &h->vals.p, &h->dlo.p, &x, &y, &b, &h->invdiag.p, &partial, &h->st.p, &parity, &pa};
  FB_HIP(hipLaunchKernel(xch ? h->spmv_xch_fn : h->spmv_fn[mode], dim3(h->sgrid), dim3(kBlock), args, 0, h->stream));
  return FB_OK;
}

// multi-GPU: fold the per-block partials into one scalar and all-reduce it; returns the device scalar pointer
// the consumer kernels should read, or nullptr (single GPU: consumers sum the partials themselves)
__global__ __launch_bounds__(kBlock) void k_fold_partials(const double* partial, int n, int count, double* out, const CGState* st) {
  __shared__ double lds[4];
  if (st && st->done) return;
  for (int c = 0; c < count; c++) {
    const double s = sum_partials(partial + (size_t)c * n, n, lds);
    if (threadIdx.x == 0) out[c] = s;
  }
}

// n = number of per-block partials per sum: h->grid for the vector kernels, h->sgrid for the SpMV launches (they differ when
// the split SpMV runs)
int global_scalar(fb_fem_s* h, const double* partial, double** out, bool check_done, int count = 1, int slot = 0, int n = -1) {
  *out = nullptr;
  if (!h->comm || (!h->comm->nccl && !h->comm->local)) return FB_OK;
  if (n < 0) n = h->grid;
  if (h->xch_mode >= FB_XCH_P2P) {  // fold + exchange + rank-ordered sum in one single-block kernel
    FB_TRY(p2p_reduce(h->p2p, partial, n, count, h->scal.p + slot, h->stream));
    *out = h->scal.p;
    return FB_OK;
  }
  hipLaunchKernelGGL(k_fold_partials, dim3(1), dim3(kBlock), 0, h->stream, partial, n, count, h->scal.p + slot, check_done ? h->st.p : nullptr);
  FB_HIP(hipGetLastError());
  // a converged solve leaves the previous (identical on every rank) values in place; the all-reduce still runs on
  // every rank so the collective sequence stays matched, and its result is ignored by the done-checking consumers
  FB_TRY(comm_allreduce_sum(h->comm, h->scal.p + slot, count, h->stream));
  *out = h->scal.p;  // consumers index the scalar block themselves ([0..2] pending sums, [3] exact rho)
  return FB_OK;
}

int pcg_iteration(fb_fem_s* h, int it, const double* b) {
  const FemPlan& P = h->plan;
  const int variant = h->literal_now ? FB_PCG_REFERENCE : h->prm.pcg_variant;  // (a tight tolerance runs the literal sequence, see pcg_solve)
  const int parity = (it - 1) & 1;
  const bool refresh = (it % 30 == 0);
  double* sc = nullptr;
  if (variant == FB_PCG_BLOCK_JACOBI) {  // literal sequence, z = B^-1 r (unsharded: the partials are summed by the consumers)
    FB_TRY(spmv(h, 1, h->d.p, h->Ad.p, nullptr, h->part_a.p, parity));
    if (!refresh) {
      hipLaunchKernelGGL(k_bj_update<false>, dim3(h->grid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->st.p, parity, h->part_a.p, h->sgrid, h->d.p,
                         h->Ad.p, h->invblk.p, h->x.p, h->r.p, h->part_b.p);
    } else {
      hipLaunchKernelGGL(k_bj_update<true>, dim3(h->grid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->st.p, parity, h->part_a.p, h->sgrid, h->d.p,
                         h->Ad.p, h->invblk.p, h->x.p, h->r.p, h->part_b.p);
      FB_TRY(spmv(h, 2, h->x.p, h->r.p, b, h->part_c.p, parity));  // r = b - A x (its Jacobi-weighted sum is not used)
      hipLaunchKernelGGL(k_bj_rho, dim3(h->grid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->st.p, h->r.p, h->invblk.p, h->part_b.p);
    }
    hipLaunchKernelGGL(k_bj_direction, dim3(h->grid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->st.p, parity, h->part_b.p, h->grid, h->r.p,
                       h->invblk.p, h->d.p);
    FB_HIP(hipGetLastError());
    return FB_OK;
  }
  if (!refresh && (variant == FB_PCG_MERGED || variant == FB_PCG_PERSISTENT) && h->xch_mode >= FB_XCH_P2P_SUMS) {
    // Peer-to-peer transport with the exchanges inside the iteration's own kernels: the vector pass posts (block 0) and
    // awaits the three sums in its prologue; in FB_XCH_P2P_FUSED the SpMV also refreshes the halo in its prologue (a block
    // per neighbour sends, every block waits and gathers halo columns from the inbox) -- two launches, as on one GPU.
    P2PArgs pa = p2p_next_sum(h->p2p);
    pa.send_ids = h->send_local.p; pa.send_off = h->send_off_dev.p; pa.halo_off = h->halo_off_dev.p; pa.slice_halo = h->slice_halo.p;
    if (h->xch_mode == FB_XCH_P2P_FUSED) {
      pa.halo_seq = p2p_next_halo(h->p2p);
      FB_TRY(spmv(h, 3, h->d.p, h->Ad.p, h->r.p, h->part_a.p, parity, &pa));
    } else {
      FB_TRY(halo_exchange(h, h->d.p));
      FB_TRY(spmv(h, 3, h->d.p, h->Ad.p, h->r.p, h->part_a.p, parity));
    }
    hipLaunchKernelGGL((k_cg_fused<true>), dim3(h->grid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->st.p, parity, h->part_a.p, h->sgrid,
                       (const double*)nullptr, h->Ad.p, h->invdiag.p, h->x.p, h->r.p, h->d.p, pa);
    FB_HIP(hipGetLastError());
    return FB_OK;
  }
  FB_TRY(halo_exchange(h, h->d.p));
  if (!refresh && (variant == FB_PCG_MERGED || variant == FB_PCG_PERSISTENT)) {
    // merged-reduction iteration: SpMV with the three sums, then one fused vector pass (one reduction / all-reduce)
    FB_TRY(spmv(h, 3, h->d.p, h->Ad.p, h->r.p, h->part_a.p, parity));
    FB_TRY(global_scalar(h, h->part_a.p, &sc, true, 3, 0, h->sgrid));
    hipLaunchKernelGGL((k_cg_fused<false>), dim3(h->vgrid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->st.p, parity, h->part_a.p, h->sgrid,
                       sc, h->Ad.p, h->invdiag.p, h->x.p, h->r.p, h->d.p, P2PArgs());
    FB_HIP(hipGetLastError());
    return FB_OK;
  }
  FB_TRY(spmv(h, 1, h->d.p, h->Ad.p, nullptr, h->part_a.p, parity));
  FB_TRY(global_scalar(h, h->part_a.p, &sc, true, 1, 0, h->sgrid));
  if (!refresh) {
    hipLaunchKernelGGL(k_cg_update<false>, dim3(h->grid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->st.p, parity,
                       h->part_a.p, h->sgrid, sc, h->d.p, h->Ad.p, h->invdiag.p, h->x.p, h->r.p, h->part_b.p);
    FB_HIP(hipGetLastError());
  } else {
    hipLaunchKernelGGL(k_cg_update<true>, dim3(h->grid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->st.p, parity,
                       h->part_a.p, h->sgrid, sc, h->d.p, h->Ad.p, h->invdiag.p, h->x.p, h->r.p, h->part_b.p);
    FB_HIP(hipGetLastError());
    FB_TRY(halo_exchange(h, h->x.p));
    FB_TRY(spmv(h, 2, h->x.p, h->r.p, b, h->part_b.p, parity));
  }
  FB_TRY(global_scalar(h, h->part_b.p, &sc, true, 1, 0, refresh ? h->sgrid : h->grid));
  // part_b comes from the exact-residual SpMV on refresh iterations, from the vector kernel otherwise
  hipLaunchKernelGGL(k_cg_direction, dim3(h->grid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->st.p, parity, h->part_b.p,
                     refresh ? h->sgrid : h->grid, sc, h->r.p, h->invdiag.p, h->d.p);
  FB_HIP(hipGetLastError());
  return FB_OK;
}


// captures iterations 1..30 (parity and the position of the exact-residual iteration repeat with period 30)
int ensure_batch_graph(fb_fem_s* h, const double* b, int batch) {
  if (h->batch_graph && h->graph_rhs == b && h->graph_literal == h->literal_now) return FB_OK;
  drop_graph(h);
  h->graph_literal = h->literal_now;
  hipGraph_t g = nullptr;
  FB_HIP(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  int rc = FB_OK;
  for (int k = 1; k <= batch && rc == FB_OK; k++) rc = pcg_iteration(h, k, b);
  const hipError_t e = hipStreamEndCapture(h->stream, &g);
  if (rc != FB_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
  if (e != hipSuccess || !g) return fail(FB_EDEVICE, "hipStreamEndCapture: %s", hipGetErrorString(e));
  const hipError_t ei = hipGraphInstantiate(&h->batch_graph, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ei != hipSuccess) { h->batch_graph = nullptr; return fail(FB_EDEVICE, "hipGraphInstantiate: %s", hipGetErrorString(ei)); }
  h->graph_rhs = b;
  return FB_OK;
}

bool host_finished(const CGState& s) {
  if (s.done) return true;
  const double rho = s.rho[s.iter & 1];
  return !(rho > s.eps2 * s.rho0) || s.iter >= s.max_iter;
}

// Jacobi-PCG on the assembled system, rhs b -> h->x.  iters_out: + converged / - not (CGSolver.cpp:189).
int pcg_solve(fb_fem_s* h, const double* b, double eps, int max_iter, int* iters_out, CGState* final_state, bool allow_persist = true);

// Jacobi-PCG inside persistent launches (normally ONE): CGSolver.cpp:129-190 in its pipelined form
int pcg_solve_pipe(fb_fem_s* h, const double* b, double eps, int max_iter, int* iters_out, CGState* final_state) {
  hipStream_t s = h->stream;
  const bool warm = h->pcg_warm;
  h->pcg_warm = false;
  int cut = max_iter + 1;  // iterations per launch: all of them (the kernel stops at convergence or max_iter)
  if (const char* e = getenv("FEMBRAIN_PERSIST_MAX_RUN")) cut = std::max(1, atoi(e));  // test knob: cut the solve into shorter launches
  int start = warm ? 2 : 1;
  CGState fin;
  memset(&fin, 0, sizeof fin);
  for (;;) {
    FB_TRY(launch_pipe(h, b, start, cut, eps, max_iter));
    h->ps.persist_launches++;
    unsigned int err = 0;
    FB_HIP(hipMemcpyAsync(&h->st_host[0], h->st.p, sizeof(CGState), hipMemcpyDeviceToHost, s));
    FB_HIP(hipMemcpyAsync(&err, h->ps.pipe_flags.p + h->ps.persist_blocks + h->ps.pipe_flag_extra + 4, sizeof err, hipMemcpyDeviceToHost, s));
    FB_HIP(hipStreamSynchronize(s));
    {
      float ms = 0;
      if (hipEventElapsedTime(&ms, h->ev_p[0], h->ev_p[1]) == hipSuccess) h->ps.persist_seconds += ms * 1e-3;
    }
    if (h->ps.shard_persist) {  // a time-out on any rank sends every rank to the two-launch solver, together
      std::vector<unsigned int> errs((size_t)h->plan.n_ranks);
      FB_TRY(comm_allgather_bytes(h->comm, &err, errs.data(), sizeof err, s));
      for (unsigned int e2 : errs) err |= e2;
    }
    if (err) {
      // A wait inside the launch gave up: the workgroups were not all resident (the device is shared with another process's
      // kernels?).  The launch wrote nothing back, so the solve is repeated from the same start with a launch per phase, and
      // this handle stays with that; fb_step_info.pcg_path / persist_fallbacks tell the host.
      FB_TRY(h->ps.pipe_flags.zero(s));
      FB_TRY(h->ps.pipe_post.zero(s));
      h->ps.persist = false;
      h->ps.persist_broken = true;
      h->ps.persist_fallbacks++;
      h->ps.clean_solves = 0;
      if (h->ps.persist_fallbacks > 1) h->ps.rearm_after = std::min(h->ps.rearm_after * 2, 1 << 20);
      if (getenv("FEMBRAIN_PERSIST_STRICT") && atoi(getenv("FEMBRAIN_PERSIST_STRICT")) != 0)
        return fail(FB_EDEVICE, "persistent PCG: a wait inside the launch timed out after %.1f ms (the workgroups were not all resident?)", h->ps.persist_timeout_ticks * 1e-5);
      fprintf(stderr, "[fembrain] persistent PCG: a wait timed out after %.1f ms; this handle falls back to the two-launch iteration\n", h->ps.persist_timeout_ticks * 1e-5);
      h->pcg_warm = warm;
      const int rc = pcg_solve(h, b, eps, max_iter, iters_out, final_state, false);
      h->last_pcg_path = FB_PCG_PATH_FALLBACK;
      return rc;
    }
    h->ps.persist_iterations += h->st_host[0].iter - (start == 0 ? fin.iter : 0);
    fin = h->st_host[0];
    if (fin.done) break;
    if (fin.iter > max_iter) return fail(FB_EDEVICE, "internal: persistent PCG ran past max_iter (iter %d)", fin.iter);
    start = 0;
  }
  if (h->ps.persist_timing.p && h->ps.pipe_rows == 1) print_pipe_timing(h);
  h->last_pcg_path = FB_PCG_PATH_PERSISTENT;
  const double rho = fin.rho[fin.iter & 1];
  const bool converged = !(rho > fin.eps2 * fin.rho0);
  if (!converged) {
    // The iteration cap was reached (CGSolver.cpp:189 returns -max_iter with the iterate it has).  The launch left its iterate in d and
    // the start vector in x.  One exact residual tells whether the pipelined recurrences were honest to the end: if the true
    // r . r / diag of the iterate is within a factor of four of what they carried, the system simply needs more iterations and the
    // iterate stands (a system that does not converge cost 2 x max_iter iterations).  Otherwise -- the recurrences
    // stalled or drifted -- the literal recurrences get the last word: the two-launch solver repeats the solve.  ("From the same start"
    // holds for a solve in ONE launch, the product's case; with the test knob FEMBRAIN_PERSIST_MAX_RUN the earlier launches have written
    // their iterate to x already, and the repeat continues from there as a warm start -- same answer to the tolerance, not the same bits.)
    const bool cap_check = !(getenv("FEMBRAIN_PERSIST_CAP_CHECK") && atoi(getenv("FEMBRAIN_PERSIST_CAP_CHECK")) == 0);  // (=0: always repeat; tests)
    if (cap_check && h->prm.pcg_variant != FB_PCG_BLOCK_JACOBI) {  // (block-Jacobi carries r . B^-1 r: not what the product kernel sums)
      FB_TRY(h->st.zero(s));  // done = 0: the product below is not a no-op
      FB_TRY(halo_exchange(h, h->d.p));
      FB_TRY(spmv(h, 2, h->d.p, h->r.p, b, h->part_b.p, 0));
      double* sc = nullptr;
      FB_TRY(global_scalar(h, h->part_b.p, &sc, false, 1, 0, h->sgrid));
      hipLaunchKernelGGL(k_cg_begin, dim3(1), dim3(kBlock), 0, s, h->st.p, h->part_b.p, h->sgrid, sc, eps, max_iter);
      FB_HIP(hipGetLastError());
      CGState chk;
      FB_HIP(hipMemcpyAsync(&chk, h->st.p, sizeof(CGState), hipMemcpyDeviceToHost, s));
      FB_HIP(hipStreamSynchronize(s));
      if (std::isfinite(chk.rho0) && chk.rho0 <= 4.0 * rho) {
        FB_HIP(hipMemcpyAsync(h->x.p, h->d.p, sizeof(double) * 3 * (size_t)h->plan.n_local, hipMemcpyDeviceToDevice, s));
        fin.rho[fin.iter & 1] = chk.rho0;  // (the exact one)
        // the device copy of the solver state says what the solve ended with, not what the check's k_cg_begin left there
        h->st_host[1] = fin;
        h->st_host[1].done = 1;
        FB_HIP(hipMemcpyAsync(h->st.p, &h->st_host[1], sizeof(CGState), hipMemcpyHostToDevice, s));
        FB_HIP(hipStreamSynchronize(s));
        if (iters_out) *iters_out = -fin.iter;
        if (final_state) *final_state = fin;
        return FB_OK;
      }
    }
    h->pcg_warm = warm;
    const int rc = pcg_solve(h, b, eps, max_iter, iters_out, final_state, false);
    h->last_pcg_path = FB_PCG_PATH_RESOLVED;
    return rc;
  }
  if (iters_out) *iters_out = converged ? fin.iter : -fin.iter;
  if (final_state) *final_state = fin;
  return FB_OK;
}

// The pipelined recurrences of the persistent solver stop making progress at a relative residual of ~1e-11 on these systems
// (measured, tools/pipelined_pcg_numerics.py and DESIGN.md; the literal recurrences go on below 1e-12): a solve asked for a
// tolerance within three orders of that goes to the two-launch solver, whatever the handle runs otherwise.
constexpr double kPersistMinEps = 1e-8;

int pcg_solve(fb_fem_s* h, const double* b, double eps, int max_iter, int* iters_out, CGState* final_state, bool allow_persist) {
  if (allow_persist && !h->ps.persist && h->ps.persist_broken && !h->ps.shard_persist && h->plan.n_ranks == 1 && h->ps.rearm_after > 0 && h->ps.clean_solves >= h->ps.rearm_after) {
    h->ps.persist = true;  // the set-up of the persistent solver is still in place (flags and sums were cleared when it fell back)
    h->ps.persist_broken = false;
    h->ps.persist_rearms++;
    read_persist_timeout(h);
    fprintf(stderr, "[fembrain] persistent PCG: re-armed after %d two-launch solves\n", h->ps.clean_solves);
  }
  if (allow_persist && h->ps.persist && eps >= kPersistMinEps &&
      (h->prm.pcg_variant == FB_PCG_MERGED || h->prm.pcg_variant == FB_PCG_PERSISTENT || h->prm.pcg_variant == FB_PCG_BLOCK_JACOBI))
    return pcg_solve_pipe(h, b, eps, max_iter, iters_out, final_state);
  if (allow_persist && h->ps.persist_broken) h->ps.clean_solves++;
  h->last_pcg_path = FB_PCG_PATH_TWO_LAUNCH;
  // The merged recurrence for rho (rho' = rho - 2 alpha S1 + alpha^2 S2) loses digits the literal sum r.r/diag keeps: measured on
  // the 17,576-node cube it stalls above 1e-12 where the literal sequence converges.  Tolerances below kPersistMinEps therefore run
  // the literal sequence of FB_PCG_REFERENCE, whatever variant the handle was made with (block-Jacobi is literal already).
  struct LiteralScope { fb_fem_s* h; ~LiteralScope() { h->literal_now = false; } } literal_scope{h};
  h->literal_now = eps < kPersistMinEps && (h->prm.pcg_variant == FB_PCG_MERGED || h->prm.pcg_variant == FB_PCG_PERSISTENT);
  const FemPlan& P = h->plan;
  hipStream_t s = h->stream;
  double* sc = nullptr;
  if (h->pcg_warm) {
    // start from the x the previous solve left (CGSolver.cpp:131-141 with a non-zero x): r = b - A x, d = r / diag
    h->pcg_warm = false;
    FB_TRY(h->st.zero(s));  // done = 0: the SpMV below is not a no-op
    FB_TRY(halo_exchange(h, h->x.p));
    FB_TRY(spmv(h, 2, h->x.p, h->r.p, b, h->part_b.p, 0));
    if (h->prm.pcg_variant == FB_PCG_BLOCK_JACOBI) {  // d = B^-1 r and rho = r . B^-1 r (the SpMV's Jacobi-weighted sum is not used)
      hipLaunchKernelGGL(k_bj_init_warm, dim3(h->grid), dim3(kBlock), 0, s, P.n_slices, P.n_owned, h->r.p, h->invblk.p, h->d.p, h->part_b.p);
      FB_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_cg_begin, dim3(1), dim3(kBlock), 0, s, h->st.p, h->part_b.p, h->grid, (const double*)nullptr, eps, max_iter);
    } else {
      hipLaunchKernelGGL(k_cg_init_warm, dim3(h->grid), dim3(kBlock), 0, s, P.n_slices, P.n_owned, h->r.p, h->invdiag.p, h->d.p);
      FB_HIP(hipGetLastError());
      FB_TRY(global_scalar(h, h->part_b.p, &sc, false, 1, 0, h->sgrid));
      hipLaunchKernelGGL(k_cg_begin, dim3(1), dim3(kBlock), 0, s, h->st.p, h->part_b.p, h->sgrid, sc, eps, max_iter);
    }
  } else if (h->prm.pcg_variant == FB_PCG_BLOCK_JACOBI) {
    hipLaunchKernelGGL(k_bj_init, dim3(h->grid), dim3(kBlock), 0, s, P.n_slices, P.n_owned, b, h->invblk.p, h->x.p, h->r.p, h->d.p, h->part_b.p);
    FB_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cg_begin, dim3(1), dim3(kBlock), 0, s, h->st.p, h->part_b.p, h->grid, (const double*)nullptr, eps, max_iter);
  } else {
    hipLaunchKernelGGL(k_cg_init, dim3(h->grid), dim3(kBlock), 0, s, P.n_slices, P.n_owned, b, h->invdiag.p, h->x.p, h->r.p, h->d.p,
                       h->part_b.p);
    FB_HIP(hipGetLastError());
    FB_TRY(global_scalar(h, h->part_b.p, &sc, false));
    hipLaunchKernelGGL(k_cg_begin, dim3(1), dim3(kBlock), 0, s, h->st.p, h->part_b.p, h->grid, sc, eps, max_iter);
  }
  FB_HIP(hipGetLastError());
  const int kBatch = 30;
  int it = 1, slot = 0;
  bool pending[2] = {false, false};
  CGState fin;
  memset(&fin, 0, sizeof fin);
  bool finished = false;
  // replay pays on small meshes only (us per iteration, replay vs launches: 8.2 vs 9.6 at 22k tets, 9.4 vs 9.8 at 105k,
  // 13.1 vs 12.9 at 257k, 29.4 vs 29.1 at 1M); sharded kernels carry sequence numbers and are launched one by one
  const bool graphable = h->use_graph && h->prm.pcg_variant != FB_PCG_BLOCK_JACOBI && P.n_slices <= 512 && (!h->comm || h->comm->n_ranks == 1);
  while (!finished) {
    const int n = std::min(kBatch, max_iter - it + 1);
    bool replayed = false;
    if (graphable && h->use_graph && n == kBatch && (it - 1) % kBatch == 0) {
      if (ensure_batch_graph(h, b, kBatch) == FB_OK && hipGraphLaunch(h->batch_graph, s) == hipSuccess) {
        replayed = true;
        it += kBatch;
      } else {  // capture or replay unavailable: plain launches from now on
        (void)hipGetLastError();
        drop_graph(h);
        h->use_graph = false;
      }
    }
    if (!replayed) {
      for (int k = 0; k < n; k++, it++) FB_TRY(pcg_iteration(h, it, b));
    }
    FB_HIP(hipMemcpyAsync(&h->st_host[slot], h->st.p, sizeof(CGState), hipMemcpyDeviceToHost, s));
    FB_HIP(hipEventRecord(h->ev_batch[slot], s));
    pending[slot] = true;
    const int prev = slot ^ 1;
    if (pending[prev]) {  // look one batch behind so the queue never drains
      FB_HIP(hipEventSynchronize(h->ev_batch[prev]));
      pending[prev] = false;
      if (host_finished(h->st_host[prev])) finished = true;
    }
    if (it > max_iter) finished = true;
    slot ^= 1;
  }
  FB_HIP(hipStreamSynchronize(s));
  if (h->p2p) FB_TRY(p2p_check(h->p2p, s));
  // the newest snapshot is in the slot written last
  fin = h->st_host[slot ^ 1];
  if (!host_finished(fin)) return fail(FB_EDEVICE, "internal: PCG batches ended without a terminal state (iter %d)", fin.iter);
  const double rho = fin.rho[fin.iter & 1];
  const bool converged = !(rho > fin.eps2 * fin.rho0);
  if (iters_out) *iters_out = converged ? fin.iter : -fin.iter;
  if (final_state) *final_state = fin;
  return FB_OK;
}

// inspection entry points (pattern, block values, mass) index the CSR pattern on the host
int ensure_host_pattern(fb_fem_s* h) {
  if (h->host_pattern) return FB_OK;
  FemPlan& P = h->plan;
  P.bptr.resize((size_t)P.n_owned + 1);
  P.bcol.resize((size_t)P.n_blocks);
  P.blk_slot.resize((size_t)P.n_blocks);
  FB_TRY(h->d_bptr.download(P.bptr.data(), P.bptr.size(), h->stream));
  FB_TRY(h->d_bcol.download(P.bcol.data(), P.bcol.size(), h->stream));
  FB_TRY(h->d_blk_slot.download(P.blk_slot.data(), P.blk_slot.size(), h->stream));
  h->host_pattern = true;
  return FB_OK;
}

// global-length host vector -> local device vector (owned + halo)
int upload_global_vec(fb_fem_s* h, const double* g, DevBuf<double>& dst) {
  const FemPlan& P = h->plan;
  if (P.n_ranks == 1 && h->ren.active) {  // caller order -> internal order on the device
    FB_TRY(h->io.reserve((size_t)3 * P.n_local));
    FB_HIP(hipMemcpyAsync(h->io.p, g, sizeof(double) * 3 * (size_t)P.n_local, hipMemcpyHostToDevice, h->stream));
    FB_TRY(gather_nodes(h->stream, P.n_local, 3, h->io.p, h->ren.d_old_of_new.p, dst.p));
    FB_HIP(hipStreamSynchronize(h->stream));
    return FB_OK;
  }
  if (P.n_ranks == 1) {
    FB_HIP(hipMemcpyAsync(dst.p, g, sizeof(double) * 3 * (size_t)P.n_local, hipMemcpyHostToDevice, h->stream));
    FB_HIP(hipStreamSynchronize(h->stream));
    return FB_OK;
  }
  std::vector<double> loc((size_t)3 * P.n_local);
  const int* ids = h->l2c.empty() ? P.local2global.data() : h->l2c.data();
  for (int l = 0; l < P.n_local; l++)
    for (int k = 0; k < 3; k++) loc[3 * (size_t)l + k] = g[3 * (size_t)ids[l] + k];
  FB_HIP(hipMemcpyAsync(dst.p, loc.data(), sizeof(double) * loc.size(), hipMemcpyHostToDevice, h->stream));
  FB_HIP(hipStreamSynchronize(h->stream));
  return FB_OK;
}


// host copies of the node maps of a renumbered handle (inspection entry points only)
int ensure_host_order(fb_fem_s* h) {
  if (!h->ren.active) return FB_OK;
  FB_TRY(h->ren.host_maps(h->stream));
  if (h->plan.n_ranks == 1) h->plan.local2global = h->ren.old_of_new;  // (a shard keeps its local -> internal map there, and l2c beside it)
  return FB_OK;
}

// The pattern in the caller's numbering (renumbered handles): row g of the caller = internal row new_of_old[g], its columns mapped
// back and sorted ascending -- fb_fem_pattern's contract -- with the internal block each of them is.
int ensure_caller_pattern(fb_fem_s* h) {
  FB_TRY(ensure_host_pattern(h));
  if (h->caller_pattern) return FB_OK;
  FB_TRY(ensure_host_order(h));
  const FemPlan& P = h->plan;
  h->c_bptr.assign((size_t)P.n_owned + 1, 0);
  h->c_bcol.resize((size_t)P.n_blocks);
  h->c_src.resize((size_t)P.n_blocks);
  std::vector<std::pair<int, int>> row;
  int at = 0;
  const bool shard = !h->l2c.empty();  // (a renumbered shard: rows in the order of fb_fem_owned_nodes, columns in the caller's ids)
  for (int g = 0; g < P.n_owned; g++) {
    const int a = shard ? g : h->ren.new_of_old[g];
    row.clear();
    for (int p = P.bptr[a]; p < P.bptr[a + 1]; p++) row.emplace_back(shard ? h->l2c[P.bcol[p]] : P.local2global[P.bcol[p]], p);
    std::sort(row.begin(), row.end());
    for (const auto& e : row) { h->c_bcol[at] = e.first; h->c_src[at] = e.second; at++; }
    h->c_bptr[(size_t)g + 1] = at;
  }
  h->caller_pattern = true;
  return FB_OK;
}


// SELL device values -> 9 doubles per block in CSR (fb_fem_pattern) order (diagonal blocks: hi + lo)
int download_blocks(fb_fem_s* h, double* out) {
  FB_TRY(ensure_host_pattern(h));
  const FemPlan& P = h->plan;
  const size_t n = (size_t)P.n_slots * 9 * 64, nl = (size_t)P.n_slices * 9 * 64;
  std::vector<double> host(n), lo(nl);
  if (h->f64) {
    FB_HIP(hipMemcpyAsync(host.data(), h->vals.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    FB_HIP(hipMemcpyAsync(lo.data(), h->dlo.p, nl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    FB_HIP(hipStreamSynchronize(h->stream));
  } else {
    std::vector<float> hf(n), lf(nl);
    FB_HIP(hipMemcpyAsync(hf.data(), h->vals.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    FB_HIP(hipMemcpyAsync(lf.data(), h->dlo.p, nl * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    FB_HIP(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; i++) host[i] = hf[i];
    for (size_t i = 0; i < nl; i++) lo[i] = lf[i];
  }
  const bool mapped = h->ren.active;
  std::vector<double> internal;
  if (mapped) {
    FB_TRY(ensure_caller_pattern(h));
    internal.resize((size_t)9 * P.n_blocks);
  }
  double* dst = mapped ? internal.data() : out;
  for (int a = 0; a < P.n_owned; a++)
    for (int p = P.bptr[a]; p < P.bptr[a + 1]; p++)
      for (int v = 0; v < 9; v++) {
        double x = host[((size_t)P.blk_slot[p] * 9 + v) * 64 + (a & 63)];
        if (P.bcol[p] == a) x += lo[((size_t)(a >> 6) * 9 + v) * 64 + (a & 63)];
        dst[9 * (size_t)p + v] = x;
      }
  if (mapped)
    for (int pc = 0; pc < P.n_blocks; pc++) memcpy(out + 9 * (size_t)pc, internal.data() + 9 * (size_t)h->c_src[pc], 9 * sizeof(double));
  return FB_OK;
}

}  // namespace

extern "C" {

const char* fb_last_error(void) { return last_error().c_str(); }

int fb_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int fb_device_info(int dev, char* name, int name_len, char* arch, int arch_len, int* n_cu) {
  hipDeviceProp_t p;
  FB_HIP(hipGetDeviceProperties(&p, dev));
  if (name && name_len > 0) snprintf(name, name_len, "%s", p.name);
  if (arch && arch_len > 0) snprintf(arch, arch_len, "%s", p.gcnArchName);
  if (n_cu) *n_cu = p.multiProcessorCount;
  return FB_OK;
}

int fb_host_register(void* p, unsigned long long bytes) {
  if (!p || bytes == 0) return fail(FB_EINVAL, "null argument");
  const hipError_t e = hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(FB_EDEVICE, "hipHostRegister(%llu bytes): %s", bytes, hipGetErrorString(e)); }
  return FB_OK;
}

int fb_host_unregister(void* p) {
  if (!p) return FB_OK;
  const hipError_t e = hipHostUnregister(p);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(FB_EDEVICE, "hipHostUnregister: %s", hipGetErrorString(e)); }
  return FB_OK;
}

void fb_fem_default_params(fb_fem_params* p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->E = 1e7; p->nu = 0.46; p->rho = 1000.0;
  p->timestep = 0.0333; p->damping_mass = 0.0; p->damping_stiffness = 0.01;
  p->cg_eps = 1e-6; p->cg_max_iter = 10000;
  p->matrix_precision = FB_MATRIX_AUTO; p->device = 0;
}

int fb_fem_transport(fb_fem_t h) {
  if (!h) return -1;
  if (!h->comm || h->comm->n_ranks == 1) return 0;
  return h->xch_mode;
}

int fb_fem_set_exchange_mode(fb_fem_t h, int mode) {
  CHECK_HANDLE(h);
  if (!h->comm || h->comm->n_ranks == 1) return fail(FB_EINVAL, "an unsharded handle has no exchange");
  if (mode < FB_XCH_COLLECTIVE || mode > FB_XCH_P2P_FUSED) return fail(FB_EINVAL, "exchange mode %d", mode);
  if (mode >= FB_XCH_P2P && !h->p2p) return fail(FB_ECOMM, "the peer-to-peer transport is not attached (mapping failed or FEMBRAIN_P2P=0)");
  if (mode == FB_XCH_COLLECTIVE && !h->comm->nccl && !h->comm->local) return fail(FB_ECOMM, "the communicator has no collective library");
  FB_HIP(hipStreamSynchronize(h->stream));
  h->xch_mode = mode;
  return FB_OK;
}

// ---- fb_fem_surface (surface.h) ----
namespace {
int surface_ready(fb_fem_s* h, bool force) {
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_surface is for unsharded handles");
  if (h->surf.valid && !force) return FB_OK;
  SlackScope slack(handle_slack(h, h->plan.n_global, h->plan.n_tets));
  const char* wk = getenv("FEMBRAIN_SURFACE_WIDE_KEYS");  // read at every build, like FEMBRAIN_PLAN_KEYS64
  return surface_build(h->stream, h->surf, h->plan.n_global, h->plan.n_tets, h->tets.p, h->x0.p, h->ren.active ? h->ren.d_old_of_new.p : nullptr,
                       h->ren.active ? h->ren.d_new_of_old.p : nullptr, wk && atoi(wk) != 0, h->plan_ws);
}
void surface_fill(const SurfaceWork& S, const float* box, fb_fem_surface_info* out) {
  if (!out) return;
  out->n_faces = S.n_faces; out->n_vertices = S.n_vertices; out->n_builds = S.n_builds;
  for (int k = 0; k < 3; k++) { out->aabb_lo[k] = box[k]; out->aabb_hi[k] = box[3 + k]; }
}
}  // namespace

extern "C++" {
namespace fb {  // for stress.hip
int handle_slack_now(const fb_fem_s* h) { return handle_slack(h, h->plan.n_global, h->plan.n_tets); }
int surface_current(fb_fem_s* h) { return surface_ready(h, false); }
// for detach.hip: what fb_fem_set_internal_force_scaling, fb_fem_set_materials and fb_fem_set_element_materials leave in a handle, from
// src's values and an id array filled on the device.  As there, the table and the kernels first and the map last: a failure leaves no map.
int inherit_materials(fb_fem_s* h, const fb_fem_s* src, DevBuf<unsigned char>* ids) {
  const double scale_before = h->force_scale;
  h->force_scale = src->force_scale;  // (the device table is made under it)
  if (ids) {
    int rc = upload_material_table(h, (int)src->mat_E.size(), src->mat_E.data(), src->mat_nu.data(), src->mat_rho.data());
    if (rc == FB_OK) rc = resolve_asm_kernels(h, true);
    if (rc != FB_OK) { h->force_scale = scale_before; return rc; }  // (the host side as it was)
    h->mat_ids.swap(*ids);
    h->mat_hi = src->mat_hi;  // (an upper bound of the ids in use, as in src)
  }
  h->mat_E = src->mat_E; h->mat_nu = src->mat_nu; h->mat_rho = src->mat_rho;
  lame_of(h->prm.E * h->force_scale, h->prm.nu, &h->lambda, &h->mu);
  h->system_valid = false;
  h->mass_valid = false;
  return FB_OK;
}
}  // namespace fb
}  // extern "C++"

int fb_fem_surface(fb_fem_t h, fb_fem_surface_info* out) {
  CHECK_HANDLE(h);
  FB_TRY(surface_ready(h, false));
  surface_fill(h->surf, h->surf.rest_box, out);
  return FB_OK;
}

int fb_fem_read_surface(fb_fem_t h, int* faces, int* vertex_ids, int* face_tets) {
  CHECK_HANDLE(h);
  FB_TRY(surface_ready(h, false));
  const SurfaceWork& S = h->surf;
  if (faces) FB_TRY(S.faces.download(faces, (size_t)3 * S.n_faces, h->stream));
  if (vertex_ids) FB_TRY(S.vertex_ids.download(vertex_ids, (size_t)S.n_vertices, h->stream));
  if (face_tets) FB_TRY(S.face_tets.download(face_tets, (size_t)S.n_faces, h->stream));
  return FB_OK;
}

int fb_fem_surface_update(fb_fem_t h, float* xyz, float* normals, fb_fem_surface_info* out) {
  CHECK_HANDLE(h);
  FB_TRY(surface_ready(h, false));
  SurfaceWork& S = h->surf;
  const size_t nv = (size_t)S.n_vertices;
  const float zero[6] = {0, 0, 0, 0, 0, 0};
  if (!nv) { surface_fill(S, zero, out); return FB_OK; }
  FB_TRY(surface_update(h->stream, S, h->x0.p, h->q.p, true));
  if (xyz) memcpy(xyz, S.host.data(), sizeof(float) * 3 * nv);
  if (normals) memcpy(normals, S.host.data() + 3 * nv, sizeof(float) * 3 * nv);
  surface_fill(S, S.host.data() + 6 * nv, out);
  return FB_OK;
}

int fb_fem_time_surface(fb_fem_t h, int reps, double* seconds_build, double* seconds_update) {
  CHECK_HANDLE(h);
  if (reps < 1) return fail(FB_EINVAL, "reps must be positive");
  FB_TRY(surface_ready(h, false));  // warm: the buffers exist
  if (seconds_build) FB_TRY(timed_median(h, reps, [&] { return surface_ready(h, true); }, seconds_build));
  if (seconds_update) FB_TRY(timed_median(h, reps, [&] { return surface_update(h->stream, h->surf, h->x0.p, h->q.p, true); }, seconds_update));
  return FB_OK;
}

int fb_fem_rebuild_elements(fb_fem_t h) {
  CHECK_HANDLE(h);
  h->system_valid = false;
  return launch_rest(h);
}

int fb_fem_set_external_forces(fb_fem_t h, const double* f) {
  CHECK_HANDLE(h);
  if (!f) return fail(FB_EINVAL, "null force vector");
  return upload_global_vec(h, f, h->fext);
}

int fb_fem_add_external_forces(fb_fem_t h, const double* f) {
  CHECK_HANDLE(h);
  if (!f) return fail(FB_EINVAL, "null force vector");
  FB_TRY(upload_global_vec(h, f, h->tmp));
  const int n = 3 * h->plan.n_local;
  hipLaunchKernelGGL(k_axpy, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, h->stream, n, 1.0, h->tmp.p, h->fext.p);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_fem_set_external_forces_zero(fb_fem_t h) {
  CHECK_HANDLE(h);
  return h->fext.zero(h->stream);
}

int fb_fem_get_external_forces(fb_fem_t h, double* f) {
  CHECK_HANDLE(h);
  if (!f) return fail(FB_EINVAL, "null force vector");
  return download_owned(h, h->fext, f);
}

int fb_fem_set_uniform_force(fb_fem_t h, int axis, double value) {
  CHECK_HANDLE(h);
  if (axis < 0 || axis > 2) return fail(FB_EINVAL, "axis %d", axis);
  const int n = h->plan.n_local;
  hipLaunchKernelGGL(k_fill_axis, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, h->stream, n, axis, value, h->fext.p);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

namespace {
// what a step reports, for both integrators (the times are those of h->last_assembly_s / last_solve_s)
void fill_step_info(const fb_fem_s* h, fb_step_info* info, int iterations, bool ok, const CGState& fin, int newton) {
  if (!info) return;
  info->cg_iterations = iterations;
  info->converged = ok ? 1 : 0;
  info->assembly_seconds = h->last_assembly_s;
  info->solve_seconds = h->last_solve_s;
  info->rho0 = fin.rho0;
  info->rho = fin.rho[fin.iter & 1];
  info->pcg_path = h->last_pcg_path;
  info->persist_fallbacks = h->ps.persist_fallbacks;
  info->newton_iterations = newton;
}

// ImplicitNewmarkSparse::DoTimestep (implicitNewmarkSparse.cpp:183-379), PCG solver
int newmark_step(fb_fem_s* h, fb_step_info* info) {
  hipStream_t s = h->stream;
  const int n = 3 * h->plan.n_owned;
  const double hh = h->prm.timestep, beta = h->nm_beta, gamma = h->nm_gamma;
  NewmarkAlphas al;
  al.a1 = 1.0 / (beta * hh * hh); al.a2 = 1.0 / (beta * hh); al.a3 = (1.0 - 2.0 * beta) / (2.0 * beta);
  al.a4 = gamma / (beta * hh); al.a5 = 1 - gamma / beta; al.a6 = (1.0 - gamma / (2.0 * beta)) * hh;
  FB_HIP(hipEventRecord(h->ev[0], s));
  const size_t bytes = sizeof(double) * (size_t)n;
  FB_HIP(hipMemcpyAsync(h->q1.p, h->q.p, bytes, hipMemcpyDeviceToDevice, s));
  FB_HIP(hipMemcpyAsync(h->qvel1.p, h->qvel.p, bytes, hipMemcpyDeviceToDevice, s));
  FB_HIP(hipMemcpyAsync(h->qacc1.p, h->qacc.p, bytes, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(k_newmark_update, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, s, n, (const double*)nullptr, h->dofmask.p, al, h->q1.p, h->qvel1.p, h->qacc1.p,
                     h->q.p, h->qvel.p, h->qacc.p);
  FB_HIP(hipGetLastError());
  int total = 0, newton = 0;
  double error0 = 0.0, asm_s = 0.0, solve_s = 0.0;
  CGState fin;
  memset(&fin, 0, sizeof fin);
  bool ok = true;
  do {
    FB_HIP(hipEventRecord(h->ev[0], s));
    FB_TRY(assemble_system(h));
    // Newton error test on the residual, summed over ALL DOFs as implicitNewmarkSparse.cpp:258-262 does before RemoveRows -- the reaction
    // forces at the clamped DOFs included: the assembly leaves the unmasked residual in res_all beside the right-hand side (whose clamped
    // rows are 0, identity rows here).  (Rounds 2-4 summed the right-hand side, i.e. the free DOFs only, and could stop an iteration early.)
    // FemBrain itself runs one Newton iteration (Deformable.cpp:205-214).
    if (h->nm_max_newton > 1) {
      hipLaunchKernelGGL(k_sumsq, dim3(1), dim3(kBlock), 0, s, (size_t)n, h->res_all.p, h->scal.p + 4);
      FB_HIP(hipGetLastError());
      double err = 0.0;
      FB_HIP(hipMemcpyAsync(&err, h->scal.p + 4, sizeof err, hipMemcpyDeviceToHost, s));
      FB_HIP(hipStreamSynchronize(s));
      if (h->comm && h->comm->n_ranks > 1) return fail(FB_EINVAL, "Newmark with more than one Newton iteration is not built for sharded handles");
      if (newton == 0) error0 = err;
      else if (err / error0 < h->nm_eps * h->nm_eps) break;
    }
    FB_HIP(hipEventRecord(h->ev[1], s));
    int iters = 0;
    h->pcg_warm = true;  // `buffer` is not cleared between solves (implicitNewmarkSparse.cpp:317-320)
    FB_TRY(pcg_solve(h, h->rhs.p, h->prm.cg_eps, h->prm.cg_max_iter, &iters, &fin));
    FB_HIP(hipEventRecord(h->ev[2], s));
    total += std::abs(iters);
    if (iters < 0) { ok = false; break; }
    hipLaunchKernelGGL(k_newmark_update, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, s, n, h->x.p, h->dofmask.p, al, h->q1.p, h->qvel1.p, h->qacc1.p, h->q.p,
                       h->qvel.p, h->qacc.p);
    FB_HIP(hipGetLastError());
    FB_HIP(hipStreamSynchronize(s));
    float ms_a = 0, ms_s = 0;
    FB_HIP(hipEventElapsedTime(&ms_a, h->ev[0], h->ev[1]));
    FB_HIP(hipEventElapsedTime(&ms_s, h->ev[1], h->ev[2]));
    asm_s += ms_a * 1e-3; solve_s += ms_s * 1e-3;
    newton++;
  } while (newton < h->nm_max_newton);
  FB_HIP(hipStreamSynchronize(s));
  h->system_valid = false;
  h->last_assembly_s = asm_s; h->last_solve_s = solve_s;
  fill_step_info(h, info, total, ok, fin, newton);
  if (!ok) return fail(FB_ESOLVER, "PCG sparse solver returned non-zero exit status %d", -total);
  return FB_OK;
}
}  // namespace

int fb_fem_set_newmark(fb_fem_t h, double beta, double gamma, int max_newton_iterations, double epsilon) {
  CHECK_HANDLE(h);
  if (!(beta > 0) || !(gamma > 0) || max_newton_iterations < 1 || !(epsilon >= 0)) return fail(FB_EINVAL, "bad Newmark parameters");
  if (h->prm.integrator != FB_INTEGRATOR_NEWMARK) return fail(FB_EINVAL, "the handle was not created with fb_fem_params.integrator = FB_INTEGRATOR_NEWMARK");
  if (max_newton_iterations > 1 && h->comm && h->comm->n_ranks > 1)
    return fail(FB_EINVAL, "Newmark with more than one Newton iteration is not built for sharded handles (the error quotient is a global sum)");
  h->nm_beta = beta; h->nm_gamma = gamma; h->nm_max_newton = max_newton_iterations; h->nm_eps = epsilon;
  h->system_valid = false;
  return FB_OK;
}

int fb_fem_step(fb_fem_t h, fb_step_info* info) {
  CHECK_HANDLE(h);
  if (h->prm.integrator == FB_INTEGRATOR_NEWMARK) return newmark_step(h, info);
  hipStream_t s = h->stream;
  FB_HIP(hipEventRecord(h->ev[0], s));
  FB_TRY(assemble_system(h));
  const bool moved = motion_active(h);  // constrained DOFs that follow targets (motion.hip): a right-hand side correction, reactions, their own state
  if (moved) FB_TRY(motion_correct_rhs(h));
  FB_HIP(hipEventRecord(h->ev[1], s));
  int iters = 0;
  CGState fin;
  FB_TRY(pcg_solve(h, h->rhs.p, h->prm.cg_eps, h->prm.cg_max_iter, &iters, &fin));
  FB_HIP(hipEventRecord(h->ev[2], s));
  const bool ok = iters >= 0;
  if (ok) {
    if (moved) FB_TRY(motion_reactions(h));
    const int n = 3 * h->plan.n_owned;
    hipLaunchKernelGGL(k_state_update, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, s, n, h->x.p, h->dofmask.p, h->prm.timestep, h->q.p,
                       h->qvel.p);
    FB_HIP(hipGetLastError());
    if (moved) FB_TRY(motion_apply(h));
  }
  FB_HIP(hipStreamSynchronize(s));
  float ms_a = 0, ms_s = 0;
  FB_HIP(hipEventElapsedTime(&ms_a, h->ev[0], h->ev[1]));
  FB_HIP(hipEventElapsedTime(&ms_s, h->ev[1], h->ev[2]));
  h->last_assembly_s = ms_a * 1e-3; h->last_solve_s = ms_s * 1e-3;
  fill_step_info(h, info, std::abs(iters), ok, fin, 1);
  if (!ok) return fail(FB_ESOLVER, "PCG sparse solver returned non-zero exit status %d", iters);
  return FB_OK;
}

int fb_fem_get_state(fb_fem_t h, double* q, double* qvel, double* qaccel) {
  CHECK_HANDLE(h);
  if (q) FB_TRY(download_owned(h, h->q, q));
  if (qvel) FB_TRY(download_owned(h, h->qvel, qvel));
  if (qaccel && h->prm.integrator == FB_INTEGRATOR_NEWMARK) FB_TRY(download_owned(h, h->qacc, qaccel));
  else if (qaccel && !h->l2c.empty()) {
    for (int l = 0; l < h->plan.n_owned; l++) memset(qaccel + 3 * (size_t)h->l2c[l], 0, 3 * sizeof(double));
  } else if (qaccel && h->ren.active) memset(qaccel, 0, sizeof(double) * 3 * (size_t)h->plan.n_global);
  else if (qaccel) memset(qaccel + 3 * (size_t)h->plan.node_lo, 0, sizeof(double) * 3 * (size_t)h->plan.n_owned);  // forced 0, PS_VolumeConservingIntegrator.cpp:55
  return FB_OK;
}

int fb_fem_set_state(fb_fem_t h, const double* q, const double* qvel, const double* qaccel) {
  CHECK_HANDLE(h);
  if (!q) return fail(FB_EINVAL, "q must not be null (IntegratorBase::SetqState)");
  FB_TRY(upload_global_vec(h, q, h->q));
  if (qvel) FB_TRY(upload_global_vec(h, qvel, h->qvel));
  if (qaccel && h->prm.integrator == FB_INTEGRATOR_NEWMARK) FB_TRY(upload_global_vec(h, qaccel, h->qacc));
  h->system_valid = false;
  return FB_OK;
}

int fb_fem_reset(fb_fem_t h) {
  CHECK_HANDLE(h);
  FB_TRY(h->q.zero(h->stream));
  FB_TRY(h->qvel.zero(h->stream));
  if (h->prm.integrator == FB_INTEGRATOR_NEWMARK) {
    FB_TRY(h->qacc.zero(h->stream));
    FB_TRY(h->x.zero(h->stream));  // the solver's start vector (IntegratorBase::ResetToRest clears its buffers)
  }
  h->system_valid = false;
  motion_clear(h->motion);
  return FB_OK;
}

int fb_fem_set_timestep(fb_fem_t h, double timestep) {
  CHECK_HANDLE(h);
  if (!(timestep > 0) || !std::isfinite(timestep)) return fail(FB_EINVAL, "timestep must be positive and finite");
  h->prm.timestep = timestep;
  h->system_valid = false;
  return FB_OK;
}

int fb_fem_set_damping(fb_fem_t h, double damping_mass, double damping_stiffness) {
  CHECK_HANDLE(h);
  // (finite negative coefficients stay accepted, as the reference accepts them; a NaN or an infinity would poison s_m / s_k)
  if (!std::isfinite(damping_mass) || !std::isfinite(damping_stiffness)) return fail(FB_EINVAL, "damping coefficients must be finite");
  h->prm.damping_mass = damping_mass; h->prm.damping_stiffness = damping_stiffness;
  h->system_valid = false;
  return FB_OK;
}

int fb_fem_set_internal_force_scaling(fb_fem_t h, double factor) {
  CHECK_HANDLE(h);
  if (!(factor > 0) || !std::isfinite(factor)) return fail(FB_EINVAL, "internal force scaling factor must be positive");
  // f_int and K are linear in Young's modulus, so scaling both (integratorBase.cpp:46, implicitNewmarkSparse.cpp:200-204;
  // PS_VolumeConservingIntegrator.cpp:84-90) is scaling the Lame parameters the element kernels use
  // (every material's E: the table of a handle with an element map is made again)
  const double before = h->force_scale;
  h->force_scale = factor;
  const int rc = refresh_materials(h, false);  // (the mass does not depend on E)
  if (rc != FB_OK) h->force_scale = before;
  return rc;
}

// ---- per-element materials ----
int fb_fem_set_materials(fb_fem_t h, int n_materials, const double* E, const double* nu, const double* rho) {
  CHECK_HANDLE(h);
  if (n_materials < 1 || n_materials > kMaxMaterials) return fail(FB_EINVAL, "a material table has 1 to %d entries, not %d", kMaxMaterials, n_materials);
  if (!E || !nu || !rho) return fail(FB_EINVAL, "null material array");
  for (int i = 0; i < n_materials; i++)  // what VolumetricMesh's parser accepts (volumetricMesh.cpp:327): E > 0, -1 < nu < 0.5, rho > 0
    if (!(E[i] > 0) || !(nu[i] > -1.0 && nu[i] < 0.5) || !(rho[i] > 0) || !std::isfinite(E[i]) || !std::isfinite(nu[i]) || !std::isfinite(rho[i]))
      return fail(FB_EINVAL, "material %d: E = %g, nu = %g, rho = %g (E > 0, -1 < nu < 0.5, rho > 0, all finite)", i, E[i], nu[i], rho[i]);
  if (h->plan.n_ranks > 1 && n_materials > 1) return fail(FB_EINVAL, "a sharded handle has one material");
  if (n_materials <= h->mat_hi) return fail(FB_EINVAL, "elements use material ids up to %d: the table cannot shrink to %d entries", h->mat_hi, n_materials);
  // the device table first (on the handle's stream, behind the launches that read the old one): if that fails the host side is untouched
  if (has_material_map(h)) FB_TRY(upload_material_table(h, n_materials, E, nu, rho));
  h->mat_E.assign(E, E + n_materials); h->mat_nu.assign(nu, nu + n_materials); h->mat_rho.assign(rho, rho + n_materials);
  h->prm.E = E[0]; h->prm.nu = nu[0]; h->prm.rho = rho[0];
  lame_of(h->prm.E * h->force_scale, h->prm.nu, &h->lambda, &h->mu);
  h->system_valid = false;
  h->mass_valid = false;
  return FB_OK;
}

int fb_fem_num_materials(fb_fem_t h) { return h ? (int)h->mat_E.size() : 0; }

int fb_fem_read_materials(fb_fem_t h, double* E, double* nu, double* rho) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  for (size_t i = 0; i < h->mat_E.size(); i++) {
    if (E) E[i] = h->mat_E[i];
    if (nu) nu[i] = h->mat_nu[i];
    if (rho) rho[i] = h->mat_rho[i];
  }
  return FB_OK;
}

int fb_fem_set_element_materials(fb_fem_t h, int first, int count, const unsigned char* ids) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "a sharded handle has one material: no element map");
  const int nt = h->plan.n_tets;
  if (first < 0 || count < 0 || first > nt || count > nt - first) return fail(FB_EINVAL, "element range [%d,%d) outside [0,%d)", first, first + count, nt);
  if (count && !ids) return fail(FB_EINVAL, "null id array");
  const int n = (int)h->mat_E.size();
  int hi = 0;
  for (int k = 0; k < count; k++) {  // on the host, before anything is uploaded: no kernel sees an id outside the table
    if (ids[k] >= n) return fail(FB_EINVAL, "element %d: material id %d, the table has %d entries", first + k, (int)ids[k], n);
    hi = std::max(hi, (int)ids[k]);
  }
  if (count == 0) return FB_OK;
  if (!has_material_map(h)) {
    if (hi == 0) return FB_OK;  // (every element is material 0 already: still no map)
    // The first map.  The table, the filled id array and the material-aware kernels (resolve_asm_kernels) are made first and the array becomes the
    // handle's LAST: mat_ids is what says "this handle has a map", so a failure on the way leaves a handle without one, as it was.
    FB_TRY(upload_material_table(h, n, h->mat_E.data(), h->mat_nu.data(), h->mat_rho.data()));
    SlackScope slack(handle_slack(h, h->plan.n_global, nt));  // the handle's slack rule, as for the element buffers
    DevBuf<unsigned char> fresh;
    FB_TRY(fresh.alloc((size_t)std::max(1, nt)));
    FB_TRY(fresh.zero(h->stream));
    FB_HIP(hipMemcpyAsync(fresh.p + first, ids, (size_t)count, hipMemcpyHostToDevice, h->stream));
    FB_HIP(hipStreamSynchronize(h->stream));
    FB_TRY(resolve_asm_kernels(h, true));
    h->mat_ids.swap(fresh);
  } else {
    FB_HIP(hipMemcpyAsync(h->mat_ids.p + first, ids, (size_t)count, hipMemcpyHostToDevice, h->stream));
    FB_HIP(hipStreamSynchronize(h->stream));
  }
  h->mat_hi = std::max(h->mat_hi, hi);
  h->system_valid = false;
  h->mass_valid = false;
  return FB_OK;
}

int fb_fem_read_element_materials(fb_fem_t h, int first, int count, unsigned char* ids) {
  CHECK_HANDLE(h);
  const int nt = h->plan.n_tets;
  if (first < 0 || count < 0 || first > nt || count > nt - first) return fail(FB_EINVAL, "element range [%d,%d) outside [0,%d)", first, first + count, nt);
  if (count && !ids) return fail(FB_EINVAL, "null id array");
  if (!has_material_map(h)) { if (count) memset(ids, 0, (size_t)count); return FB_OK; }
  return h->mat_ids.download(ids, (size_t)count, h->stream, (size_t)first);
}

long long fb_fem_element_map_bytes(fb_fem_t h) { return h && has_material_map(h) ? (long long)(h->mat_ids.cap * sizeof(unsigned char)) : 0; }

int fb_fem_set_cg(fb_fem_t h, double eps, int max_iter) {
  CHECK_HANDLE(h);
  if (!(eps > 0) || max_iter < 0) return fail(FB_EINVAL, "bad PCG parameters");
  h->prm.cg_eps = eps; h->prm.cg_max_iter = max_iter;
  return FB_OK;
}

int fb_fem_floor_collision(fb_fem_t h, double floor_y, double restitution, int* n_collided) {
  CHECK_HANDLE(h);
  FB_TRY(h->counter.zero(h->stream));
  const int n = h->plan.n_owned;
  hipLaunchKernelGGL(k_floor, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, h->stream, n, h->x0.p, floor_y, restitution, h->q.p,
                     h->qvel.p, h->counter.p);
  FB_HIP(hipGetLastError());
  int c = 0;
  FB_TRY(h->counter.download(&c, 1, h->stream));
  if (n_collided) *n_collided = c;
  h->system_valid = false;
  return FB_OK;
}

int fb_fem_plan_on_device(fb_fem_t h) { return h && h->device_plan ? 1 : 0; }
int fb_fem_assembly_kernel(fb_fem_t h) { return h && h->asm_tets ? (h->asm_staged ? 2 : 1) : 0; }
int fb_fem_assembly_wide_slices(fb_fem_t h) { return h && h->asm_tets ? h->asm_wide : 0; }

long long fb_fem_device_plan_get(fb_fem_t h, const char* name, int* out, long long capacity) {
  CHECK_HANDLE(h);
  if (!name) return fail(FB_EINVAL, "null name");
  const FemPlan& P = h->plan;
  const std::string n(name);
  const void* src = nullptr;
  long long cnt = 0;
  if (n == "slice_off") { src = h->slice_off.p; cnt = P.n_slices + 1; }
  else if (n == "colidx") { src = h->colidx.p; cnt = (long long)P.n_slots * kSliceRows; }
  else if (n == "slot_coff") { src = h->slot_coff.p; cnt = P.n_slots; }
  else if (n == "slot_ccnt") { src = h->slot_ccnt.p; cnt = P.n_slots; }
  else if (n == "contrib") { src = h->contrib.p; cnt = (long long)P.n_crows * kSliceRows; }
  else if (h->device_plan && n == "bptr") { src = h->d_bptr.p; cnt = P.n_owned + 1; }
  else if (h->device_plan && n == "bcol") { src = h->d_bcol.p; cnt = P.n_blocks; }
  else if (h->device_plan && n == "blk_slot") { src = h->d_blk_slot.p; cnt = P.n_blocks; }
  else {
    // the persistent solver's plan (fem_persist.hip): assembled on the host
    std::vector<int> v;
    const int got = persist_plan_array(h, name, &v);
    if (got < 0) return got;
    if (!got) return fail(FB_EINVAL, "no device plan array '%s'", name);
    if (out && capacity > 0) memcpy(out, v.data(), sizeof(int) * (size_t)std::min<long long>((long long)v.size(), capacity));
    return (long long)v.size();
  }
  if (out && capacity > 0 && cnt > 0) {
    FB_HIP(hipMemcpyAsync(out, src, sizeof(int) * (size_t)std::min(cnt, capacity), hipMemcpyDeviceToHost, h->stream));
    FB_HIP(hipStreamSynchronize(h->stream));
  }
  return cnt;
}

int fb_fem_num_nodes(fb_fem_t h) { return h ? h->plan.n_global : 0; }
int fb_fem_num_tets(fb_fem_t h) { return h ? h->plan.n_tets : 0; }
int fb_fem_num_blocks(fb_fem_t h) { return h ? h->plan.n_blocks : 0; }
int fb_fem_matrix_precision(fb_fem_t h) { return h && h->f64 ? FB_MATRIX_F64 : FB_MATRIX_F32; }
int fb_fem_owned_range(fb_fem_t h, int lo_hi[2]) {
  if (!h || !lo_hi) return fail(FB_EINVAL, "null argument");
  lo_hi[0] = h->plan.node_lo; lo_hi[1] = h->plan.node_hi;
  return FB_OK;
}

int fb_fem_pattern(fb_fem_t h, int* bptr, int* bcol) {
  if (!h || !bptr || !bcol) return fail(FB_EINVAL, "null argument");
  FB_HIP(hipSetDevice(h->prm.device));
  FB_TRY(ensure_host_pattern(h));
  const FemPlan& P = h->plan;
  if (h->ren.active) {
    FB_TRY(ensure_caller_pattern(h));
    memcpy(bptr, h->c_bptr.data(), sizeof(int) * (P.n_owned + 1));
    memcpy(bcol, h->c_bcol.data(), sizeof(int) * (size_t)P.n_blocks);
    return FB_OK;
  }
  memcpy(bptr, P.bptr.data(), sizeof(int) * (P.n_owned + 1));
  for (int p = 0; p < P.n_blocks; p++) bcol[p] = P.local2global[P.bcol[p]];
  return FB_OK;
}

int fb_fem_halo_info(fb_fem_t h, int* n_halo_nodes, int* n_neighbour_ranks) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  const FemPlan& P = h->plan;
  if (n_halo_nodes) *n_halo_nodes = P.n_local - P.n_owned;
  int nb = 0;
  for (int q = 0; q + 1 < (int)P.halo_off.size(); q++) nb += P.halo_off[q + 1] > P.halo_off[q] ? 1 : 0;
  if (n_neighbour_ranks) *n_neighbour_ranks = nb;
  return FB_OK;
}

int fb_fem_renumbering(fb_fem_t h, int* span_caller, int* span_internal) {
  if (!h) return 0;
  if (h->span_stale && !h->poisoned && hipSetDevice(h->prm.device) == hipSuccess) {  // (a merged fb_fem_resync_delta left the measurement for now)
    int span = 0;
    double mean = 0.0;
    if (tet_span_device(h->stream, h->plan.n_tets, h->tets.p, h->plan.n_global, nullptr, h->plan_ws, &span, &mean) == FB_OK) {
      h->ren.span_after = span; h->ren.mean_after = mean;
      h->span_stale = false;
    }
  }
  if (span_caller) *span_caller = h->ren.span_before;
  if (span_internal) *span_internal = h->ren.span_after;
  return h->ren.active ? 1 : 0;
}

int fb_fem_owned_nodes(fb_fem_t h, int* ids) {
  if (!h || !ids) return fail(FB_EINVAL, "null argument");
  FB_HIP(hipSetDevice(h->prm.device));
  FB_TRY(ensure_host_order(h));
  const FemPlan& P = h->plan;
  for (int l = 0; l < P.n_owned; l++) ids[l] = h->l2c.empty() ? P.local2global[l] : h->l2c[l];
  return FB_OK;
}

int fb_fem_element_stiffness(fb_fem_t h, int first, int count, double* K0, double* Minv) {
  CHECK_HANDLE(h);
  if (first < 0 || count < 0 || first + count > h->plan.n_tets || !K0) return fail(FB_EINVAL, "element range [%d,%d) outside [0,%d)", first, first + count, h->plan.n_tets);
  const int kChunk = 1 << 16;
  DevBuf<double> dK, dM;
  FB_TRY(dK.alloc((size_t)144 * std::min(count, kChunk)));
  if (Minv) FB_TRY(dM.alloc((size_t)16 * std::min(count, kChunk)));
  for (int done = 0; done < count; done += kChunk) {
    const int n = std::min(kChunk, count - done);
    FB_TRY(launch_element_K0(h, first + done, n, dK.p, Minv ? dM.p : nullptr));
    FB_TRY(dK.download(K0 + (size_t)144 * done, (size_t)144 * n, h->stream));
    if (Minv) FB_TRY(dM.download(Minv + (size_t)16 * done, (size_t)16 * n, h->stream));
  }
  return FB_OK;
}

int fb_fem_time_element_stiffness(fb_fem_t h, int reps, double* seconds_per_pass) {
  CHECK_HANDLE(h);
  if (reps < 1 || !seconds_per_pass) return fail(FB_EINVAL, "bad arguments");
  const int kChunk = 1 << 16, nt = h->plan.n_tets;
  DevBuf<double> dK;
  FB_TRY(dK.alloc((size_t)144 * std::min(nt, kChunk)));  // the 1.15 GB of a 1M-tet K0 set are produced chunk by chunk into the same scratch
  auto pass = [&]() {
    for (int done = 0; done < nt; done += kChunk) FB_TRY(launch_element_K0(h, done, std::min(kChunk, nt - done), dK.p, nullptr));
    return FB_OK;
  };
  FB_TRY(pass());
  FB_TRY(timed_reps(h, reps, pass, seconds_per_pass));
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int fb_fem_assemble(fb_fem_t h, const double* u, double* f, double* K_blocks) {
  CHECK_HANDLE(h);
  if (!u) return fail(FB_EINVAL, "null displacement");
  FB_TRY(upload_global_vec(h, u, h->tmp));
  FB_TRY(h->Ad.zero(h->stream));  // stands in for qvel and fext (both unused in raw mode)
  AsmParams ap;
  asm_materials(h, ap);
  ap.s_k = 1.0; ap.s_m = 0.0; ap.g_k = 0.0; ap.g_m = 0.0; ap.g_a = 0.0; ap.rhs_scale = 0.0; ap.apply_mask = 0;
  FB_TRY(launch_warp(h, h->tmp.p, nullptr));
  FB_TRY(h->f64 ? launch_rows<double>(h, ap, h->Ad.p, h->Ad.p, h->mblk.p, h->r.p, nullptr, nullptr)
                : launch_rows<float>(h, ap, h->Ad.p, h->Ad.p, h->mblk.p, h->r.p, nullptr, nullptr));
  h->system_valid = false;
  if (f) FB_TRY(download_owned(h, h->r, f));
  if (K_blocks) FB_TRY(download_blocks(h, K_blocks));
  return FB_OK;
}

int fb_fem_system(fb_fem_t h, double* Keff_blocks, double* rhs) {
  CHECK_HANDLE(h);
  FB_TRY(assemble_system(h));
  if (motion_active(h)) FB_TRY(motion_correct_rhs(h));  // (the right-hand side the step would solve)
  if (rhs) FB_TRY(download_owned(h, h->rhs, rhs));
  if (Keff_blocks) FB_TRY(download_blocks(h, Keff_blocks));
  return FB_OK;
}

int fb_fem_mass(fb_fem_t h, double* m_blocks) {
  CHECK_HANDLE(h);
  if (!m_blocks) return fail(FB_EINVAL, "null output");
  std::vector<double> u((size_t)3 * h->plan.n_global, 0.0);
  FB_TRY(fb_fem_assemble(h, u.data(), nullptr, nullptr));
  FB_TRY(ensure_host_pattern(h));
  const FemPlan& P = h->plan;
  std::vector<double> host((size_t)P.n_slots * 64);
  FB_TRY(h->mblk.download(host.data(), host.size(), h->stream));
  const bool mapped = h->ren.active;
  std::vector<double> internal;
  if (mapped) {
    FB_TRY(ensure_caller_pattern(h));
    internal.resize((size_t)P.n_blocks);
  }
  double* dst = mapped ? internal.data() : m_blocks;
  for (int a = 0; a < P.n_owned; a++)
    for (int p = P.bptr[a]; p < P.bptr[a + 1]; p++) dst[p] = host[(size_t)P.blk_slot[p] * 64 + (a & 63)];
  if (mapped)
    for (int pc = 0; pc < P.n_blocks; pc++) m_blocks[pc] = internal[(size_t)h->c_src[pc]];
  return FB_OK;
}

int fb_fem_spmv(fb_fem_t h, const double* x, double* y) {
  CHECK_HANDLE(h);
  if (!x || !y) return fail(FB_EINVAL, "null vector");
  if (!h->system_valid) FB_TRY(assemble_system(h));
  FB_TRY(upload_global_vec(h, x, h->tmp));
  FB_TRY(halo_exchange(h, h->tmp.p));
  FB_TRY(spmv(h, 0, h->tmp.p, h->Ad.p, nullptr, nullptr, 0));
  return download_owned(h, h->Ad, y);
}

int fb_fem_pcg(fb_fem_t h, const double* rhs, double* x, double eps, int max_iter, int* iterations_out) {
  CHECK_HANDLE(h);
  if (!rhs || !x) return fail(FB_EINVAL, "null vector");
  if (!(eps > 0) || max_iter < 0) return fail(FB_EINVAL, "bad PCG parameters");
  if (!h->system_valid) FB_TRY(assemble_system(h));
  FB_TRY(upload_global_vec(h, rhs, h->tmp));
  int iters = 0;
  FB_TRY(pcg_solve(h, h->tmp.p, eps, max_iter, &iters, nullptr));
  if (iterations_out) *iterations_out = iters;
  return download_owned(h, h->x, x);
}

int fb_fem_time_spmv(fb_fem_t h, int reps, double* seconds_per_spmv) {
  CHECK_HANDLE(h);
  if (reps < 1 || !seconds_per_spmv) return fail(FB_EINVAL, "bad arguments");
  if (!h->system_valid) FB_TRY(assemble_system(h));
  // the kernel timed is the one the PCG loop launches every iteration: k_spmv<MT,3> (q = A d + the three merged sums),
  // on the state a solve of the current right-hand side starts from (so its convergence test does not exit early)
  const FemPlan& P = h->plan;
  hipLaunchKernelGGL(k_cg_init, dim3(h->grid), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->rhs.p, h->invdiag.p, h->x.p, h->r.p, h->d.p,
                     h->part_b.p);
  hipLaunchKernelGGL(k_cg_begin, dim3(1), dim3(kBlock), 0, h->stream, h->st.p, h->part_b.p, h->grid, (const double*)nullptr, 1e-30, 1 << 30);
  FB_HIP(hipGetLastError());
  FB_TRY(spmv(h, 3, h->d.p, h->Ad.p, h->r.p, h->part_a.p, 0));  // warm
  return timed_reps(h, reps, [&] { return spmv(h, 3, h->d.p, h->Ad.p, h->r.p, h->part_a.p, 0); }, seconds_per_spmv);
}

int fb_fem_time_exchange(fb_fem_t h, int reps, double* seconds_per_halo, double* seconds_per_sum) {
  CHECK_HANDLE(h);
  if (reps < 1) return fail(FB_EINVAL, "bad arguments");
  if (seconds_per_halo) *seconds_per_halo = 0.0;
  if (seconds_per_sum) *seconds_per_sum = 0.0;
  if (!h->comm || h->comm->n_ranks == 1) return FB_OK;
  hipStream_t s = h->stream;
  double* sc = nullptr;
  FB_TRY(halo_exchange(h, h->tmp.p));  // warm, and lines the ranks up
  FB_TRY(global_scalar(h, h->part_a.p, &sc, false, 3));
  float ms = 0;
  // (three events around two loops with no wait between them: timed_reps twice would put a second record and a wait on the stream)
  FB_HIP(hipEventRecord(h->ev[0], s));
  for (int i = 0; i < reps; i++) FB_TRY(halo_exchange(h, h->tmp.p));
  FB_HIP(hipEventRecord(h->ev[1], s));
  for (int i = 0; i < reps; i++) FB_TRY(global_scalar(h, h->part_a.p, &sc, false, 3));
  FB_HIP(hipEventRecord(h->ev[2], s));
  FB_HIP(hipStreamSynchronize(s));
  if (h->p2p) FB_TRY(p2p_check(h->p2p, s));
  FB_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  if (seconds_per_halo) *seconds_per_halo = ms * 1e-3 / reps;
  FB_HIP(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
  if (seconds_per_sum) *seconds_per_sum = ms * 1e-3 / reps;
  return FB_OK;
}

int fb_fem_time_assembly(fb_fem_t h, int reps, double* seconds_per_assembly) {
  CHECK_HANDLE(h);
  if (reps < 1 || !seconds_per_assembly) return fail(FB_EINVAL, "bad arguments");
  FB_TRY(assemble_system(h));
  return timed_reps(h, reps, [&] { return assemble_system(h); }, seconds_per_assembly);
}


int fb_fem_iteration_bytes(fb_fem_t h, double* bytes) {
  if (!h || !bytes) return fail(FB_EINVAL, "null argument");
  const FemPlan& P = h->plan;
  // SURVEY.md 8(d), one Jacobi-PCG iteration: the BSR SpMV (nnzb 3x3 blocks with a 2- or 4-byte column id, the row pointers,
  // the low part of the diagonal blocks) + the fused lower bound of the vector traffic, 9 vector streams (x, r, d read and
  // written, q, 1/diag and d read by the product), here in fp64
  const double idx = h->c16 ? 2.0 : 4.0;
  *bytes = (double)P.n_blocks * (9.0 * mt_size(h) + idx) + (P.n_owned + 1) * 4.0 + 6.0 * mt_size(h) * P.n_owned + 9.0 * 3.0 * P.n_owned * 8.0;
  return FB_OK;
}

int fb_fem_spmv_bytes(fb_fem_t h, double* bytes) {
  if (!h || !bytes) return fail(FB_EINVAL, "null argument");
  const FemPlan& P = h->plan;
  // SURVEY.md 8d BSR figure, for the launch the PCG loop makes (k_spmv<MT,3>): nnzb*(9 values + 4 B index) + (rows+1)*4
  // + the low part of each row's diagonal block (9 values per row) + fp64 vectors: d read once, q written once, and the
  // own-row r and 1/diag the merged sums need
  // (the index is 2 bytes where the row kernel reads 16-bit column differences)
  const double idx = (h->c16 && h->split == 0) ? 2.0 : 4.0;
  // (6 of the 9 planes of the symmetric low part are read)
  *bytes = (double)P.n_blocks * (9.0 * mt_size(h) + idx) + (P.n_owned + 1) * 4.0 + 6.0 * mt_size(h) * P.n_owned + 3.0 * P.n_owned * 8.0 * 4.0;
  return FB_OK;
}

int fb_fem_assembly_bytes(fb_fem_t h, double* bytes) {
  if (!h || !bytes) return fail(FB_EINVAL, "null argument");
  const FemPlan& P = h->plan;
  // pass 1: tet ids 16 + rest record 128 + 4 nodes * (x0 + u) 48 + rotated record 16*MT + element force 96
  // pass 2: contribution words 16*4 per tet + Keff values 9*MT per block + index 4 per block + 5 node vectors
  *bytes = (double)P.n_tets * (16.0 + 128.0 + 192.0 + 16.0 * mt_size(h) + 96.0 + 64.0) + (double)P.n_blocks * (9.0 * mt_size(h) + 4.0) +
           3.0 * P.n_owned * 8.0 * 5.0;
  return FB_OK;
}

}  // extern "C"
