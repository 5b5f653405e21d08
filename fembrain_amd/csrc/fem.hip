// C-ABI of the FEM hot path (include/fembrain_hip.h): handle life cycle, the per-step driver and the
// inspection entry points.  Kernels live in fem_device.hip.h, the host-side plan in fem_plan.cpp.
#include <cfloat>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include <chrono>

#include "fem_device.hip.h"
#include "fem_handle.h"

using namespace fb;

namespace {

size_t mt_size(const fb_fem_s* h) { return h->f64 ? sizeof(double) : sizeof(float); }


// one wavefront per slice: does any of its columns lie in the halo?
__global__ __launch_bounds__(kBlock) void k_slice_halo(int n_slices, int n_owned, const int* __restrict__ slice_off, const int* __restrict__ colidx,
                                                       unsigned char* __restrict__ out) {
  const int s = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= n_slices) return;
  bool any = false;
  for (int k = slice_off[s]; k < slice_off[s + 1]; k++) any = any || colidx[(size_t)k * 64 + lane] >= n_owned;
  const unsigned long long b = __ballot(any);
  if (lane == 0) out[s] = b != 0ULL ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_widen_positions(long long n, const float* __restrict__ in, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

// Zero fills of a (re-)build, batched: about twenty buffers are cleared, and a fill per buffer costs 4-5 us of launch each however
// small it is.  add() notes them (4-byte granularity), flush() clears up to kZeroMax per launch.
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
}  // namespace fb
namespace {

// slack of this handle's allocations (common.h): a quarter for a mesh that will be cut, or what reserve_nodes / reserve_elements ask for
int handle_slack(const fb_fem_s* h, int n_nodes, int n_tets) {
  if (!h->prm.expect_cuts) return 2;
  double f = 0.25;
  if (h->prm.reserve_nodes > n_nodes && n_nodes > 0) f = std::max(f, (double)h->prm.reserve_nodes / n_nodes - 1.0);
  if (h->prm.reserve_elements > n_tets && n_tets > 0) f = std::max(f, (double)h->prm.reserve_elements / n_tets - 1.0);
  return std::max(2, std::min(32, (int)std::ceil(f * 16.0)));
}

constexpr int kFreshOrderPercent = 2;
int fresh_order_percent() {
  const char* e = getenv("FEMBRAIN_FRESH_ORDER_PERCENT");
  return e ? std::max(0, atoi(e)) : kFreshOrderPercent;
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

int upload_plan(fb_fem_s* h, const double* xyz_global, const float* xyz_device = nullptr, const double* xyz_device64 = nullptr) {
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
    const long long n3 = 3LL * P.n_local;
    FB_TRY(h->x0.alloc((size_t)n3));
    hipLaunchKernelGGL(k_widen_positions, dim3((unsigned)((n3 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n3, xyz_device, h->x0.p);
    FB_HIP(hipGetLastError());
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

// ---- per-element materials ----
inline bool has_material_map(const fb_fem_s* h) { return h->mat_ids.p != nullptr; }

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

int launch_rest(fb_fem_s* h, int* first_flat = nullptr) {
  h->mass_valid = false;  // (the rest volumes may change)
  const int nt = h->plan.n_tets;
  hipLaunchKernelGGL(k_tet_rest, dim3(ceil_div(nt, kBlock)), dim3(kBlock), 0, h->stream, nt, h->tets.p, h->x0.p, h->rest.p, first_flat, h->volf.p);
  FB_HIP(hipGetLastError());
  return FB_OK;
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

void drop_graph(fb_fem_s* h) {
  if (h->batch_graph) (void)hipGraphExecDestroy(h->batch_graph);
  h->batch_graph = nullptr;
  h->graph_rhs = nullptr;
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

// The plan of an unsharded handle, built on the device (plan_device.hip).  The host keeps the scalars, the slice offsets,
// the identity numbering and the constraint mask; the pattern arrays stay on the device until an inspection entry point
// asks for them (ensure_host_pattern).
// tets: host node ids, or -- d_tets non-null -- ids already on this device (the polygonizer's own output: in range by construction)
int build_plan_on_device(fb_fem_s* h, int n_nodes, int n_tets, const int* tets, int n_fixed, const int* fixed, const double* xyz, const uint4* d_tets = nullptr,
                         const float* d_xyz = nullptr, const double* d_xyz64 = nullptr) {
  if (n_nodes <= 0 || n_tets <= 0 || (!tets && !d_tets)) return fail(FB_EINVAL, "empty mesh (%d nodes, %d tets)", n_nodes, n_tets);
  if ((long long)n_tets >= (1LL << 28)) return fail(FB_EINVAL, "too many tets for the packed contribution word");

  static const bool timing = getenv("FEMBRAIN_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (timing) fprintf(stderr, "[fembrain] device plan: %s at %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  };
  FemPlan& P = h->plan;
  P = FemPlan();
  P.n_global = n_nodes; P.n_ranks = 1; P.rank = 0;
  P.splits = {0, n_nodes};
  P.node_lo = 0; P.node_hi = n_nodes;
  P.n_owned = P.n_local = n_nodes; P.n_halo = 0;
  P.local2global.resize(n_nodes);
  for (int l = 0; l < n_nodes; l++) P.local2global[l] = l;
  P.halo_off.assign(2, 0);
  P.send_off.assign(2, 0);
  P.n_tets = n_tets;
  if (d_tets) {
    FB_TRY(h->tets.alloc((size_t)n_tets));
    FB_HIP(hipMemcpyAsync(h->tets.p, d_tets, sizeof(int4) * (size_t)n_tets, hipMemcpyDeviceToDevice, h->stream));
  } else {
    FB_TRY(h->tets.upload((const int4*)tets, (size_t)n_tets, h->stream));
  }
  lap("elements uploaded");
  {
    // the internal node order (renumber.h): decided from the widest element, built from the rest positions
    bool want = false;
    FB_TRY(renumber_decide(h->stream, renumber_mode(h), n_nodes, n_tets, h->tets.p, h->plan_ws, h->ren, &want));
    if (want) {
      FB_TRY(h->xyz_in.reserve((size_t)3 * n_nodes));
      if (d_xyz64) {
        FB_HIP(hipMemcpyAsync(h->xyz_in.p, d_xyz64, sizeof(double) * 3 * (size_t)n_nodes, hipMemcpyDeviceToDevice, h->stream));
      } else if (d_xyz) {
        const long long n3 = 3LL * n_nodes;
        hipLaunchKernelGGL(k_widen_positions, dim3((unsigned)((n3 + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, n3, d_xyz, h->xyz_in.p);
        FB_HIP(hipGetLastError());
      } else {
        FB_HIP(hipMemcpyAsync(h->xyz_in.p, xyz, sizeof(double) * 3 * (size_t)n_nodes, hipMemcpyHostToDevice, h->stream));
      }
      FB_TRY(renumber_build(h->stream, renumber_mode(h), n_nodes, n_tets, h->tets.p, h->xyz_in.p, h->plan_ws, h->ren));
      if (h->ren.active) {
        FB_TRY(relabel_tets(h->stream, n_tets, h->tets.p, n_nodes, h->ren.d_new_of_old.p));
        FB_TRY(h->x0.alloc((size_t)3 * n_nodes));
        FB_TRY(gather_nodes(h->stream, n_nodes, 3, h->xyz_in.p, h->ren.d_old_of_new.p, h->x0.p));
        h->x0_ready = true;  // (P.local2global -- internal id -> the caller's -- is fetched when an inspection entry point asks: ensure_host_order)
        h->ren_nodes_at_build = n_nodes;
      }
    }
    if (getenv("FEMBRAIN_TIMING"))
      fprintf(stderr, "[fembrain] node order: widest element %d -> %d (%s%s)\n", h->ren.span_before, h->ren.span_after, h->ren.active ? "renumbered" : "caller's order kept",
              h->ren.active && h->ren.sigma ? ", rows sorted by element count inside windows" : "");
  }
  lap("node order");
  // constraint masks on the device, in the internal order (host: 0.23 ms of loops and two uploads at 1M tets)
  FB_TRY(device_constraint_masks(h->stream, n_nodes, n_fixed, fixed, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->fixed_stage, h->dofmask, h->nodemask));
  P.n_fixed_owned = n_fixed;
  h->masks_ready = true;
  lap("constraints");
  DevicePlan D;
  D.slice_off = &h->slice_off; D.colidx = &h->colidx; D.slot_coff = &h->slot_coff; D.slot_ccnt = &h->slot_ccnt; D.contrib = &h->contrib;
  D.bptr = &h->d_bptr; D.bcol = &h->d_bcol; D.blk_slot = &h->d_blk_slot; D.coldelta = &h->coldelta; D.ucnt_keep = &h->d_ucnt;
  // (the widest element was measured for the node order: FB_RENUMBER_OFF skips that pass and leaves the sort its 64-bit keys)
  const int span = renumber_mode(h) == FB_RENUMBER_OFF ? -1 : (h->ren.active ? h->ren.span_after : h->ren.span_before);
  const int rc = build_plan_device(h->stream, n_nodes, n_tets, h->tets.p, D, h->plan_ws, nullptr, span);
  if (h->plan_ws.bytes() > ((size_t)2 << 30)) h->plan_ws.release();  // kept for the next re-sync only while it is small change (0.8 GB at 1M tets)
  if (rc != FB_OK && D.first_bad_tet >= 0 && tets) {  // say which node, as the host builder does
    for (int k = 0; k < 4; k++) {
      const int id = tets[4 * (size_t)D.first_bad_tet + k];
      if (id < 0 || id >= n_nodes) return fail(FB_EINVAL, "tet %d references node %d outside [0,%d)", D.first_bad_tet, id, n_nodes);
    }
  }
  FB_TRY(rc);
  P.n_blocks = D.n_blocks; P.n_slices = D.n_slices; P.n_slots = D.n_slots; P.n_crows = D.n_crows;
  h->c16 = (D.deltas_fit16 && read_host_knobs().spmv_c16) ? 1 : 0;
  P.slice_off = D.slice_off_host;
  h->csr_ready = true;
  return FB_OK;
}

// global node ids of a rank's elements -> local ids: owned nodes first, then the halo in ascending global order
__global__ void __launch_bounds__(kBlock) k_tets_to_local(int n_tets, int4* __restrict__ tets, int node_lo, int n_owned, const int* __restrict__ halo, int n_halo) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_tets) return;
  int4 t = tets[e];
  int* v = &t.x;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int g = v[i];
    if (g >= node_lo && g < node_lo + n_owned) { v[i] = g - node_lo; continue; }
    int lo = 0, hi = n_halo;  // lower bound; g is in the list by construction
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (halo[mid] < g) lo = mid + 1; else hi = mid;
    }
    v[i] = n_owned + lo;
  }
  tets[e] = t;
}

// One rank's share of a sharded system: partition, local numbering, halo and send lists on the host (build_fem_partition: one
// pass over the element list), then pattern / SELL-64 / contribution lists of the owned rows on the device -- the part that
// took 68-75 ms per rank at 1M tets on the host.
int build_shard_plan_on_device(fb_fem_s* h, int n_nodes, int n_tets, const int* tets, int n_fixed, const int* fixed, int n_ranks, int rank,
                               const int* splits, const double* xyz) {
  FemPlan& P = h->plan;
  static const bool timing = getenv("FEMBRAIN_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (timing) fprintf(stderr, "[fembrain] shard plan: %s at %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  };
  // the partition (elements with an owned node, halo, send lists, local numbering) is computed on the device from the uploaded
  // list, be it the rank's own elements or the whole mesh; on the host only for more than 64 ranks or FEMBRAIN_PARTITION_DEVICE=0
  const bool on_device = n_ranks <= 64 && !(getenv("FEMBRAIN_PARTITION_DEVICE") && atoi(getenv("FEMBRAIN_PARTITION_DEVICE")) == 0);
  DevBuf<int> d_halo;
  if (on_device) {
    FB_TRY(begin_fem_partition(P, n_nodes, n_tets, n_ranks, rank, splits));
    FB_TRY(h->tets.upload((const int4*)tets, (size_t)n_tets, h->stream));
    if (renumber_mode(h) == FB_RENUMBER_ON) {
      // Opt-in on a sharded handle (include/fembrain_hip.h, "Node numbering"): every rank derives the SAME internal order from the whole
      // mesh, relabels its copy of the element list, and the ranks then own contiguous ranges of THAT order -- slabs of the body with
      // two neighbours each, whatever the caller's numbering.  Everything below works on internal ids; l2c maps back at the ABI.
      bool want = false;
      FB_TRY(renumber_decide(h->stream, FB_RENUMBER_ON, n_nodes, n_tets, h->tets.p, h->plan_ws, h->ren, &want));
      if (want) {
        FB_TRY(h->xyz_in.reserve((size_t)3 * n_nodes));
        FB_HIP(hipMemcpyAsync(h->xyz_in.p, xyz, sizeof(double) * 3 * (size_t)n_nodes, hipMemcpyHostToDevice, h->stream));
        FB_TRY(renumber_build(h->stream, FB_RENUMBER_ON, n_nodes, n_tets, h->tets.p, h->xyz_in.p, h->plan_ws, h->ren));
      }
      if (h->ren.active) {
        FB_TRY(relabel_tets(h->stream, n_tets, h->tets.p, n_nodes, h->ren.d_new_of_old.p));
        FB_TRY(h->ren.host_maps(h->stream));
        h->order_sum = 0;
        for (int l = 0; l < n_nodes; l++) h->order_sum += (unsigned long long)(l + 1) * (unsigned long long)(h->ren.old_of_new[l] + 7);
      }
      lap("node order");
    }
    DevicePartition dp;
    const int rc = device_partition(h->stream, n_tets, h->tets, n_nodes, n_ranks, rank, P.splits, dp, h->plan_ws);
    if (rc != FB_OK && dp.first_bad_tet >= 0) {  // say which node, as the host builder does
      for (int k = 0; k < 4; k++) {
        const int id = tets[4 * (size_t)dp.first_bad_tet + k];
        if (id < 0 || id >= n_nodes) return fail(FB_EINVAL, "tet %d references node %d outside [0,%d)", dp.first_bad_tet, id, n_nodes);
      }
    }
    FB_TRY(rc);
    P.n_tets = dp.n_kept;
    P.tet_global = dp.tet_global;
    P.n_owned_corners = dp.owned_corners;
    set_partition_halo(P, dp.halo);
    P.send_off = dp.send_off;
    P.send_local = dp.send_local;
  } else {
    FB_TRY(build_fem_partition(P, n_nodes, n_tets, tets, n_ranks, rank, splits, false));
  }
  lap(on_device ? "partition (device)" : "partition (host)");
  if (h->ren.active) {
    // caller ids of the local nodes, and the constrained DOFs in internal ids (ascending again)
    h->l2c.resize((size_t)P.n_local);
    for (int l = 0; l < P.n_local; l++) h->l2c[l] = h->ren.old_of_new[P.local2global[l]];
    for (int i = 0; i < n_fixed; i++) {
      if (fixed[i] < 0 || fixed[i] >= 3 * n_nodes) return fail(FB_EINVAL, "constrained DOF %d out of range [0,%d)", fixed[i], 3 * n_nodes);
      if (i && fixed[i] <= fixed[i - 1]) return fail(FB_EINVAL, "constrained DOFs must be strictly ascending (index %d)", i);
    }
    std::vector<int> mapped((size_t)n_fixed);
    for (int i = 0; i < n_fixed; i++) mapped[i] = 3 * h->ren.new_of_old[fixed[i] / 3] + fixed[i] % 3;
    std::sort(mapped.begin(), mapped.end());
    FB_TRY(plan_set_constraints(P, n_fixed, mapped.data()));
  } else {
    FB_TRY(plan_set_constraints(P, n_fixed, fixed));
  }
  lap("constraints");
  if (P.n_halo > 0) FB_TRY(d_halo.upload(P.local2global.data() + P.n_owned, (size_t)P.n_halo, h->stream));
  if (on_device) {
    // numbered locally already
  } else if (P.tets.empty()) {  // host partition of the caller's own list: local numbering on the device
    FB_TRY(h->tets.upload((const int4*)tets, (size_t)P.n_tets, h->stream));
    hipLaunchKernelGGL(k_tets_to_local, dim3(ceil_div(P.n_tets, kBlock)), dim3(kBlock), 0, h->stream, P.n_tets, h->tets.p, P.node_lo, P.n_owned, d_halo.p, P.n_halo);
    FB_HIP(hipGetLastError());
  } else {
    FB_TRY(h->tets.upload((const int4*)P.tets.data(), (size_t)P.n_tets, h->stream));
  }
  lap("element upload");
  PlanShard sh;
  sh.n_rows = P.n_owned; sh.node_lo = P.node_lo; sh.n_global = P.n_global; sh.d_halo = d_halo.p; sh.n_halo = P.n_halo;
  sh.n_pairs = 4 * P.n_owned_corners + P.n_owned;
  DevicePlan D;
  D.slice_off = &h->slice_off; D.colidx = &h->colidx; D.slot_coff = &h->slot_coff; D.slot_ccnt = &h->slot_ccnt; D.contrib = &h->contrib;
  D.bptr = &h->d_bptr; D.bcol = &h->d_bcol; D.blk_slot = &h->d_blk_slot; D.coldelta = &h->coldelta; D.halo_base = &h->halo_base;
  const int rc = build_plan_device(h->stream, P.n_local, P.n_tets, h->tets.p, D, h->plan_ws, &sh);
  if (h->plan_ws.bytes() > ((size_t)2 << 30)) h->plan_ws.release();
  FB_TRY(rc);
  P.n_blocks = D.n_blocks; P.n_slices = D.n_slices; P.n_slots = D.n_slots; P.n_crows = D.n_crows;
  h->c16 = (D.deltas_fit16 && read_host_knobs().spmv_c16) ? 2 : 0;  // the halo form
  P.slice_off = D.slice_off_host;
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

// rest state of a device-built plan; the kernel reports the first flat element (see build)
int rest_state_checked(fb_fem_s* h) {
  const int none = 0x7fffffff;
  FB_TRY(h->flat_flag.alloc(1));
  FB_HIP(hipMemcpyAsync(h->flat_flag.p, &none, sizeof(int), hipMemcpyHostToDevice, h->stream));
  FB_TRY(launch_rest(h, h->flat_flag.p));
  int first = none;
  FB_TRY(h->flat_flag.download(&first, 1, h->stream));
  if (first != none)
    return fail(FB_EINVAL, "element %d has zero (or non-finite) rest volume", h->plan.tet_global.empty() ? first : h->plan.tet_global[first]);
  return FB_OK;
}

int build(fb_fem_s* h, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed, const int* fixed, int n_ranks,
          int rank, const int* splits, const DeviceTetMesh* dm = nullptr) {
  drop_graph(h);  // the buffers it refers to are about to be replaced
  h->surf.valid = false;  // a new mesh generation (fb_fem_surface)
  h->stress.valid = false;  // (fb_fem_read_stress / fb_fem_surface_stress)
  SlackScope slack(handle_slack(h, n_nodes, n_tets));
  if (n_ranks == 1 && fixed != h->fixed_caller.data()) h->fixed_caller.assign(fixed, fixed + n_fixed);
  if (h->prm.matrix_precision == FB_MATRIX_AUTO) h->f64 = auto_matrix_f64(h, n_nodes, n_ranks);
  h->last_resync_path = FB_RESYNC_FULL;
  h->csr_ready = false;
  h->span_stale = false;
  h->ren.clear();
  h->l2c.clear();
  h->order_sum = 0;
  h->x0_ready = false;
  h->masks_ready = false;
  h->caller_pattern = false;
  static const bool timing = getenv("FEMBRAIN_TIMING") != nullptr;  // development aid: where a (re)build spends its time
  const auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (timing) fprintf(stderr, "[fembrain] build: %s at %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  };
  const bool want_device = !(getenv("FEMBRAIN_PLAN_DEVICE") && atoi(getenv("FEMBRAIN_PLAN_DEVICE")) == 0);
  h->device_plan = (want_device || dm) && (n_ranks == 1 || !dm);
  h->host_pattern = !h->device_plan;
  if (h->device_plan) {
    const int rc = n_ranks > 1 ? build_shard_plan_on_device(h, n_nodes, n_tets, tets, n_fixed, fixed, n_ranks, rank, splits, xyz)
                               : build_plan_on_device(h, n_nodes, n_tets, tets, n_fixed, fixed, xyz, dm ? dm->tets : nullptr, dm ? dm->xyz : nullptr, dm ? dm->xyz64 : nullptr);
    if (dm && rc != FB_OK) return rc;
    if (rc == FB_ENOMEM) {  // no room for the sort's temporaries: the host builder needs none on the device
      (void)hipGetLastError();
      h->device_plan = false;
      h->host_pattern = true;
      h->ren.clear();  // (the host builder works in the caller's order)
      h->l2c.clear();
      h->order_sum = 0;
      h->x0_ready = false;
      h->masks_ready = false;
    } else if (rc != FB_OK) {
      return rc;
    }
    lap("device plan");
  }
  if (!h->device_plan) {
    h->c16 = 0;
    FB_TRY(build_fem_plan(h->plan, n_nodes, n_tets, tets, n_fixed, fixed, n_ranks, rank, splits));
    lap("host plan");
  }
  // A flat element makes inverse4x4 (corotationalLinearFEM.cpp:529-572) divide by zero; the reference then carries
  // inf/NaN into the step silently.  Refuse it here instead (checked on this rank's elements, rest geometry; a handle
  // whose plan was built on the device lets the rest-state kernel look, below).
  for (int e = 0; e < (h->device_plan ? 0 : h->plan.n_tets); e++) {
    const double* p[4];
    for (int k = 0; k < 4; k++)
      p[k] = xyz + 3 * (size_t)(h->device_plan ? tets[4 * (size_t)e + k] : h->plan.local2global[h->plan.tets[4 * (size_t)e + k]]);
    double a[3], b[3], c[3];
    for (int k = 0; k < 3; k++) { a[k] = p[1][k] - p[0][k]; b[k] = p[2][k] - p[0][k]; c[k] = p[3][k] - p[0][k]; }
    const double det = a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    if (!(det != 0.0) || !std::isfinite(det))
      return fail(FB_EINVAL, "element %d has zero (or non-finite) rest volume", h->plan.tet_global.empty() ? e : h->plan.tet_global[e]);
  }
  lap("volume check");
  if (has_material_map(h) && !h->map_from_delta) {  // a new mesh: every element is material 0 again, the table stays (a delta re-sync swaps its own map in afterwards)
    FB_TRY(h->mat_ids.alloc((size_t)std::max(1, n_tets)));
    FB_TRY(h->mat_ids.zero(h->stream));
    h->mat_hi = 0;
  }
  FB_TRY(upload_plan(h, xyz, dm ? dm->xyz : nullptr, dm ? dm->xyz64 : nullptr));
  lap("upload");
  if (h->device_plan) {
    FB_TRY(rest_state_checked(h));
  } else {
    FB_TRY(launch_rest(h));
    FB_HIP(hipStreamSynchronize(h->stream));
  }
  lap("rest state");
  return FB_OK;
}


// Collective, BEFORE the rank-local build: FB_RENUMBER_AUTO on a sharded handle ("the same contiguous-range rule after an
// RCM / space-filling-curve renumbering").  Equal ranges of the caller's ids are slabs of the body only while the caller numbers plane
// by plane; after cuts (nodes appended at the end: VolMesh.cpp:1086-1091) or on a TetGen mesh every rank is a neighbour of every other
// and half the mesh is halo (profiles/r04_numbering_probe_after.json: 7 neighbours and 128k halo nodes per rank at 8 ranks, against 2 and
// 6k).  Every rank counts the ranks its own elements couple it to under the caller's numbering and sums a checksum of the element list
// it was handed; the ranks all-gather (neighbours, sizes, checksum, mode) and switch the internal order on -- all of them or none --
// when some rank would have more than two neighbours (or, from 8,192 nodes, most of its elements reaching into another rank) AND every
// rank holds the same whole mesh (the internal order is derived from all
// nodes and all elements; a rank that was handed its own elements only keeps the caller's numbering, as before).  One pass over the
// element list on the host (2 ms per million tets) and one all-gather of 40 bytes.
struct ShardOrderVote { int neighbours, n_nodes, n_tets, mode; unsigned long long sum; int splits_sum, own_elements, boundary_elements, pad; };
int vote_shard_order(fb_fem_s* h, int n_nodes, int n_tets, const int* tets, int n_ranks, int rank, const int* splits) {
  h->shard_auto_on = false;
  h->shard_vote_neighbours = 0;
  if (!h->comm || n_ranks < 2) return FB_OK;
  ShardOrderVote mine;
  memset(&mine, 0, sizeof mine);
  int mode = h->prm.renumber > 0 ? FB_RENUMBER_ON : (h->prm.renumber < 0 ? FB_RENUMBER_OFF : FB_RENUMBER_AUTO);
  if (const char* e = getenv("FEMBRAIN_RENUMBER")) mode = atoi(e) != 0 ? FB_RENUMBER_ON : FB_RENUMBER_OFF;
  mine.mode = mode; mine.n_nodes = n_nodes; mine.n_tets = n_tets; mine.neighbours = -1;
  if (mode == FB_RENUMBER_AUTO && tets && n_tets > 0 && n_nodes > 0 && n_ranks <= 64) {
    // (bad ranges, bad ids: the build refuses them with its own message; this rank then votes "unknown")
    shard_neighbour_count(n_nodes, n_tets, tets, n_ranks, rank, splits, &mine.neighbours, &mine.sum, &mine.splits_sum, &mine.own_elements, &mine.boundary_elements);
  }
  std::vector<ShardOrderVote> all((size_t)n_ranks);
  FB_TRY(comm_allgather_bytes(h->comm, &mine, all.data(), sizeof mine, h->stream));
  bool same = true, any_wide = false;
  int most = 0;
  for (int q = 0; q < n_ranks; q++) {
    same = same && all[q].mode == FB_RENUMBER_AUTO && all[q].neighbours >= 0 && all[q].n_nodes == all[0].n_nodes && all[q].n_tets == all[0].n_tets &&
           all[q].sum == all[0].sum && all[q].splits_sum == all[0].splits_sum;
    // more than two neighbour ranks; or (meshes of a size AUTO renumbers at all) most of a rank's elements reach into another rank -- the
    // two-rank form of the same disorder, where "every rank a neighbour" still means one
    any_wide = any_wide || all[q].neighbours > 2 || (n_nodes >= kRenumberMinNodes && 2LL * all[q].boundary_elements > all[q].own_elements);
    most = std::max(most, all[q].neighbours);
  }
  h->shard_vote_neighbours = most;
  h->shard_auto_on = same && any_wide;
  if (getenv("FEMBRAIN_TIMING"))
    fprintf(stderr, "[fembrain] rank %d: node-order vote: %d neighbour ranks here, %d at most, same mesh on every rank: %s -> %s\n", rank, mine.neighbours, most, same ? "yes" : "no",
            h->shard_auto_on ? "internal slab order" : "caller's numbering");
  return FB_OK;
}

// collective: a renumbered sharded handle works only if every rank derived the same internal order (from the same whole mesh)
int agree_on_node_order(fb_fem_s* h) {
  if (!h->comm || h->comm->n_ranks < 2) return FB_OK;
  const int R = h->comm->n_ranks;
  std::vector<unsigned long long> sums((size_t)R);
  FB_TRY(comm_allgather_bytes(h->comm, &h->order_sum, sums.data(), sizeof(unsigned long long), h->stream));
  for (int q = 0; q < R; q++)
    if (sums[q] != sums[0])
      return fail(FB_EINVAL, "the ranks derived different node orders (FB_RENUMBER_ON on a sharded handle needs the WHOLE mesh -- all nodes, all elements -- on every rank, and the same setting)");
  return FB_OK;
}

// collective: every rank of the communicator creates its handle at the same point of its program
int attach_p2p(fb_fem_s* h) {
  const FemPlan& P = h->plan;
  FB_TRY(p2p_attach(h->comm, P.n_local - P.n_owned, P.halo_off.data(), h->stream, &h->p2p));
  if (!h->p2p) return FB_OK;
  h->xch_mode = FB_XCH_P2P_FUSED;
  if (const char* e = getenv("FEMBRAIN_XCH_MODE")) {  // 2 / 3 / 4: how much of the exchange rides inside the PCG kernels
    const int m = atoi(e);
    if (m >= FB_XCH_COLLECTIVE && m <= FB_XCH_P2P_FUSED) h->xch_mode = m;
  }
  FB_TRY(h->send_off_dev.upload(P.send_off, h->stream));
  FB_TRY(h->halo_off_dev.upload(P.halo_off, h->stream));
  // slices with a halo column are done after the halo wait
  if (h->device_plan) {
    FB_TRY(h->slice_halo.alloc((size_t)std::max(1, P.n_slices)));
    hipLaunchKernelGGL(k_slice_halo, dim3(ceil_div(std::max(1, P.n_slices), kWavesPerBlock)), dim3(kBlock), 0, h->stream, P.n_slices, P.n_owned, h->slice_off.p,
                       h->colidx.p, h->slice_halo.p);
    FB_HIP(hipGetLastError());
  } else {
    std::vector<unsigned char> sh((size_t)std::max(1, P.n_slices), 0);
    for (int sl = 0; sl < P.n_slices; sl++)
      for (size_t k = (size_t)P.slice_off[sl] * kSliceRows; k < (size_t)P.slice_off[sl + 1] * kSliceRows && !sh[sl]; k++) sh[sl] = P.colidx[k] >= P.n_owned;
    FB_TRY(h->slice_halo.upload(sh, h->stream));
  }
  if (P.send_local.empty()) FB_TRY(h->send_local.alloc(1));
  return FB_OK;
}

int prewarm_delta(fb_fem_s* h, int n_fixed, const int* fixed);

int create_common(fb_fem_t* out, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed, const int* fixed,
                  const fb_fem_params* params, int n_ranks, int rank, const int* splits, fb_comm_t comm, const DeviceTetMesh* dm = nullptr) {
  if (!out || (!dm && (!xyz || !tets)) || !params) return fail(FB_EINVAL, "null argument");
  if (dm && dm->device != params->device) return fail(FB_EINVAL, "the polygonizer lives on device %d, the FEM handle is asked for device %d", dm->device, params->device);
  if (n_fixed < 0 || (n_fixed > 0 && !fixed)) return fail(FB_EINVAL, "bad constrained DOF list");
  if (params->integrator != FB_INTEGRATOR_VOLUME_CONSERVING && params->integrator != FB_INTEGRATOR_NEWMARK) return fail(FB_EINVAL, "unknown integrator %d", params->integrator);
  if (!(params->timestep > 0) || !(params->E > 0) || !(params->rho > 0) || !(params->nu > -1.0 && params->nu < 0.5) ||
      !std::isfinite(params->timestep) || !std::isfinite(params->E) || !std::isfinite(params->rho) ||
      !std::isfinite(params->damping_mass) || !std::isfinite(params->damping_stiffness))
    return fail(FB_EINVAL, "bad material / timestep / damping parameters");
  if (params->pcg_variant != FB_PCG_MERGED && params->pcg_variant != FB_PCG_REFERENCE && params->pcg_variant != FB_PCG_PERSISTENT &&
      params->pcg_variant != FB_PCG_BLOCK_JACOBI)
    return fail(FB_EINVAL, "unknown pcg_variant %d", params->pcg_variant);
  if (n_ranks > 1 && !comm) return fail(FB_EINVAL, "sharded handle needs a communicator");
  if (comm && (comm->n_ranks != n_ranks || comm->rank != rank)) return fail(FB_EINVAL, "communicator rank/size does not match the handle");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FB_EDEVICE, "no HIP device visible");
  if (params->device < 0 || params->device >= ndev) return fail(FB_EINVAL, "device %d out of range (%d visible)", params->device, ndev);
  FB_HIP(hipSetDevice(params->device));
  fb_fem_s* h = new fb_fem_s;
  h->prm = *params;
  h->comm = comm;  // a one-rank communicator with a live RCCL handle still runs the collectives (plumbing test)
  if (params->matrix_precision != FB_MATRIX_F32 && params->matrix_precision != FB_MATRIX_F64 && params->matrix_precision != FB_MATRIX_AUTO) {
    delete h;
    return fail(FB_EINVAL, "unknown matrix_precision %d", params->matrix_precision);
  }
  h->f64 = params->matrix_precision == FB_MATRIX_F64;  // (FB_MATRIX_AUTO: build() decides by size, at every re-sync again)
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, params->device) == hipSuccess) h->n_cu_device = prop.multiProcessorCount;
  }
  h->lambda = (params->nu * params->E) / ((1 + params->nu) * (1 - 2 * params->nu));
  h->mu = params->E / (2 * (1 + params->nu));
  h->mat_E.assign(1, params->E); h->mat_nu.assign(1, params->nu); h->mat_rho.assign(1, params->rho);  // the one-entry table of the params
  int rc = FB_OK;
  do {
   // collective, before anything rank-local can fail: the node order of a sharded handle under FB_RENUMBER_AUTO
   if (comm && comm->n_ranks > 1 && (rc = vote_shard_order(h, n_nodes, n_tets, tets, n_ranks, rank, splits)) != FB_OK) break;
   // rank-local set-up; a failure here (stream, events, pinned memory, the build) must still reach the agreement below -- the other ranks
   // are on their way into that all-gather
   do {
    // FEMBRAIN_CU_MASK=first:count -- the handle's stream runs on `count` CUs from bit `first` of the CU mask only (development and test
    // aid: two processes on one GPU, each with a persistent kernel on its own half of the CUs); the persistent grid follows
    if (const char* cm = getenv("FEMBRAIN_CU_MASK")) {
      int first = 0, count = 0;
      if (sscanf(cm, "%d:%d", &first, &count) != 2 || first < 0 || count < 8 || first + count > 512) { rc = fail(FB_EINVAL, "FEMBRAIN_CU_MASK=first:count"); break; }
      uint32_t mask[16];
      memset(mask, 0, sizeof mask);
      for (int b = first; b < first + count; b++) mask[b >> 5] |= 1u << (b & 31);
      if (hipExtStreamCreateWithCUMask(&h->stream, 16, mask) != hipSuccess) { rc = fail(FB_EDEVICE, "hipExtStreamCreateWithCUMask failed"); break; }
      h->cu_limit = count;
    } else
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(FB_EDEVICE, "hipStreamCreate failed"); break; }
    for (auto& e : h->ev) if (hipEventCreate(&e) != hipSuccess) rc = fail(FB_EDEVICE, "hipEventCreate failed");
    for (auto& e : h->ev_batch) if (hipEventCreate(&e) != hipSuccess) rc = fail(FB_EDEVICE, "hipEventCreate failed");
    for (auto& e : h->ev_p) if (hipEventCreate(&e) != hipSuccess) rc = fail(FB_EDEVICE, "hipEventCreate failed");
    if (rc != FB_OK) break;
    if (hipHostMalloc((void**)&h->st_host, 2 * sizeof(CGState), hipHostMallocDefault) != hipSuccess) { rc = fail(FB_ENOMEM, "hipHostMalloc failed"); break; }
    if (const char* e = getenv("FEMBRAIN_GRAPH")) h->use_graph = atoi(e) != 0;
    rc = build(h, n_nodes, xyz, n_tets, tets, n_fixed, fixed, n_ranks, rank, splits, dm);
    // a mesh that will be cut: the workspace of fb_fem_resync_delta now, not inside the first cut
    if (rc == FB_OK && h->prm.expect_cuts && n_ranks == 1 && h->device_plan) rc = prewarm_delta(h, n_fixed, fixed);
   } while (0);
    if (comm && comm->n_ranks > 1) {  // creation is collective: the ranks agree on the outcome so far before the collective attach
      const std::string why = rc == FB_OK ? std::string() : last_error();
      std::vector<int> rcs((size_t)n_ranks, 0);
      const int mine = rc;
      const int rc_x = comm_allgather_bytes(comm, &mine, rcs.data(), sizeof(int), h->stream);  // (host-staged or on the null stream if ours could not be made)
      if (rc_x != FB_OK) { rc = rc_x; break; }
      for (int q = 0; q < n_ranks && rc == FB_OK; q++)
        if (rcs[q] != FB_OK) rc = fail(rcs[q], "handle creation failed on rank %d (code %d)", q, rcs[q]);
      if (mine != FB_OK) { last_error() = why; rc = mine; }
      if (rc == FB_OK) rc = agree_on_node_order(h);
    }
    if (rc == FB_OK && comm && comm->n_ranks > 1) rc = attach_p2p(h);
    if (rc == FB_OK && comm && comm->n_ranks > 1) rc = attach_pipe_shard(h);
  } while (0);
  if (rc != FB_OK) {
    std::string keep = last_error();
    fb_fem_destroy(h);
    last_error() = keep;
    return rc;
  }
  *out = h;
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

int fb_fem_create(fb_fem_t* out, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs,
                  const int* fixed_dofs, const fb_fem_params* params) {
  return create_common(out, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, params, 1, 0, nullptr, nullptr);
}

int fb_fem_create_from_poly(fb_fem_t* out, fb_poly_t poly, int n_fixed_dofs, const int* fixed_dofs, const fb_fem_params* params) {
  DeviceTetMesh dm;
  FB_TRY(poly_device_tetmesh(poly, &dm));
  if (dm.n_tets < 1) return fail(FB_EINVAL, "the polygonizer holds no tets");
  return create_common(out, dm.n_vertices, nullptr, dm.n_tets, nullptr, n_fixed_dofs, fixed_dofs, params, 1, 0, nullptr, nullptr, &dm);
}

int fb_fem_create_sharded(fb_fem_t* out, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs,
                          const int* fixed_dofs, const fb_fem_params* params, int n_ranks, int rank, const int* node_splits,
                          fb_comm_t comm) {
  return create_common(out, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, params, n_ranks, rank, node_splits, comm);
}

int fb_fem_destroy(fb_fem_t h) {
  if (!h) return FB_OK;
  (void)hipSetDevice(h->prm.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (auto& e : h->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : h->ev_batch) if (e) (void)hipEventDestroy(e);
  for (auto& e : h->ev_p) if (e) (void)hipEventDestroy(e);
  if (h->st_host) (void)hipHostFree(h->st_host);
  if (h->p2p) p2p_detach(h->p2p);
  release_shard_persist(h);
  drop_graph(h);
  DevBuf<double>* vecs[] = {&h->q, &h->qvel, &h->fext, &h->fint, &h->rhs, &h->x, &h->r, &h->d, &h->Ad, &h->invdiag, &h->tmp};
  for (auto* v : vecs) v->release();
  hipStream_t s = h->stream;
  if (h->side) { (void)hipStreamSynchronize(h->side); (void)hipStreamDestroy(h->side); }
  for (auto& e : h->ev_side) if (e) (void)hipEventDestroy(e);
  delete h;  // frees the remaining device buffers
  if (s) (void)hipStreamDestroy(s);
  return FB_OK;
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


// collective re-sync of a sharded handle; node_splits NULL keeps the handle's ranges when the node count is unchanged, else equal ranges
static int resync_sharded(fb_fem_t h, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs, const int* fixed_dofs,
                          const int* node_splits) {
  // every rank re-syncs at the same point of its program; the peer-to-peer inboxes are sized by the halo and are attached again
  h->poisoned = true;
  h->system_valid = false;
  const int n_ranks = h->plan.n_ranks, rank = h->plan.rank;
  const std::vector<int> kept = h->plan.splits;
  if (!node_splits && n_nodes == h->plan.n_global) node_splits = kept.data();
  // build() is rank-local (a bad node id or a flat element after a cut, no memory ...); what follows is collective.  The ranks
  // agree on the outcome first: if any of them failed, none enters the collective attach -- all stay poisoned and return an
  // error, instead of the healthy ones waiting in an all-gather for a rank that has left.
  FB_TRY(vote_shard_order(h, n_nodes, n_tets, tets, n_ranks, rank, node_splits));  // (collective; before the rank-local build)
  const int rc_mine = build(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, n_ranks, rank, node_splits);
  const std::string why_mine = rc_mine == FB_OK ? std::string() : last_error();
  if (h->comm && h->comm->n_ranks > 1) {
    std::vector<int> rcs((size_t)n_ranks, 0);
    const int rc_x = comm_allgather_bytes(h->comm, &rc_mine, rcs.data(), sizeof(int), h->stream);
    if (rc_x != FB_OK) return rc_x;
    for (int q = 0; q < n_ranks; q++)
      if (rcs[q] != FB_OK && rc_mine == FB_OK)
        return fail(rcs[q], "re-sync failed on rank %d (code %d); this rank's handle is unusable until a re-sync succeeds on every rank", q, rcs[q]);
  }
  if (rc_mine != FB_OK) { last_error() = why_mine; return rc_mine; }
  FB_TRY(agree_on_node_order(h));
  const int mode = h->xch_mode;
  if (h->p2p) { p2p_detach(h->p2p); h->p2p = nullptr; }
  if (h->comm && h->comm->n_ranks > 1) FB_TRY(attach_p2p(h));
  if (h->comm && h->comm->n_ranks > 1) FB_TRY(attach_pipe_shard(h));
  if (h->p2p && mode >= FB_XCH_P2P) h->xch_mode = mode;   // the form chosen before the re-sync stays
  else if (mode == FB_XCH_COLLECTIVE) h->xch_mode = FB_XCH_COLLECTIVE;
  h->poisoned = false;
  return FB_OK;
}

int fb_fem_resync_sharded(fb_fem_t h, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs, const int* fixed_dofs,
                          const int* node_splits) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  FB_HIP(hipSetDevice(h->prm.device));
  if (!xyz || !tets) return fail(FB_EINVAL, "null mesh");
  FB_HIP(hipStreamSynchronize(h->stream));
  if (h->plan.n_ranks == 1) {
    if (node_splits && (node_splits[0] != 0 || node_splits[1] != n_nodes)) return fail(FB_EINVAL, "node splits must cover [0,%d)", n_nodes);
    return fb_fem_resync(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs);
  }
  return resync_sharded(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, node_splits);
}

int fb_fem_resync(fb_fem_t h, int n_nodes, const double* xyz, int n_tets, const int* tets, int n_fixed_dofs, const int* fixed_dofs) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  FB_HIP(hipSetDevice(h->prm.device));
  if (!xyz || !tets) return fail(FB_EINVAL, "null mesh");
  FB_HIP(hipStreamSynchronize(h->stream));
  if (h->plan.n_ranks > 1) return resync_sharded(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, nullptr);
  // build() replaces the plan and the buffers in place; if it fails half way (a node id out of range after a bad
  // subdivision, a flat element, no memory) the handle holds pieces of two meshes and must not step
  h->poisoned = true;
  h->system_valid = false;
  FB_TRY(build(h, n_nodes, xyz, n_tets, tets, n_fixed_dofs, fixed_dofs, 1, 0, nullptr));
  h->poisoned = false;
  return FB_OK;
}

// ---- fb_fem_resync_delta (delta.h) ----
namespace {
// The full builder from the device copy of the new mesh in the caller's numbering (no sorted list to update, or the new mesh is to
// get a new node order): what fb_fem_resync does, without the host hop.
int resync_delta_rebuild(fb_fem_s* h, int n_old, int n_new, int n_fixed, const int* fixed) {
  hipStream_t s = h->stream;
  MeshDelta& D = h->delta;
  const int nt_old = D.n_tets_old, nt_new = D.n_tets_new();
  // the old element list and the rest positions in the caller's numbering
  FB_TRY(h->tets_caller.alloc((size_t)nt_old));
  FB_HIP(hipMemcpyAsync(h->tets_caller.p, h->tets.p, sizeof(int4) * (size_t)nt_old, hipMemcpyDeviceToDevice, s));
  if (h->ren.active) FB_TRY(relabel_tets(s, nt_old, h->tets_caller.p, n_old, h->ren.d_old_of_new.p));
  FB_TRY(h->tets_next.alloc((size_t)nt_new));
  FB_TRY(delta_tets(s, D, h->tets_caller.p, nullptr, h->tets_next.p));
  FB_TRY(h->x0_next.alloc((size_t)3 * n_new));
  if (h->ren.active) FB_TRY(scatter_nodes(s, n_old, 3, h->x0.p, h->ren.d_old_of_new.p, h->x0_next.p));
  else FB_HIP(hipMemcpyAsync(h->x0_next.p, h->x0.p, sizeof(double) * 3 * (size_t)n_old, hipMemcpyDeviceToDevice, s));
  if (D.n_new_nodes) FB_HIP(hipMemcpyAsync(h->x0_next.p + 3 * (size_t)n_old, D.new_xyz.p, sizeof(double) * 3 * (size_t)D.n_new_nodes, hipMemcpyDeviceToDevice, s));
  DeviceTetMesh dm;
  dm.device = h->prm.device; dm.n_vertices = n_new; dm.n_tets = nt_new; dm.xyz = nullptr;
  dm.tets = reinterpret_cast<const uint4*>(h->tets_next.p); dm.xyz64 = h->x0_next.p;
  FB_TRY(build(h, n_new, nullptr, nt_new, nullptr, n_fixed, fixed, 1, 0, nullptr, &dm));
  h->last_resync_path = FB_RESYNC_DELTA_REBUILT;
  return FB_OK;
}

// device_src: removed / added / new_xyz are device arrays (fb_fem_cut; no element changed in place)
int resync_delta(fb_fem_s* h, int n_removed, const int* removed, int n_changed, const int* changed_ids, const int* changed_nodes, int n_added, const int* added,
                 int n_new_nodes, const double* new_xyz, int n_fixed, const int* fixed, bool device_src = false) {
  static const bool timing = getenv("FEMBRAIN_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (timing) fprintf(stderr, "[fembrain] delta re-sync: %s at %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  };
  hipStream_t s = h->stream;
  MeshDelta& D = h->delta;
  PlanWorkspace& W = h->plan_ws;
  const int n_old = h->plan.n_global, nt_old = h->plan.n_tets, n_new = n_old + n_new_nodes;
  SlackScope slack(handle_slack(h, n_new, nt_old - n_removed + n_added));
  drop_graph(h);
  h->surf.valid = false;  // a new mesh generation (fb_fem_surface)
  h->stress.valid = false;  // (fb_fem_read_stress / fb_fem_surface_stress)
  if (fixed != h->fixed_caller.data()) h->fixed_caller.assign(fixed, fixed + n_fixed);
  if (device_src)
    FB_TRY(delta_upload_device(s, nt_old, n_removed, removed, n_added, reinterpret_cast<const int4*>(added), n_new_nodes, new_xyz, D, W));
  else
    FB_TRY(delta_upload(s, nt_old, n_removed, removed, n_changed, changed_ids, changed_nodes, n_added, added, n_new_nodes, new_xyz, D, W));
  const int nt_new = D.n_tets_new();
  if (has_material_map(h)) {
    // the element map through the change, on the device: kept and changed elements keep their material in order, the pieces of a cut
    // inherit their parent's (k_cut_pieces' cut_tets / piece_off), other added elements get 0.  Swapped in when the re-sync is complete.
    FB_TRY(h->mat_ids_next.alloc((size_t)std::max(1, nt_new)));
    if (device_src) FB_TRY(delta_element_bytes(s, D, h->mat_ids.p, h->mat_ids_next.p, h->cut.n_cut, h->cut.cut_tets.p, h->cut.piece_off.p, h->cut.pcount.p));
    else FB_TRY(delta_element_bytes(s, D, h->mat_ids.p, h->mat_ids_next.p));
  }
  lap("change uploaded");
  const char* env = getenv("FEMBRAIN_RESYNC_DELTA");
  bool merge = h->csr_ready && !(env && !strcmp(env, "rebuild"));
  // A renumbered handle keeps the order it has while nodes are added -- new nodes are merged in, old ones stay where they are although
  // the cut has changed how many elements sit on them, so rows of unlike length come to share a slice and the matrix pads.  Measured at
  // 1.1M tets (tools/probe_resync_delta.py): 9 % more nodes merged in, 42.5 us per PCG iteration against 30.6 in a fresh order -- 26 ms per
  // step -- where the full builder from the device copy of the mesh costs 2.9 ms once.  So once kFreshOrderPercent more nodes have come
  // than the order was built for, the change gets a fresh order (FEMBRAIN_FRESH_ORDER_PERCENT overrides: the tests keep the merged
  // path busy with larger changes)
  if (merge && h->ren.active && (long long)n_new * 100 > (long long)h->ren_nodes_at_build * (100 + fresh_order_percent())) merge = false;
  // FB_MATRIX_AUTO is decided again at every re-sync: a mesh that has grown across the size rule gets its values in the other width,
  // which the full builder allocates
  if (merge && h->prm.matrix_precision == FB_MATRIX_AUTO && auto_matrix_f64(h, n_new, 1) != h->f64) merge = false;
  const int mode = renumber_mode(h);
  int span = -1;
  double mean = 0.0;
  if (merge && !h->ren.active && mode != FB_RENUMBER_OFF) {
    // A handle in the caller's order: would the full builder try a new node order for the new mesh (renumber_decide)?  Then it is to
    // decide.  The widest element of the new list: the kept elements are no wider than before, so the new ones settle it unless
    // the old widest element was removed -- measured over the whole new list, as the builder would.
    FB_TRY(h->tets_next.alloc((size_t)nt_new));
    FB_TRY(delta_tets(s, D, h->tets.p, nullptr, h->tets_next.p));
    FB_TRY(tet_span_device(s, nt_new, h->tets_next.p, n_new, nullptr, W, &span, &mean));
    if (mode == FB_RENUMBER_ON || (n_new >= kRenumberMinNodes && span > renumber_span_limit(n_new))) merge = false;
  }
  if (!merge) {
    h->map_from_delta = true;  // (the full builder leaves the map alone: the old one is still being read by the kernels queued above)
    const int rc = resync_delta_rebuild(h, n_old, n_new, n_fixed, fixed);
    h->map_from_delta = false;
    // (also where the builder failed half way: the handle is poisoned then and launches nothing until a re-sync succeeds, but the map's
    // length follows the element count the plan may already have)
    if (has_material_map(h)) h->mat_ids.swap(h->mat_ids_next);
    return rc;
  }

  // ---- the node order ----
  if (h->ren.active) {
    if (n_new_nodes) {
      FB_TRY(delta_node_order(s, D, n_old, h->ren.geom, h->ren.d_keys.p, h->ren.d_old_of_new.p, h->map_next_a, h->map_next_b, W, h->ren.sigma ? h->ren.n_windows : 0,
                              h->ren.sigma ? h->ren.d_win_keys.p : nullptr));
      h->ren.d_old_of_new.swap(h->map_next_a);
      h->ren.d_new_of_old.swap(h->map_next_b);
      h->ren.d_keys.swap(D.node_keys);
      h->ren.n = n_new;
      h->ren.old_of_new.clear();
      h->ren.new_of_old.clear();
    }
    FB_TRY(delta_relabel_nodes(s, D, n_new, h->ren.d_new_of_old.p));
    FB_TRY(h->tets_next.alloc((size_t)nt_new));
    FB_TRY(delta_tets(s, D, h->tets.p, D.mapped ? D.imap.p : nullptr, h->tets_next.p));
    h->span_stale = true;  // (the widest element under the merged order is measured when fb_fem_renumbering asks: a pass and a wait saved here)
  } else {
    h->ren.clear();
    if (mode != FB_RENUMBER_OFF) { h->ren.span_before = h->ren.span_after = span; h->ren.mean_before = h->ren.mean_after = mean; }
    else {
      FB_TRY(h->tets_next.alloc((size_t)nt_new));
      FB_TRY(delta_tets(s, D, h->tets.p, nullptr, h->tets_next.p));
    }
  }
  h->tets.swap(h->tets_next);
  FB_TRY(h->x0_next.alloc((size_t)3 * n_new));
  FB_TRY(delta_positions(s, D, n_old, h->x0.p, h->x0_next.p));
  h->x0.swap(h->x0_next);
  h->l2c.clear();
  h->order_sum = 0;
  h->x0_ready = true;
  h->caller_pattern = false;
  h->last_resync_path = FB_RESYNC_DELTA_MERGED;
  lap("node order and elements");
  FB_TRY(device_constraint_masks(s, n_new, n_fixed, fixed, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->fixed_stage, h->dofmask, h->nodemask));
  h->masks_ready = true;
  // ---- the plan, from the plan (delta.hip) ----
  OldPlanArrays old_plan = {h->d_bptr.p, h->d_bcol.p, h->d_ucnt.p, h->slice_off.p, h->slot_coff.p, h->contrib.p, n_old, h->plan.n_blocks};
  FemPlan& P = h->plan;
  P = FemPlan();
  P.n_global = n_new; P.n_ranks = 1; P.rank = 0;
  P.splits = {0, n_new};
  P.node_lo = 0; P.node_hi = n_new;
  P.n_owned = P.n_local = n_new; P.n_halo = 0;
  P.local2global.resize(n_new);
  for (int l = 0; l < n_new; l++) P.local2global[l] = l;
  P.halo_off.assign(2, 0);
  P.send_off.assign(2, 0);
  P.n_tets = nt_new;
  P.n_fixed_owned = n_fixed;
  DevicePlan Dp;
  // (built next to the arrays it is built from; colidx, the list heights and the 16-bit column words are read by no stage of it)
  Dp.slice_off = &D.slice_off2; Dp.colidx = &h->colidx; Dp.slot_coff = &D.slot_coff2; Dp.slot_ccnt = &h->slot_ccnt; Dp.contrib = &D.contrib2;
  Dp.bptr = &D.bptr2; Dp.bcol = &D.bcol2; Dp.blk_slot = &D.blk_slot2; Dp.coldelta = &h->coldelta; Dp.ucnt_keep = &D.ucnt2;
  h->csr_ready = false;
  FB_TRY(delta_plan(s, D, old_plan, h->tets_next.p, h->tets.p, n_new, Dp, W));  // (tets_next: the old list, swapped out above)
  h->slice_off.swap(D.slice_off2); h->slot_coff.swap(D.slot_coff2); h->contrib.swap(D.contrib2);
  h->d_bptr.swap(D.bptr2); h->d_bcol.swap(D.bcol2); h->d_blk_slot.swap(D.blk_slot2); h->d_ucnt.swap(D.ucnt2);
  h->csr_ready = true;
  P.n_blocks = Dp.n_blocks; P.n_slices = Dp.n_slices; P.n_slots = Dp.n_slots; P.n_crows = Dp.n_crows;
  h->c16 = (Dp.deltas_fit16 && read_host_knobs().spmv_c16) ? 1 : 0;
  P.slice_off = Dp.slice_off_host;
  h->device_plan = true;
  h->host_pattern = false;
  lap("plan");
  if (has_material_map(h)) h->mat_ids.swap(h->mat_ids_next);
  FB_TRY(upload_plan(h, nullptr));
  lap("per-step arrays");
  FB_TRY(rest_state_checked(h));
  lap("rest state");
  return FB_OK;
}

// fb_fem_params.expect_cuts: everything a fb_fem_resync_delta allocates -- the second set of plan arrays it builds into, the element and
// node maps, the sort's temporaries for a change of a twentieth of the elements -- is allocated at creation by running the empty change
int prewarm_delta(fb_fem_s* h, int n_fixed, const int* fixed) {
  MeshDelta& D = h->delta;
  FB_TRY(delta_reserve(h->stream, D, h->plan_ws, (long long)16 * (h->plan.n_tets / 20 + 64)));
  if (h->ren.active) {
    // ... and the node order's second stage on this mesh, into a scratch order: a cut mesh needs it (renumber.h) where the uncut one did
    // not, and the first launch of its kernels in a process costs milliseconds (7 of the 9.7 ms of a first cut, tools/probe_resync_delta.py)
    Renumbering scratch;
    FB_TRY(renumber_build(h->stream, FB_RENUMBER_ON, h->plan.n_global, h->plan.n_tets, h->tets.p, h->x0.p, h->plan_ws, scratch, true));
  }
  FB_TRY(resync_delta(h, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, n_fixed, fixed));
  h->last_resync_path = FB_RESYNC_FULL;
  return FB_OK;
}

}  // namespace

int fb_fem_resync_delta(fb_fem_t h, int n_removed, const int* removed, int n_changed, const int* changed_ids, const int* changed_nodes, int n_added,
                        const int* added_tets, int n_new_nodes, const double* new_xyz, int n_fixed_dofs, const int* fixed_dofs) {
  if (!h) return fail(FB_EINVAL, "null FEM handle");
  FB_HIP(hipSetDevice(h->prm.device));
  if (h->poisoned) return fail(FB_EINVAL, "the handle is unusable after a failed re-sync: a full fb_fem_resync first");
  if (h->plan.n_ranks > 1 || !h->device_plan) return fail(FB_EINVAL, "fb_fem_resync_delta is for unsharded handles whose plan was built on the device");
  if (n_removed < 0 || n_changed < 0 || n_added < 0 || n_new_nodes < 0 || n_fixed_dofs < 0) return fail(FB_EINVAL, "negative count");
  if ((n_removed && !removed) || (n_changed && (!changed_ids || !changed_nodes)) || (n_added && !added_tets) || (n_new_nodes && !new_xyz) || (n_fixed_dofs && !fixed_dofs))
    return fail(FB_EINVAL, "null array with a non-zero count");
  const int nt_old = h->plan.n_tets;
  const long long n_new = (long long)h->plan.n_global + n_new_nodes, nt_new = (long long)nt_old - n_removed + n_added;
  if (n_new >= (1LL << 31) - 2 || nt_new >= (1LL << 28)) return fail(FB_EINVAL, "mesh too large");
  if (nt_new < 1) return fail(FB_EINVAL, "the change leaves no element");
  for (int k = 0; k < n_removed; k++)
    if (removed[k] < 0 || removed[k] >= nt_old || (k && removed[k] <= removed[k - 1])) return fail(FB_EINVAL, "removed[%d] = %d: ids must ascend inside [0,%d)", k, removed[k], nt_old);
  for (int k = 0, r = 0; k < n_changed; k++) {
    if (changed_ids[k] < 0 || changed_ids[k] >= nt_old || (k && changed_ids[k] <= changed_ids[k - 1]))
      return fail(FB_EINVAL, "changed_ids[%d] = %d: ids must ascend inside [0,%d)", k, changed_ids[k], nt_old);
    while (r < n_removed && removed[r] < changed_ids[k]) r++;
    if (r < n_removed && removed[r] == changed_ids[k]) return fail(FB_EINVAL, "element %d is both removed and changed", changed_ids[k]);
  }
  for (long long k = 0; k < 4LL * n_changed; k++)
    if (changed_nodes[k] < 0 || changed_nodes[k] >= n_new) return fail(FB_EINVAL, "changed element %d references node %d outside [0,%lld)", changed_ids[k / 4], changed_nodes[k], n_new);
  for (long long k = 0; k < 4LL * n_added; k++)
    if (added_tets[k] < 0 || added_tets[k] >= n_new) return fail(FB_EINVAL, "added element %lld references node %d outside [0,%lld)", k / 4, added_tets[k], n_new);
  for (int k = 0; k < n_fixed_dofs; k++) {
    if (fixed_dofs[k] < 0 || fixed_dofs[k] >= 3 * n_new) return fail(FB_EINVAL, "constrained DOF %d out of range [0,%lld)", fixed_dofs[k], 3 * n_new);
    if (k && fixed_dofs[k] <= fixed_dofs[k - 1]) return fail(FB_EINVAL, "constrained DOFs must be strictly ascending (index %d)", k);
  }
  FB_HIP(hipStreamSynchronize(h->stream));
  h->poisoned = true;
  h->system_valid = false;
  FB_TRY(resync_delta(h, n_removed, removed, n_changed, changed_ids, changed_nodes, n_added, added_tets, n_new_nodes, new_xyz, n_fixed_dofs, fixed_dofs));
  h->poisoned = false;
  return FB_OK;
}

int fb_fem_resync_path(fb_fem_t h) { return h ? h->last_resync_path : FB_RESYNC_FULL; }

// ---- fb_fem_cut (subdivide.h) ----
int fb_fem_cut(fb_fem_t h, int n_strip_points, const double* strip_xyz, int mode, int modify, fb_cut_result* out) {
  CHECK_HANDLE(h);
  if (out) memset(out, 0, sizeof(*out));
  if (h->plan.n_ranks > 1 || !h->device_plan) return fail(FB_EINVAL, "fb_fem_cut is for unsharded handles whose plan was built on the device");
  if (mode != FB_CUT_BAKE && mode != FB_CUT_CARRY) return fail(FB_EINVAL, "cut mode %d: FB_CUT_BAKE or FB_CUT_CARRY", mode);
  std::vector<double> quads;
  FB_TRY(cut_quads(n_strip_points, strip_xyz, quads));
  hipStream_t s = h->stream;
  CutWork& C = h->cut;
  C.valid = false;
  C.mode = mode;
  C.n_quads = (int)(quads.size() / 12);
  C.n_cut = C.n_a = C.n_b = C.n_unhandled = C.n_edges = C.n_added = 0;
  C.min_ratio = 0.0;
  C.min_volume = 0.0;
  C.unhandled_ids.clear();
  C.unhandled_codes.clear();
  bool delta = false;
  int status = FB_CUT_NOTHING;
  const int n_old = h->plan.n_global, nt_old = h->plan.n_tets;
  const int* caller_of = h->ren.active ? h->ren.d_old_of_new.p : nullptr;
  const int* internal_of = h->ren.active ? h->ren.d_new_of_old.p : nullptr;
  if (C.n_quads) {
    FB_TRY(C.quads.alloc(quads.size()));
    FB_HIP(hipMemcpyAsync(C.quads.p, quads.data(), sizeof(double) * quads.size(), hipMemcpyHostToDevice, s));
    FB_TRY(cut_classify(s, C, nt_old, h->tets.p, caller_of, h->x0.p, h->q.p, h->plan_ws));
    if (C.n_unhandled) {
      status = FB_CUT_UNHANDLED;
      FB_TRY(cut_read_unhandled(s, C, h->plan_ws));
    } else if (C.n_cut) {
      FB_TRY(cut_emit(s, C, n_old, h->tets.p, caller_of, internal_of, h->x0.p, h->q.p, h->plan_ws));
      delta = true;
      status = modify ? FB_CUT_DONE : FB_CUT_DRY;
      if ((long long)n_old + 2LL * C.n_edges >= (1LL << 31) - 2 || (long long)nt_old - C.n_cut + C.n_added >= (1LL << 28)) return fail(FB_EINVAL, "mesh too large after the cut");
      // a split point on a node (t = 0 or |edge|) would leave a flat piece, which the rest state refuses after the point of no return
      if (modify && !(C.min_ratio > 0.0)) return fail(FB_EINVAL, "the cut would leave a piece without volume (smallest piece / parent volume %g)", C.min_ratio);
      // ... and so would a piece the records cannot hold: every handle keeps the rest volumes as floats (volf, and the element records of fp32
      // storage, which FB_MATRIX_AUTO may choose at any later re-sync).  Below FLT_MIN a float loses bits and from 1.4e-45 down it is zero: the
      // piece then weighs and resists nothing, and a node that lies in such pieces only gets an empty row.  k_tet_rest itself is fp64 and would
      // accept the piece (its determinant is not zero), so this is checked here, before anything changes.
      if (modify && !((float)C.min_volume >= FLT_MIN))
        return fail(FB_EINVAL, "the cut would leave a piece of volume %g, which the fp32 element records cannot hold (below %g; smallest piece / parent volume %g)",
                    C.min_volume, (double)FLT_MIN, C.min_ratio);
    }
  }
  C.valid = true;
  C.n_nodes = n_old;
  if (out) {
    out->status = status;
    out->n_quads = C.n_quads;
    out->n_case_a = C.n_a; out->n_case_b = C.n_b; out->n_unhandled = C.n_unhandled;
    if (delta) {
      out->n_cut_edges = C.n_edges;
      out->n_removed = C.n_cut; out->n_added = C.n_added; out->n_new_nodes = 2 * C.n_edges;
      out->min_volume_ratio = C.min_ratio;
    }
  }
  if (status != FB_CUT_DONE) return FB_OK;
  // ---- the point of no return ----
  const int n_new = n_old + 2 * C.n_edges;
  const bool newmark = h->prm.integrator == FB_INTEGRATOR_NEWMARK;
  const int n_vec = newmark ? 3 : 2;
  const size_t len = (size_t)3 * n_new;
  h->poisoned = true;
  h->system_valid = false;
  if (mode == FB_CUT_CARRY) {  // the state in the caller's order, new nodes interpolated
    FB_TRY(h->carry.reserve(len * n_vec));
    const DevBuf<double>* src[3] = {&h->q, &h->qvel, &h->qacc};
    for (int v = 0; v < n_vec; v++) {
      double* dst = h->carry.p + len * v;
      if (h->ren.active) FB_TRY(gather_nodes(s, n_old, 3, src[v]->p, h->ren.d_new_of_old.p, dst));
      else FB_HIP(hipMemcpyAsync(dst, src[v]->p, sizeof(double) * 3 * (size_t)n_old, hipMemcpyDeviceToDevice, s));
      FB_TRY(cut_interpolate(s, C, n_old, dst));
    }
  } else {
    FB_TRY(cut_bake(s, 3LL * n_old, h->x0.p, h->q.p));  // the deformed shape is the new rest shape (Deformable.cpp:144-147)
  }
  const std::vector<int> fixed = h->fixed_caller;
  FB_TRY(resync_delta(h, C.n_cut, C.cut_tets.p, 0, nullptr, nullptr, C.n_added, reinterpret_cast<const int*>(C.added.p), 2 * C.n_edges, C.new_xyz.p, (int)fixed.size(),
                      fixed.data(), true));
  if (mode == FB_CUT_CARRY) {
    DevBuf<double>* dst[3] = {&h->q, &h->qvel, &h->qacc};
    for (int v = 0; v < n_vec; v++) {
      const double* src = h->carry.p + len * v;
      if (h->ren.active) FB_TRY(gather_nodes(s, n_new, 3, src, h->ren.d_old_of_new.p, dst[v]->p));
      else FB_HIP(hipMemcpyAsync(dst[v]->p, src, sizeof(double) * len, hipMemcpyDeviceToDevice, s));
    }
  }
  FB_HIP(hipStreamSynchronize(s));
  h->poisoned = false;
  return FB_OK;
}

int fb_fem_read_cut(fb_fem_t h, int* removed, int* added_tets, double* new_xyz, int* edge_nodes, double* edge_frac, int* unhandled_ids, int* unhandled_codes) {
  CHECK_HANDLE(h);
  const CutWork& C = h->cut;
  if (!C.valid) return fail(FB_EINVAL, "no fb_fem_cut has run on this handle");
  hipStream_t s = h->stream;
  const bool delta = C.n_cut > 0 && C.n_unhandled == 0;
  if (delta) {
    if (removed) FB_TRY(C.cut_tets.download(removed, (size_t)C.n_cut, s));
    if (added_tets) FB_TRY(C.added.download(reinterpret_cast<int4*>(added_tets), (size_t)C.n_added, s));
    if (new_xyz) FB_TRY(C.new_xyz.download(new_xyz, (size_t)6 * C.n_edges, s));
    if (edge_nodes || edge_frac) {
      std::vector<unsigned long long> keys((size_t)C.n_edges);
      std::vector<double> frac((size_t)C.n_edges);
      FB_TRY(C.ukeys.download(keys.data(), keys.size(), s));
      FB_TRY(C.frac.download(frac.data(), frac.size(), s));
      for (int k = 0; k < C.n_edges; k++)
        for (int c = 0; c < 2; c++) {
          if (edge_nodes) { edge_nodes[4 * k + 2 * c] = (int)(keys[k] >> 32); edge_nodes[4 * k + 2 * c + 1] = (int)(keys[k] & 0xffffffffu); }
          if (edge_frac) edge_frac[2 * k + c] = frac[k];
        }
    }
  }
  for (size_t k = 0; k < C.unhandled_ids.size(); k++) {
    if (unhandled_ids) unhandled_ids[k] = C.unhandled_ids[k];
    if (unhandled_codes) unhandled_codes[k] = C.unhandled_codes[k];
  }
  return FB_OK;
}

int fb_fem_read_mesh(fb_fem_t h, double* rest_xyz, int* tets) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_read_mesh is for unsharded handles");
  hipStream_t s = h->stream;
  const int n = h->plan.n_global, nt = h->plan.n_tets;
  if (rest_xyz) FB_TRY(download_owned(h, h->x0, rest_xyz));
  if (tets) {
    if (h->ren.active) {
      FB_TRY(h->tets_caller.alloc((size_t)nt));
      FB_HIP(hipMemcpyAsync(h->tets_caller.p, h->tets.p, sizeof(int4) * (size_t)nt, hipMemcpyDeviceToDevice, s));
      FB_TRY(relabel_tets(s, nt, h->tets_caller.p, n, h->ren.d_old_of_new.p));
      FB_TRY(h->tets_caller.download(reinterpret_cast<int4*>(tets), (size_t)nt, s));
    } else {
      FB_TRY(h->tets.download(reinterpret_cast<int4*>(tets), (size_t)nt, s));
    }
  }
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
  hipEvent_t e0, e1;
  FB_HIP(hipEventCreate(&e0));
  FB_HIP(hipEventCreate(&e1));
  int rc = FB_OK;
  auto median = [](std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
  for (int what = 0; what < 2 && rc == FB_OK; what++) {
    double* dst = what == 0 ? seconds_build : seconds_update;
    if (!dst) continue;
    std::vector<double> t;
    for (int r = 0; r < reps && rc == FB_OK; r++) {
      if (hipEventRecord(e0, h->stream) != hipSuccess) { rc = fail(FB_EDEVICE, "hipEventRecord failed"); break; }
      rc = what == 0 ? surface_ready(h, true) : surface_update(h->stream, h->surf, h->x0.p, h->q.p, true);
      if (rc != FB_OK) break;
      float ms = 0;
      if (hipEventRecord(e1, h->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
        rc = fail(FB_EDEVICE, "timing events failed");
        break;
      }
      t.push_back(ms * 1e-3);
    }
    if (rc == FB_OK) *dst = median(t);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
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

int fb_fem_set_uniform_force(fb_fem_t h, int axis, double value) {
  CHECK_HANDLE(h);
  if (axis < 0 || axis > 2) return fail(FB_EINVAL, "axis %d", axis);
  const int n = h->plan.n_local;
  hipLaunchKernelGGL(k_fill_axis, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, h->stream, n, axis, value, h->fext.p);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

namespace {
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
  if (info) {
    info->cg_iterations = total;
    info->converged = ok ? 1 : 0;
    info->assembly_seconds = asm_s;
    info->solve_seconds = solve_s;
    info->rho0 = fin.rho0;
    info->rho = fin.rho[fin.iter & 1];
    info->pcg_path = h->last_pcg_path;
    info->persist_fallbacks = h->ps.persist_fallbacks;
    info->newton_iterations = newton;
  }
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
  FB_HIP(hipEventRecord(h->ev[1], s));
  int iters = 0;
  CGState fin;
  FB_TRY(pcg_solve(h, h->rhs.p, h->prm.cg_eps, h->prm.cg_max_iter, &iters, &fin));
  FB_HIP(hipEventRecord(h->ev[2], s));
  const bool ok = iters >= 0;
  if (ok) {
    const int n = 3 * h->plan.n_owned;
    hipLaunchKernelGGL(k_state_update, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, s, n, h->x.p, h->dofmask.p, h->prm.timestep, h->q.p,
                       h->qvel.p);
    FB_HIP(hipGetLastError());
  }
  FB_HIP(hipStreamSynchronize(s));
  float ms_a = 0, ms_s = 0;
  FB_HIP(hipEventElapsedTime(&ms_a, h->ev[0], h->ev[1]));
  FB_HIP(hipEventElapsedTime(&ms_s, h->ev[1], h->ev[2]));
  h->last_assembly_s = ms_a * 1e-3; h->last_solve_s = ms_s * 1e-3;
  if (info) {
    info->cg_iterations = std::abs(iters);
    info->converged = ok ? 1 : 0;
    info->assembly_seconds = h->last_assembly_s;
    info->solve_seconds = h->last_solve_s;
    info->rho0 = fin.rho0;
    info->rho = fin.rho[fin.iter & 1];
    info->pcg_path = h->last_pcg_path;
    info->persist_fallbacks = h->ps.persist_fallbacks;
    info->newton_iterations = 1;
  }
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

int fb_fem_set_constrained_dofs(fb_fem_t h, int n_fixed_dofs, const int* fixed_dofs) {
  CHECK_HANDLE(h);
  if (n_fixed_dofs < 0 || (n_fixed_dofs > 0 && !fixed_dofs)) return fail(FB_EINVAL, "bad constrained DOF list");
  if (h->device_plan && h->plan.n_ranks == 1) {
    FB_TRY(device_constraint_masks(h->stream, h->plan.n_global, n_fixed_dofs, fixed_dofs, h->ren.active ? h->ren.d_new_of_old.p : nullptr, h->fixed_stage, h->dofmask, h->nodemask));
    h->plan.n_fixed_owned = n_fixed_dofs;
    h->fixed_caller.assign(fixed_dofs, fixed_dofs + n_fixed_dofs);
  } else if (!h->l2c.empty()) {  // a renumbered shard: the list in internal ids, ascending again
    const int r = 3 * h->plan.n_global;
    for (int i = 0; i < n_fixed_dofs; i++) {
      if (fixed_dofs[i] < 0 || fixed_dofs[i] >= r) return fail(FB_EINVAL, "constrained DOF %d out of range [0,%d)", fixed_dofs[i], r);
      if (i && fixed_dofs[i] <= fixed_dofs[i - 1]) return fail(FB_EINVAL, "constrained DOFs must be strictly ascending (index %d)", i);
    }
    std::vector<int> mapped((size_t)n_fixed_dofs);
    for (int i = 0; i < n_fixed_dofs; i++) mapped[i] = 3 * h->ren.new_of_old[fixed_dofs[i] / 3] + fixed_dofs[i] % 3;
    std::sort(mapped.begin(), mapped.end());
    FB_TRY(plan_set_constraints(h->plan, n_fixed_dofs, mapped.data()));
    FB_TRY(upload_masks(h));
  } else {
    FB_TRY(plan_set_constraints(h->plan, n_fixed_dofs, fixed_dofs));
    FB_TRY(upload_masks(h));
  }
  h->system_valid = false;
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
  FB_HIP(hipEventRecord(h->ev[0], h->stream));
  for (int r = 0; r < reps; r++) FB_TRY(pass());
  FB_HIP(hipEventRecord(h->ev[1], h->stream));
  FB_HIP(hipStreamSynchronize(h->stream));
  FB_HIP(hipGetLastError());
  float ms = 0;
  FB_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  *seconds_per_pass = ms * 1e-3 / reps;
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
  FB_HIP(hipEventRecord(h->ev[0], h->stream));
  for (int i = 0; i < reps; i++) FB_TRY(spmv(h, 3, h->d.p, h->Ad.p, h->r.p, h->part_a.p, 0));
  FB_HIP(hipEventRecord(h->ev[1], h->stream));
  FB_HIP(hipStreamSynchronize(h->stream));
  float ms = 0;
  FB_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  *seconds_per_spmv = ms * 1e-3 / reps;
  return FB_OK;
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
  FB_HIP(hipEventRecord(h->ev[0], h->stream));
  for (int i = 0; i < reps; i++) FB_TRY(assemble_system(h));
  FB_HIP(hipEventRecord(h->ev[1], h->stream));
  FB_HIP(hipStreamSynchronize(h->stream));
  float ms = 0;
  FB_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  *seconds_per_assembly = ms * 1e-3 / reps;
  return FB_OK;
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
