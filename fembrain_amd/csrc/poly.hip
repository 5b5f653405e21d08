// BlobTree field sweep, grid classification and the tetrahedral polygonizer on gfx950 -- the GPU side of
// PS::SKETCH::GPUPoly (reference src/implicit/OclPolygonizer.{h,cpp}) and PS::SKETCH::FieldComputer
// (src/implicit/FieldComputer.{h,cpp}); kernels replace data/opencl/Polygonizer.cl and Tetrahedralizer.cl.
//
// Design (MI355X): every pass is a flat HBM-bound sweep with one thread per grid point / cell and no host
// round trip (the reference does D2H + host scan + H2D between passes, OclPolygonizer.cpp:663-730):
//   sweep      float4 (x,y,z,f) per point, 16 B/lane coalesced stores + one inside bit per point (wave ballot)
//   classify   cell configs (u8) and edge flags (u8) from the 2 MB inside bitmask only; included-cell and
//              included-vertex bitmasks by ballot; per-64 popcounts
//   scan       exclusive scan of the per-word popcounts (n/64 entries) -- any thread then gets the rank of any
//              point/cell as base[word] + popc(mask[word] & lower bits): no full-size offset arrays
//   emit       tet-mesh vertices (grid order) and 6 tets per included cell (Tetrahedralizer.cl:67-132 pattern)
//
// Field semantics follow the reference CPU path FieldComputer::fieldValue / computePrimitiveField
// (src/implicit/Polygonizer.cpp:1544-2108) evaluated in scalar fp32 with its exact operation order:
// range operators SUM their primitives, and the running `outField` is carried from one operator to the next
// exactly as that code does.  Not reproduced (documented in DESIGN.md): its all-SIMD-lanes-outside bounding-box
// cull (depends on the host SIMD width), the rsqrt+Newton approximation (1/sqrt here), the rational pow of the
// Ricci blend (powf here).
//
// Field semantics are a property of the handle (fb_poly_set_field_semantics), compiled into the kernels as a template
// parameter so that the default path is untouched:
//   SEM_CPU (default)  the CPU path as described above, without computePrimitiveField's primitive box cull
//   SEM_CPU_BOX        the same WITH that cull (isOutsidePrim, Polygonizer.cpp:1485-1505,1548-1552), tested per point
//   SEM_OPENCL         the OpenCL kernel's evaluation (data/opencl/Polygonizer.cl:483-886) -- the path that wrote the .veg
//                      files the reference ships: binary operators evaluated by ComputeOpField(operator INDEX, ..) (:825),
//                      range operators by their own type, instanced nodes 0, over the `next` links of
//                      LinearBlobTree::setTraversalRoute (LinearBlobTree.cpp:333-429)
// Here: the handle, the drivers, the C ABI.  Kernels: poly_device.hip.h.  Host compiler: poly_program.h (types), poly_compile.cpp (compiler, support boxes, cube table).
#include "common.h"
#include "launch.hip.h"
#include "poly_program.h"
#include "poly_device.hip.h"  // (with `using namespace fb`)

namespace {
static_assert(kPB == fb::kB, "launch_1d sizes its workgroups by kB, the kernels index by kPB");

// ---- the kernels that evaluate the field, one row per semantics.  A handle stores its row where its semantics are set ----
struct SemKernels {
  int sem;
  decltype(&k_sweep<false, SEM_CPU>) sweep[2];  // [CULL]
  decltype(&k_field_array<SEM_CPU>) field_array;
  decltype(&k_surface_vertices<SEM_CPU>) surface_vertices;
  decltype(&k_off_surface<SEM_CPU>) off_surface;
};
#define FB_K_SEM(SEM) {SEM, {k_sweep<false, SEM>, k_sweep<true, SEM>}, k_field_array<SEM>, k_surface_vertices<SEM>, k_off_surface<SEM>}
const SemKernels kSemKernels[] = {FB_K_SEM(SEM_CPU_BOX), FB_K_SEM(SEM_OPENCL), FB_K_SEM(SEM_CPU)};
#undef FB_K_SEM

const SemKernels* sem_kernels(int sem) {
  for (const SemKernels& k : kSemKernels)
    if (k.sem == sem) return &k;
  return nullptr;
}

// The environment knobs of the polygonizer (development aids), read once, at fb_poly_create
struct PolyKnobs {
  bool classify_masks = false;  // FEMBRAIN_CLASSIFY_MASKS: k_classify always loads the masks, also where the rows are whole words
  int emit_blocks = 0;          // FB_EMIT_BLOCKS: workgroups of k_tet_elements; 0 = not set, emit_elements' rule
};

}  // namespace

struct fb_poly_s {
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<float> header, ops, prims, mtx;
  int n_ops = 0, n_prims = 0, n_mtx = 0;
  TreeProgram tp;  // the compiled program, its value slots and the primitives' support boxes
  DevBuf<Instr> d_prog;
  DevBuf<float> d_prims, d_mtx, d_pbox, d_cbox;
  std::vector<float> cbox;  // SEM_CPU_BOX: the reference's primitive boxes, given by the caller (fb_poly_set_field_semantics)
  int sem = SEM_CPU;
  const SemKernels* k = sem_kernels(SEM_CPU);  // the row of `sem`
  PolyKnobs knobs;
  Grid G;
  int gz_total = 0;  // point planes of the whole grid this one is a slab of (= G.g[2] for a grid of its own)
  bool have_grid = false, classified = false, tetra = false, materialized = false;
  DevBuf<float> fval;    // the field at every grid point, as k_sweep stores it
  DevBuf<float4> grid;   // (x, y, z, f) per point: materialised by fb_poly_read_grid only
  bool grid_current = false;
  DevBuf<unsigned long long> inside, cinc, vinc, lastx, lasty, lastz, valid, crossx, crossy, crossz, firstx, firsty, firstz;
  DevBuf<uint4> block_sums;                // k_classify -> k_ranks: included cells, tet vertices, crossed edges, surface cells per workgroup
  long long n_words = 0;
  DevBuf<unsigned char> config, flags;
  DevBuf<unsigned int> aux_pop, cbase, vbase, vsum;
  DevBuf<unsigned int> totals;  // [0] crossed edges [1] surface cells [2] included cells [3] tet vertices
  DevBuf<float> tv;
  DevBuf<uint4> tt;
  // marching-cubes surface
  bool surfaced = false;
  DevBuf<unsigned char> d_tri, d_nvert, d_edge_info;
  DevBuf<unsigned long long> surf;
  DevBuf<unsigned int> edge_pop, idx_pop, ebase, ibase, esum, isum;
  DevBuf<float> sv, sn, deformed, sfrac;
  DevBuf<uint2> sends, tlist;
  DevBuf<unsigned long long> elist;
  DevBuf<unsigned int> si;
  DevBuf<double> disp;
  fb_poly_counts counts;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // timed_reps: two; timed_stages: one before each of four stages and one after
};

namespace {

#define CHECK_POLY(h)                                    \
  if (!(h)) return fail(FB_EINVAL, "null poly handle"); \
  FB_HIP(hipSetDevice((h)->device))

TreeSource tree_source(const fb_poly_s* h, int sem) { return TreeSource{h->ops.data(), h->prims.data(), h->mtx.data(), h->n_ops, h->n_prims, h->n_mtx, sem}; }
size_t stack_bytes(const fb_poly_s* h) { return (size_t)std::max(1, h->tp.depth) * kPB * sizeof(float); }  // dynamic LDS of the kernels that evaluate the field

// the program (or one dummy step: keeps a valid pointer), the caller's boxes where the semantics have them, the support boxes
int upload_program(fb_poly_s* h) {
  static const Instr none = {};
  FB_TRY(h->tp.prog.empty() ? h->d_prog.upload(&none, 1, h->stream) : h->d_prog.upload(h->tp.prog, h->stream));
  if (!h->cbox.empty()) FB_TRY(h->d_cbox.upload(h->cbox, h->stream));
  support_boxes(tree_source(h, h->sem), &h->tp);
  return h->d_pbox.upload(h->tp.pbox, h->stream);
}

// what was computed on another grid, or under other semantics, is void
void void_results(fb_poly_s* h) { h->have_grid = h->classified = h->tetra = h->surfaced = false; }

// an output array of a count that may be 0: at least one element, so that the kernels get a valid pointer
template <class T>
int alloc_some(DevBuf<T>& b, size_t n) { return b.alloc(std::max<size_t>(1, n)); }

// the divisors that take a linear index apart on rows of x and planes of x * y
struct GridDivs { FastDiv xy, x; };
GridDivs grid_divs(unsigned int x, unsigned int y) { return GridDivs{fast_div(x * y), fast_div(x)}; }
GridDivs grid_divs(const Grid& G) { return grid_divs((unsigned int)G.g[0], (unsigned int)G.g[1]); }

// the float4 grid of the API from the stored field values, once per sweep
int materialize_grid(fb_poly_s* h) {
  if (h->grid_current) return FB_OK;
  const Grid& G = h->G;
  FB_TRY(h->grid.alloc((size_t)G.n_points));
  const GridDivs d = grid_divs(G);
  FB_TRY(launch_1d(k_grid_xyzf, G.n_points, h->stream, G, d.xy, d.x, h->fval.p, h->grid.p));
  h->grid_current = true;
  return FB_OK;
}

int do_sweep(fb_poly_s* h) {
  const Grid& G = h->G;
  h->grid_current = false;
  const int blocks = (int)((G.n_points + (long long)kPB * kSweepPts - 1) / ((long long)kPB * kSweepPts));
  const GridDivs d = grid_divs(G);
  const bool cull = h->n_prims > 2;  // with one or two primitives the box test costs more than it can save (sphere at 256^3: 66 vs 50 us)
  hipLaunchKernelGGL(h->k->sweep[cull], dim3(blocks), dim3(kPB), stack_bytes(h), h->stream, G, d.xy, d.x, h->d_prog.p, (int)h->tp.prog.size(), h->n_prims,
                     h->tp.depth, h->d_prims.p, h->d_mtx.p, h->d_pbox.p, h->d_cbox.p, h->fval.p, h->inside.p);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int set_grid(fb_poly_s* h, const float lo[3], float cellsize, const int dims[3], int z0 = 0, int gz_total = 0) {
  if (!(cellsize > 0)) return fail(FB_EINVAL, "cellsize must be positive");
  Grid G;
  G.cellsize = cellsize;
  G.z0 = z0;
  h->gz_total = gz_total > 0 ? gz_total : dims[2];
  G.n_points = 1; G.n_cells = 1;
  for (int a = 0; a < 3; a++) {
    if (dims[a] < 2) return fail(FB_EINVAL, "grid needs at least 2 points per axis");
    G.lo[a] = lo[a]; G.g[a] = dims[a]; G.c[a] = dims[a] - 1;
    G.n_points *= dims[a]; G.n_cells *= (dims[a] - 1);
  }
  if (G.n_points >= (1LL << 31)) return fail(FB_EINVAL, "grid too large");
  h->G = G;
  const size_t pw = (size_t)((G.n_points + 63) / 64);
  FB_TRY(h->fval.alloc((size_t)G.n_points));
  h->grid_current = false;
  DevBuf<unsigned long long>* masks[] = {&h->inside, &h->cinc, &h->vinc, &h->lastx, &h->lasty, &h->lastz, &h->valid, &h->crossx, &h->crossy, &h->crossz,
                                         &h->surf, &h->firstx, &h->firsty, &h->firstz};
  for (auto* m : masks) FB_TRY(m->alloc(pw + 1));
  h->n_words = (long long)pw;
  FB_TRY(h->vbase.alloc(pw));
  FB_TRY(h->cbase.alloc(pw));
  FB_TRY(h->aux_pop.alloc(pw));
  const size_t pch = (pw + kChunk - 1) / kChunk;
  if (pch > 16 * kPB) return fail(FB_EINVAL, "grid too large for the chunked scan");
  FB_TRY(h->vsum.alloc(pch));  // (sized per chunk: the surface pass's scans and the emission grids read its length)
  FB_TRY(h->block_sums.alloc((pw + kPB - 1) / kPB));
  DevBuf<unsigned int>* words[] = {&h->edge_pop, &h->idx_pop, &h->ebase, &h->ibase};
  for (auto* m : words) FB_TRY(m->alloc(pw));
  FB_TRY(h->esum.alloc(pch));
  FB_TRY(h->isum.alloc(pch));
  FB_TRY(h->config.alloc((size_t)G.n_cells));
  FB_TRY(h->flags.alloc((size_t)G.n_points));
  FB_TRY(h->totals.alloc(6));
  FB_TRY(launch_1d(k_grid_masks, G.n_points, h->stream, G, h->lastx.p, h->lasty.p, h->lastz.p, h->valid.p, h->firstx.p, h->firsty.p, h->firstz.p));
  h->materialized = false;
  void_results(h);
  return FB_OK;
}

// fb_poly_sweep_grid and fb_poly_sweep_slab: the grid (a slab: planes z0.. of a grid of gz_total), its sweep, and the wait
int sweep_new_grid(fb_poly_s* h, const float lo[3], float cellsize, const int dims[3], int z0 = 0, int gz_total = 0) {
  FB_TRY(set_grid(h, lo, cellsize, dims, z0, gz_total));
  FB_TRY(do_sweep(h));
  FB_HIP(hipStreamSynchronize(h->stream));
  h->have_grid = true;
  return FB_OK;
}

int do_classify(fb_poly_s* h) {
  const Grid& G = h->G;
  const long long pw = h->n_words;  // a thread per mask word, in both kernels
  const bool rows64 = G.g[0] % 64 == 0 && pw < (1LL << 31) && !h->knobs.classify_masks;
  const unsigned int wpr = (unsigned int)(G.g[0] / 64);
  const GridDivs d = rows64 ? grid_divs(wpr, (unsigned int)G.g[1]) : grid_divs(1u, 1u);
  FB_TRY(launch_1d(rows64 ? k_classify<true> : k_classify<false>, pw, h->stream, G, d.xy, d.x, pw, h->inside.p, h->lastx.p, h->lasty.p, h->lastz.p, h->firstx.p,
                   h->firsty.p, h->firstz.p, h->valid.p, h->cinc.p, h->crossx.p, h->crossy.p, h->crossz.p, h->vinc.p, h->aux_pop.p, h->block_sums.p));
  FB_TRY(launch_1d(k_ranks, pw, h->stream, pw, h->cinc.p, h->vinc.p, h->block_sums.p, h->cbase.p, h->vbase.p, h->totals.p));
  h->materialized = false;
  return FB_OK;
}

int fetch_counts(fb_poly_s* h) {
  unsigned int t[4];
  FB_TRY(h->totals.download(t, 4, h->stream));
  fb_poly_counts& c = h->counts;
  memset(&c, 0, sizeof c);
  for (int a = 0; a < 3; a++) c.grid[a] = h->G.g[a];
  c.n_points = (int)h->G.n_points; c.n_cells = (int)h->G.n_cells;
  c.n_crossed_edges = (int)t[0]; c.n_surface_cells = (int)t[1];
  c.n_included_cells = (int)t[2]; c.n_tet_vertices = (int)t[3];
  c.n_tets = 6 * c.n_included_cells;
  return FB_OK;
}

// the two launches of do_emit, which fb_poly_time_stages times one by one
int emit_vertices(fb_poly_s* h) {
  const Grid& G = h->G;
  const GridDivs d = grid_divs(G);
  hipLaunchKernelGGL(k_tet_vertices, dim3((unsigned)((((G.n_points + 63) >> 6) + kVW - 1) / kVW)), dim3(kPB), 0, h->stream, G, d.xy, d.x, h->vinc.p, h->vbase.p, h->tv.p);
  FB_HIP(hipGetLastError());
  return FB_OK;
}
int emit_elements(fb_poly_s* h) {
  const Grid& G = h->G;
  // each wave owns a run of mask words: 4 words per wave measured best at 256^3 (16,384 blocks: 235 us pipeline; 16 words 249 us,
  // 1 word 323 us) -- the loaded waves sit in the part of the grid the surface encloses, shorter runs spread them over more CUs
  const long long words = (G.n_points + 63) / 64;
  const int pb = (int)std::min<long long>((G.n_points + kPB - 1) / kPB, h->knobs.emit_blocks > 0 ? h->knobs.emit_blocks : std::max<long long>(1, (words + 15) / 16));
  hipLaunchKernelGGL(k_tet_elements, dim3(pb), dim3(kPB), 0, h->stream, G, h->cinc.p, h->cbase.p, h->vinc.p, h->vbase.p, h->tt.p);
  FB_HIP(hipGetLastError());
  return FB_OK;
}
int do_emit(fb_poly_s* h) { FB_TRY(emit_vertices(h)); return emit_elements(h); }

// scans + emission of the marching-cubes surface; totals[4] = surface vertices, totals[5] = triangle indices
int do_surface_counts(fb_poly_s* h) {
  const long long pw = h->n_words;
  const int pch = (int)h->vsum.n;
  FB_TRY(launch_1d(k_surface_pops, pw, h->stream, h->G, pw, h->inside.p, h->lastx.p, h->lasty.p, h->lastz.p, h->valid.p, h->aux_pop.p, h->d_nvert.p, h->surf.p,
                   h->edge_pop.p, h->idx_pop.p));
  ScanJobs jobs;
  jobs.j[0] = ScanJob{h->edge_pop.p, nullptr, h->esum.p, nullptr, h->ebase.p, h->totals.p + 4, nullptr};
  jobs.j[1] = ScanJob{h->idx_pop.p, nullptr, h->isum.p, nullptr, h->ibase.p, h->totals.p + 5, nullptr};
  hipLaunchKernelGGL(k_chunk_sums, dim3(pch, 2), dim3(kPB), 0, h->stream, jobs, (int)pw);
  FB_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_scan_chunks, dim3(2), dim3(kPB), 0, h->stream, jobs, pch);
  FB_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_chunk_scan, dim3(pch, 2), dim3(kPB), 0, h->stream, jobs, (int)pw);
  FB_HIP(hipGetLastError());
  return FB_OK;
}

int do_surface_emit(fb_poly_s* h) {
  const Grid& G = h->G;
  const long long pw = h->n_words;
  const long long nv = h->counts.n_surface_vertices, ntri = h->counts.n_surface_indices / 3;
  if (nv == 0 && ntri == 0) return FB_OK;
  FB_TRY(launch_1d(k_surface_lists, pw, h->stream, G, pw, h->inside.p, h->surf.p, h->crossx.p, h->crossy.p, h->crossz.p, h->ebase.p, h->ibase.p, h->d_nvert.p,
                   h->elist.p, h->tlist.p));
  if (nv > 0) {
    hipLaunchKernelGGL(h->k->surface_vertices, dim3((int)((nv + kPB - 1) / kPB)), dim3(kPB), stack_bytes(h), h->stream, G, nv, h->elist.p, h->d_prog.p,
                       (int)h->tp.prog.size(), h->n_prims, h->d_prims.p, h->d_mtx.p, h->d_cbox.p, h->fval.p, h->vinc.p, h->vbase.p, h->sv.p, h->sn.p, h->sends.p, h->sfrac.p);
    FB_HIP(hipGetLastError());
  }
  if (ntri > 0) FB_TRY(launch_1d(k_surface_elements, ntri, h->stream, G, ntri, h->tlist.p, h->crossx.p, h->crossy.p, h->crossz.p, h->ebase.p, h->d_tri.p, h->d_edge_info.p, h->si.p));
  return FB_OK;
}

// number of set bits of a scanned mask below bit `bit` (base[w] = set bits before word w)
int count_before(fb_poly_s* h, const DevBuf<unsigned long long>& mask, const DevBuf<unsigned int>& base, long long bit, unsigned int total, unsigned int* out) {
  if (bit >= h->G.n_points) { *out = total; return FB_OK; }
  unsigned long long w = 0;
  unsigned int b = 0;
  FB_TRY(mask.download(&w, 1, h->stream, (size_t)(bit >> 6)));
  FB_TRY(base.download(&b, 1, h->stream, (size_t)(bit >> 6)));
  *out = b + (unsigned int)__builtin_popcountll(w & ((1ULL << (bit & 63)) - 1ULL));
  return FB_OK;
}

struct SlabRange { unsigned int v0, v1, c0, c1; };  // owned vertices [v0, v1) and included cells [c0, c1) in the slab's own numbering

int slab_range(fb_poly_s* h, int own_first_plane, int own_planes, int own_layers, SlabRange* r) {
  if (!h->tetra) return fail(FB_EINVAL, "tetrahedralize first");
  const Grid& G = h->G;
  const int p0 = own_first_plane - G.z0, p1 = p0 + own_planes, l1 = p0 + own_layers;
  if (own_planes < 0 || own_layers < 0 || p0 < 0 || p1 > G.g[2] || l1 > G.c[2])
    return fail(FB_EINVAL, "planes [%d, %d) / layers [%d, %d) are not inside the slab [%d, %d)", own_first_plane, own_first_plane + own_planes,
                own_first_plane, own_first_plane + own_layers, G.z0, G.z0 + G.g[2]);
  // the vertex marks of a plane are complete only if both cell layers next to it were classified here (or do not exist)
  if (p0 == 0 && G.z0 > 0 && own_planes > 0) return fail(FB_EINVAL, "the slab must start one plane below the first owned plane %d", own_first_plane);
  if (own_layers > 0 && l1 + 1 > G.c[2] && G.z0 + G.g[2] < h->gz_total)
    return fail(FB_EINVAL, "the slab must reach two planes above the last owned cell layer %d", own_first_plane + own_layers - 1);
  const long long gxy = (long long)G.g[0] * G.g[1];
  const unsigned int nv = (unsigned int)h->counts.n_tet_vertices, nc = (unsigned int)(h->counts.n_tets / 6);
  FB_TRY(count_before(h, h->vinc, h->vbase, p0 * gxy, nv, &r->v0));
  FB_TRY(count_before(h, h->vinc, h->vbase, p1 * gxy, nv, &r->v1));
  FB_TRY(count_before(h, h->cinc, h->cbase, p0 * gxy, nc, &r->c0));
  FB_TRY(count_before(h, h->cinc, h->cbase, l1 * gxy, nc, &r->c1));
  return FB_OK;
}

}  // namespace

namespace fb {
int poly_device_tetmesh(fb_poly_t h, DeviceTetMesh* out) {
  CHECK_POLY(h);
  if (!h->tetra) return fail(FB_EINVAL, "tetrahedralize first");
  FB_HIP(hipStreamSynchronize(h->stream));
  out->device = h->device; out->n_vertices = h->counts.n_tet_vertices; out->n_tets = h->counts.n_tets;
  out->xyz = h->tv.p; out->tets = h->tt.p;
  return FB_OK;
}
int poly_device_surface(fb_poly_t h, DeviceSurface* out) {
  CHECK_POLY(h);
  if (!h->surfaced) return fail(FB_EINVAL, "run fb_poly_surface first");
  FB_HIP(hipStreamSynchronize(h->stream));
  out->device = h->device; out->n_vertices = h->counts.n_surface_vertices; out->n_triangles = h->counts.n_surface_indices / 3;
  out->xyz = h->sv.p; out->indices = h->si.p;
  return FB_OK;
}
}  // namespace fb

extern "C" {

int fb_poly_create(fb_poly_t* out, int device, const float* header12, int n_ops, const float* ops16, int n_prims, const float* prims20,
                   int n_mtx, const float* mtx12) {
  if (!out || !header12 || n_prims < 1 || !prims20 || n_ops < 0 || (n_ops > 0 && !ops16) || n_mtx < 1 || !mtx12)
    return fail(FB_EINVAL, "bad BlobTree arrays (need >= 1 primitive and the identity matrix node)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FB_EDEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(FB_EINVAL, "device %d out of range", device);
  FB_HIP(hipSetDevice(device));
  fb_poly_s* h = new fb_poly_s;
  h->device = device;
  if (const char* e = getenv("FEMBRAIN_CLASSIFY_MASKS")) h->knobs.classify_masks = atoi(e) != 0;
  if (const char* e = getenv("FB_EMIT_BLOCKS")) h->knobs.emit_blocks = atoi(e);
  h->header.assign(header12, header12 + 12);
  h->ops.assign(ops16, ops16 + 16 * (size_t)n_ops);
  h->prims.assign(prims20, prims20 + 20 * (size_t)n_prims);
  h->mtx.assign(mtx12, mtx12 + 12 * (size_t)n_mtx);
  h->n_ops = n_ops; h->n_prims = n_prims; h->n_mtx = n_mtx;
  int rc = FB_OK;
  for (int i = 0; i < n_prims && rc == FB_OK; i++) {
    const int im = (int)h->prims[20 * (size_t)i + 1];
    if (im < 0 || im >= n_mtx) rc = fail(FB_EINVAL, "primitive %d references matrix %d of %d", i, im, n_mtx);
  }
  if (rc == FB_OK) rc = compile_tree(tree_source(h, h->sem), &h->tp);
  if (rc == FB_OK && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(FB_EDEVICE, "hipStreamCreate failed");
  for (auto& e : h->ev)
    if (rc == FB_OK && hipEventCreate(&e) != hipSuccess) rc = fail(FB_EDEVICE, "hipEventCreate failed");
  if (rc == FB_OK) rc = h->d_prims.upload(h->prims, h->stream);
  if (rc == FB_OK) rc = h->d_mtx.upload(h->mtx, h->stream);
  if (rc == FB_OK) rc = upload_program(h);
  const CubeTable& ct = cube_table();
  if (rc == FB_OK) rc = h->d_tri.upload(&ct.tri[0][0], sizeof ct.tri, h->stream);
  if (rc == FB_OK) rc = h->d_nvert.upload(ct.nvert, sizeof ct.nvert, h->stream);
  if (rc == FB_OK) rc = h->d_edge_info.upload(ct.edge_info, sizeof ct.edge_info, h->stream);
  if (rc != FB_OK) {
    std::string keep = last_error();
    fb_poly_destroy(h);
    last_error() = keep;
    return rc;
  }
  *out = h;
  return FB_OK;
}

int fb_poly_compile_info(int n_ops, const float* ops16, int n_prims, const float* prims20, int* n_steps, int* n_slots) {
  if (n_prims < 1 || !prims20 || n_ops < 0 || (n_ops > 0 && !ops16)) return fail(FB_EINVAL, "bad BlobTree arrays");
  TreeProgram tp;
  FB_TRY(compile_tree(TreeSource{ops16, prims20, nullptr, n_ops, n_prims, 0, SEM_CPU}, &tp));
  if (n_steps) *n_steps = (int)tp.prog.size();
  if (n_slots) *n_slots = tp.depth;
  return FB_OK;
}

int fb_poly_set_field_semantics(fb_poly_t h, int semantics, const float* prim_boxes6) {
  CHECK_POLY(h);
  if (semantics != SEM_CPU && semantics != SEM_CPU_BOX && semantics != SEM_OPENCL) return fail(FB_EINVAL, "unknown field semantics %d", semantics);
  if (semantics == SEM_CPU_BOX && !prim_boxes6) return fail(FB_EINVAL, "FB_FIELD_CPU_BOX needs the primitive boxes (6 floats per primitive)");
  FB_HIP(hipStreamSynchronize(h->stream));
  TreeProgram next;
  FB_TRY(compile_tree(tree_source(h, semantics), &next));  // a refusal: the handle keeps working with the semantics it had
  h->sem = semantics;
  h->k = sem_kernels(semantics);
  h->tp.prog = std::move(next.prog);
  h->tp.depth = next.depth;
  h->cbox.clear();
  if (semantics == SEM_CPU_BOX) h->cbox.assign(prim_boxes6, prim_boxes6 + 6 * (size_t)h->n_prims);
  FB_TRY(upload_program(h));
  FB_HIP(hipStreamSynchronize(h->stream));
  void_results(h);  // results of the old semantics
  return FB_OK;
}

int fb_poly_field_semantics(fb_poly_t h) { return h ? h->sem : FB_EINVAL; }

int fb_poly_destroy(fb_poly_t h) {
  if (!h) return FB_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (auto& e : h->ev)
    if (e) (void)hipEventDestroy(e);
  hipStream_t s = h->stream;
  delete h;
  if (s) (void)hipStreamDestroy(s);
  return FB_OK;
}

int fb_poly_field_array(fb_poly_t h, int n, float* xyzf) {
  CHECK_POLY(h);
  if (n < 0 || (n > 0 && !xyzf)) return fail(FB_EINVAL, "bad point array");  // PS::SKETCH error codes, OclPolygonizer.h:26-33
  if (n == 0) return FB_OK;
  DevBuf<float4> pts;
  FB_TRY(pts.upload((const float4*)xyzf, (size_t)n, h->stream));
  hipLaunchKernelGGL(h->k->field_array, dim3(ceil_div(n, kPB)), dim3(kPB), stack_bytes(h), h->stream, n, h->d_prog.p, (int)h->tp.prog.size(), h->n_prims, h->d_prims.p,
                     h->d_mtx.p, h->d_cbox.p, pts.p);
  FB_HIP(hipGetLastError());
  return pts.download((float4*)xyzf, (size_t)n, h->stream);
}

int fb_poly_sweep_grid(fb_poly_t h, const float lower[3], float cellsize, const int dims[3]) {
  CHECK_POLY(h);
  if (!lower || !dims) return fail(FB_EINVAL, "null grid description");
  return sweep_new_grid(h, lower, cellsize, dims);
}

int fb_poly_sweep_slab(fb_poly_t h, const float lower[3], float cellsize, const int dims[3], int z_first, int z_count) {
  CHECK_POLY(h);
  if (!lower || !dims) return fail(FB_EINVAL, "null grid description");
  if (z_first < 0 || z_count < 2 || z_first + z_count > dims[2]) return fail(FB_EINVAL, "slab planes [%d, %d) do not fit a grid of %d planes", z_first, z_first + z_count, dims[2]);
  const int sub[3] = {dims[0], dims[1], z_count};
  return sweep_new_grid(h, lower, cellsize, sub, z_first, dims[2]);
}

int fb_poly_slab_counts(fb_poly_t h, int own_first_plane, int own_planes, int own_layers, int* n_vertices, int* n_tets) {
  CHECK_POLY(h);
  SlabRange r;
  FB_TRY(slab_range(h, own_first_plane, own_planes, own_layers, &r));
  if (n_vertices) *n_vertices = (int)(r.v1 - r.v0);
  if (n_tets) *n_tets = (int)(6 * (r.c1 - r.c0));
  return FB_OK;
}

int fb_poly_read_tetmesh_slab(fb_poly_t h, int own_first_plane, int own_planes, int own_layers, unsigned int vertex_base, float* xyz, unsigned int* tets) {
  CHECK_POLY(h);
  SlabRange r;
  FB_TRY(slab_range(h, own_first_plane, own_planes, own_layers, &r));
  if (xyz && r.v1 > r.v0) FB_TRY(h->tv.download(xyz, 3 * (size_t)(r.v1 - r.v0), h->stream, 3 * (size_t)r.v0));
  const long long nt = 6LL * (r.c1 - r.c0);
  if (tets && nt > 0) {
    DevBuf<uint4> out;
    FB_TRY(out.alloc((size_t)nt));
    // a vertex's number in the whole grid = its number here - (vertices of the planes below the owned ones) + vertex_base
    FB_TRY(launch_1d(k_renumber_tets, nt, h->stream, nt, h->tt.p + 6 * (size_t)r.c0, vertex_base - r.v0, out.p));
    FB_TRY(out.download((uint4*)tets, (size_t)nt, h->stream));
  }
  return FB_OK;
}

int fb_poly_sweep(fb_poly_t h, float cellsize, int dims_out[3]) {
  CHECK_POLY(h);
  if (cellsize < 0.01f) return fail(FB_EINVAL, "cellsize %g below the reference minimum 0.01 (GPUPoly::run)", cellsize);
  // OclPolygonizer.cpp:1363-1378: cells = ceil(extent / cellsize) + 1 per axis, points = cells + 1, origin = bbox lower
  float lo[3] = {h->header[0], h->header[1], h->header[2]};
  int dims[3];
  for (int a = 0; a < 3; a++) {
    const float extent = h->header[4 + a] - h->header[a];
    dims[a] = (int)ceilf(extent / cellsize) + 2;
  }
  if (dims_out) memcpy(dims_out, dims, sizeof dims);
  return fb_poly_sweep_grid(h, lo, cellsize, dims);
}

int fb_poly_read_grid(fb_poly_t h, float* xyzf) {
  CHECK_POLY(h);
  if (!h->have_grid || !xyzf) return fail(FB_EINVAL, "no swept grid / null buffer");
  FB_TRY(materialize_grid(h));
  return h->grid.download((float4*)xyzf, (size_t)h->G.n_points, h->stream);
}

int fb_poly_classify(fb_poly_t h, fb_poly_counts* counts) {
  CHECK_POLY(h);
  if (!h->have_grid) return fail(FB_EINVAL, "sweep the grid first");
  FB_TRY(do_classify(h));
  FB_TRY(fetch_counts(h));
  h->classified = true;
  h->surfaced = false;
  if (counts) *counts = h->counts;
  return FB_OK;
}

int fb_poly_read_classification(fb_poly_t h, unsigned char* edge_flags, unsigned int* edge_counts, unsigned char* cell_configs) {
  CHECK_POLY(h);
  if (!h->classified) return fail(FB_EINVAL, "classify first");
  const size_t np = (size_t)h->G.n_points;
  if (!h->materialized) {
    FB_TRY(launch_1d(k_materialize, (long long)np, h->stream, h->G, h->inside.p, h->crossx.p, h->crossy.p, h->crossz.p, h->flags.p, h->config.p));
    h->materialized = true;
  }
  if (edge_flags || edge_counts) {
    std::vector<unsigned char> f(np);
    FB_TRY(h->flags.download(f.data(), np, h->stream));
    if (edge_flags) memcpy(edge_flags, f.data(), np);
    if (edge_counts)
      for (size_t i = 0; i < np; i++) edge_counts[i] = (unsigned int)__builtin_popcount(f[i]);
  }
  if (cell_configs) FB_TRY(h->config.download(cell_configs, (size_t)h->G.n_cells, h->stream));
  return FB_OK;
}

int fb_poly_tetrahedralize(fb_poly_t h, fb_poly_counts* counts) {
  CHECK_POLY(h);
  if (!h->classified) return fail(FB_EINVAL, "classify first");
  FB_TRY(alloc_some(h->tv, 3 * (size_t)h->counts.n_tet_vertices));
  FB_TRY(alloc_some(h->tt, (size_t)h->counts.n_tets));
  FB_TRY(do_emit(h));
  FB_HIP(hipStreamSynchronize(h->stream));
  h->tetra = true;
  if (counts) *counts = h->counts;
  return FB_OK;
}

int fb_poly_read_tetmesh(fb_poly_t h, float* xyz, unsigned int* tets) {
  CHECK_POLY(h);
  if (!h->tetra) return fail(FB_EINVAL, "tetrahedralize first");
  if (xyz) FB_TRY(h->tv.download(xyz, 3 * (size_t)h->counts.n_tet_vertices, h->stream));
  if (tets) FB_TRY(h->tt.download((uint4*)tets, (size_t)h->counts.n_tets, h->stream));
  return FB_OK;
}

int fb_poly_cube_table(unsigned char tri[4096], unsigned char nvert[256]) {
  const CubeTable& ct = cube_table();
  if (tri) memcpy(tri, ct.tri, sizeof ct.tri);
  if (nvert) memcpy(nvert, ct.nvert, sizeof ct.nvert);
  return FB_OK;
}

int fb_poly_surface(fb_poly_t h, fb_poly_counts* counts) {
  CHECK_POLY(h);
  if (!h->classified) return fail(FB_EINVAL, "classify first");
  FB_TRY(do_surface_counts(h));
  unsigned int t[2];
  FB_TRY(h->totals.download(t, 2, h->stream, 4));
  if ((int)t[0] != h->counts.n_crossed_edges) return fail(FB_EDEVICE, "surface vertex scan (%u) disagrees with the edge table (%d)", t[0], h->counts.n_crossed_edges);
  h->counts.n_surface_vertices = (int)t[0];
  h->counts.n_surface_indices = (int)t[1];
  const size_t nv = t[0], ni = t[1];
  for (auto* b : {&h->sv, &h->sn}) FB_TRY(alloc_some(*b, 3 * nv));
  FB_TRY(alloc_some(h->si, ni));
  FB_TRY(alloc_some(h->sends, nv));
  FB_TRY(alloc_some(h->sfrac, nv));
  FB_TRY(alloc_some(h->elist, nv));
  FB_TRY(alloc_some(h->tlist, ni / 3));
  FB_TRY(do_surface_emit(h));
  FB_HIP(hipStreamSynchronize(h->stream));
  h->surfaced = true;
  if (counts) *counts = h->counts;
  return FB_OK;
}

int fb_poly_read_surface(fb_poly_t h, float* xyz, float* normals, unsigned int* indices) {
  CHECK_POLY(h);
  if (!h->surfaced) return fail(FB_EINVAL, "run fb_poly_surface first");
  const size_t nv = 3 * (size_t)h->counts.n_surface_vertices;
  if (xyz) FB_TRY(h->sv.download(xyz, nv, h->stream));
  if (normals) FB_TRY(h->sn.download(normals, nv, h->stream));
  if (indices) FB_TRY(h->si.download(indices, (size_t)h->counts.n_surface_indices, h->stream));
  return FB_OK;
}

int fb_poly_apply_displacements(fb_poly_t h, int mesh, int n_dof, const double* displacements, float* xyz_out) {
  CHECK_POLY(h);
  const bool tet = mesh == FB_MESH_TET;
  if (mesh != FB_MESH_TET && mesh != FB_MESH_SURFACE) return fail(FB_EINVAL, "mesh must be FB_MESH_SURFACE or FB_MESH_TET");
  if (tet ? !h->tetra : !h->surfaced) return fail(FB_EINVAL, "no valid vertex buffer: polygonize first");  // m_isValidVertex
  const long long n = 3LL * (tet ? h->counts.n_tet_vertices : h->counts.n_surface_vertices);
  if (n_dof != n || !displacements) return fail(FB_EINVAL, "displacement vector has %d entries, the mesh has %lld", n_dof, n);
  if (n == 0) return FB_OK;
  FB_TRY(h->disp.upload(displacements, (size_t)n, h->stream));
  FB_TRY(h->deformed.alloc((size_t)n));
  FB_TRY(launch_1d(k_apply_displacements, n, h->stream, n, tet ? h->tv.p : h->sv.p, h->disp.p, h->deformed.p));
  if (xyz_out) return h->deformed.download(xyz_out, (size_t)n, h->stream);
  FB_HIP(hipStreamSynchronize(h->stream));
  return FB_OK;
}

int fb_poly_read_surface_colors(fb_poly_t h, float* rgba) {
  CHECK_POLY(h);
  if (!h->surfaced) return fail(FB_EINVAL, "run fb_poly_surface first");
  if (!rgba) return fail(FB_EINVAL, "null output");
  if (h->sem != SEM_CPU) return fail(FB_EINVAL, "the colour pass is built for FB_FIELD_CPU semantics only");
  const long long nv = h->counts.n_surface_vertices;
  if (nv == 0) return FB_OK;
  const long long kChunk = 1 << 16;
  DevBuf<float> scratch;
  DevBuf<float4> out;
  FB_TRY(scratch.alloc((size_t)5 * std::max(1, h->tp.depth) * (size_t)std::min(nv, kChunk)));
  FB_TRY(out.alloc((size_t)nv));
  for (long long first = 0; first < nv; first += kChunk) {
    const long long n = std::min(kChunk, nv - first), nth = std::min(nv, kChunk);
    FB_TRY(launch_1d(k_surface_colors, n, h->stream, first, n, h->sv.p, h->d_prog.p, (int)h->tp.prog.size(), h->n_prims, h->d_prims.p, h->d_mtx.p, scratch.p, nth, out.p));
  }
  return out.download((float4*)rgba, (size_t)nv, h->stream);
}

int fb_poly_field_color_array(fb_poly_t h, int n, float* xyzf, float* rgb) {
  CHECK_POLY(h);
  if (n < 0 || (n > 0 && (!xyzf || !rgb))) return fail(FB_EINVAL, "bad point array");
  if (h->sem != SEM_CPU) return fail(FB_EINVAL, "the colour pass is built for FB_FIELD_CPU semantics only");
  if (n == 0) return FB_OK;
  DevBuf<float4> pts;
  DevBuf<float> scratch, col;
  FB_TRY(pts.upload((const float4*)xyzf, (size_t)n, h->stream));
  FB_TRY(scratch.alloc((size_t)5 * std::max(1, h->tp.depth) * (size_t)n));
  FB_TRY(col.alloc((size_t)3 * n));
  FB_TRY(launch_1d(k_field_color_array, n, h->stream, n, pts.p, h->d_prog.p, (int)h->tp.prog.size(), h->n_prims, h->d_prims.p, h->d_mtx.p, scratch.p, n, col.p));
  FB_TRY(pts.download((float4*)xyzf, (size_t)n, h->stream));
  return col.download(rgb, (size_t)3 * n, h->stream);
}

int fb_poly_off_surface(fb_poly_t h, float len, float* xyzf_pairs) {
  CHECK_POLY(h);
  if (!h->surfaced) return fail(FB_EINVAL, "run fb_poly_surface first");
  if (!xyzf_pairs) return fail(FB_EINVAL, "null output");
  const long long nv = h->counts.n_surface_vertices;
  if (nv == 0) return FB_OK;
  DevBuf<float4> out;
  FB_TRY(out.alloc((size_t)(2 * nv)));
  hipLaunchKernelGGL(h->k->off_surface, dim3((int)((nv + kPB - 1) / kPB)), dim3(kPB), stack_bytes(h), h->stream, nv, len, h->sv.p, h->sn.p, h->d_prog.p,
                     (int)h->tp.prog.size(), h->n_prims, h->d_prims.p, h->d_mtx.p, h->d_cbox.p, out.p);
  FB_HIP(hipGetLastError());
  return out.download((float4*)xyzf_pairs, (size_t)(2 * nv), h->stream);
}

int fb_poly_time_surface(fb_poly_t h, int reps, double* seconds) {
  CHECK_POLY(h);
  if (!h->surfaced || reps < 1 || !seconds) return fail(FB_EINVAL, "run fb_poly_surface once first");
  // (same counts as the validated run: grid and tree are unchanged)
  return timed_reps(h, reps, [&] { FB_TRY(do_surface_counts(h)); return do_surface_emit(h); }, seconds);
}

int fb_poly_read_surface_binding(fb_poly_t h, unsigned int* tet_vertex_pairs, float* weights) {
  CHECK_POLY(h);
  if (!h->surfaced) return fail(FB_EINVAL, "run fb_poly_surface first");
  const size_t nv = (size_t)h->counts.n_surface_vertices;
  if (tet_vertex_pairs) FB_TRY(h->sends.download((uint2*)tet_vertex_pairs, nv, h->stream));
  if (weights) FB_TRY(h->sfrac.download(weights, nv, h->stream));
  return FB_OK;
}

int fb_poly_interpolate_displacements(fb_poly_t h, int n_tet_dof, const double* tet_displacements, float* xyz_out) {
  CHECK_POLY(h);
  if (!h->surfaced) return fail(FB_EINVAL, "run fb_poly_surface first");
  if (n_tet_dof != 3 * h->counts.n_tet_vertices || !tet_displacements)
    return fail(FB_EINVAL, "displacement vector has %d entries, the tet mesh of this grid has %d DOF", n_tet_dof, 3 * h->counts.n_tet_vertices);
  const long long nv = h->counts.n_surface_vertices;
  if (nv == 0) return FB_OK;
  FB_TRY(h->disp.upload(tet_displacements, (size_t)n_tet_dof, h->stream));
  FB_TRY(h->deformed.alloc((size_t)(3 * nv)));
  FB_TRY(launch_1d(k_interpolate_displacements, 3 * nv, h->stream, nv, h->sv.p, h->sends.p, h->sfrac.p, h->disp.p, h->deformed.p));
  if (xyz_out) return h->deformed.download(xyz_out, (size_t)(3 * nv), h->stream);
  FB_HIP(hipStreamSynchronize(h->stream));
  return FB_OK;
}

int fb_poly_time_pipeline(fb_poly_t h, int reps, double* sweep_seconds, double* pipeline_seconds) {
  CHECK_POLY(h);
  if (!h->tetra || reps < 1) return fail(FB_EINVAL, "run sweep, classify and tetrahedralize once first");
  const int pairs[][2] = {{0, 1}, {0, 2}};  // the sweep | with classification and emission (the validated run's counts: grid and tree are unchanged)
  double s[2];
  FB_TRY(timed_stages<2>(h, reps, [&](int k) { if (k == 0) return do_sweep(h); FB_TRY(do_classify(h)); return do_emit(h); }, pairs, s));
  if (sweep_seconds) *sweep_seconds = s[0];
  if (pipeline_seconds) *pipeline_seconds = s[1];
  return FB_OK;
}

int fb_poly_time_grid(fb_poly_t h, int reps, double* sweep_and_grid_seconds) {
  CHECK_POLY(h);
  if (!h->have_grid || reps < 1 || !sweep_and_grid_seconds) return fail(FB_EINVAL, "sweep a grid once first");
  FB_TRY(materialize_grid(h));  // (allocation outside the timed region)
  return timed_reps(h, reps, [&] { FB_TRY(do_sweep(h)); return materialize_grid(h); }, sweep_and_grid_seconds);
}

int fb_poly_time_stages(fb_poly_t h, int reps, double seconds[5]) {
  CHECK_POLY(h);
  if (!h->tetra || reps < 1 || !seconds) return fail(FB_EINVAL, "run sweep, classify and tetrahedralize once first");
  int (*const stage[4])(fb_poly_s*) = {do_sweep, do_classify, emit_vertices, emit_elements};
  const int pairs[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {0, 4}};  // each stage, and all four with the events between them
  return timed_stages<4>(h, reps, [&](int k) { return stage[k](h); }, pairs, seconds);
}

}  // extern "C"
