// Boundary triangles, positions and normals of the handle's tet mesh (surface.h), hand-written for gfx950.
//
// Build: a face is a 64-bit key (its three caller ids, ascending) and a 32-bit payload (element, local face, sign of the element's
// determinant).  The 4 n_tets pairs are generated in element order and sorted by a STABLE radix sort, so inside a run of equal keys
// the entries stand in the order SurfaceMesh::setupFromTetMesh (SurfaceMesh.cpp:155-193) meets them; insert / erase / insert on its
// std::set leaves a face exactly when the run is odd, with the vertex order of the run's last entry, and the set is read out in key
// order (:200-207) -- the order of the sorted array.  No float is added anywhere and the only atomics are integer ORs into a bitmap, so
// the arrays are the same from run to run.  The time is the sort's (4 n_tets pairs of 12 bytes, 3 x bits(n_nodes) key bits).
//
// Update: a thread per surface vertex walks the faces of its vertex in ascending face order (the incidence list is the 3 n_faces
// corners sorted stably by compact vertex), recomputes each unit normal in fp64 from x0 + q and rounds position and normal once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_prims.hip.h"
#include "launch.hip.h"
#include "mesh_device.hip.h"
#include "surface.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

// local faces of SurfaceMesh.cpp:180-190, 2 bits per corner, 6 bits per face: det >= 0 (1,2,3) (2,0,3) (3,0,1) (1,0,2), else
// (3,2,1) (3,0,2) (1,0,3) (2,0,1)
__device__ __forceinline__ void face_corners(bool neg, int f, int* c0, int* c1, int* c2) {
  const unsigned pos_t = (1u | 2u << 2 | 3u << 4) | (2u | 0u << 2 | 3u << 4) << 6 | (3u | 0u << 2 | 1u << 4) << 12 | (1u | 0u << 2 | 2u << 4) << 18;
  const unsigned neg_t = (3u | 2u << 2 | 1u << 4) | (3u | 0u << 2 | 2u << 4) << 6 | (1u | 0u << 2 | 3u << 4) << 12 | (2u | 0u << 2 | 1u << 4) << 18;
  const unsigned m = (neg ? neg_t : pos_t) >> (6 * f);
  *c0 = m & 3; *c1 = (m >> 2) & 3; *c2 = (m >> 4) & 3;
}

// the face of a payload: node ids in the handle's internal order in the payload's winding
__device__ __forceinline__ void payload_face(const int4* __restrict__ tets, uint32_t pay, int* n0, int* n1, int* n2) {
  const int4 t = tets[(pay & ~kFaceNeg) >> 2];
  int c0, c1, c2;
  face_corners((pay & kFaceNeg) != 0u, (int)(pay & 3u), &c0, &c1, &c2);
  *n0 = tet_node(t, c0); *n1 = tet_node(t, c1); *n2 = tet_node(t, c2);
}

// A thread per element: the sign of its determinant once (SurfaceMesh.cpp:165, vec3d::dot of vec3d::cross, no contraction), four keys
// and payloads.  shift > 0: key = a << 2 shift | b << shift | c.  shift == 0 (wide path): key = c only; k_face_keys_ab makes the second
// pass's keys from the payloads.
__global__ __launch_bounds__(kB) void k_face_keys(int n_tets, const int4* __restrict__ tets, const double* __restrict__ x0, const int* __restrict__ caller_of,
                                                  int shift, unsigned long long* __restrict__ keys, uint32_t* __restrict__ pay) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  const int4 t = tets[e];
  double v[4][3];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double* p = x0 + 3 * (size_t)tet_node(t, k);
    v[k][0] = p[0]; v[k][1] = p[1]; v[k][2] = p[2];
  }
  const double a[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
  const double b[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
  const double c[3] = {v[3][0] - v[0][0], v[3][1] - v[0][1], v[3][2] - v[0][2]};
  const double cr[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double det = a[0] * cr[0] + a[1] * cr[1] + a[2] * cr[2];
  const bool neg = !(det >= 0);
  unsigned id[4];
#pragma unroll
  for (int k = 0; k < 4; k++) id[k] = (unsigned)(caller_of ? caller_of[tet_node(t, k)] : tet_node(t, k));
  unsigned long long ko[4];
  uint32_t po[4];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    int c0, c1, c2;
    face_corners(neg, f, &c0, &c1, &c2);
    unsigned x = id[c0], y = id[c1], z = id[c2];
    sort3(x, y, z);
    ko[f] = shift ? ((unsigned long long)x << (2 * shift) | (unsigned long long)y << shift | z) : (unsigned long long)z;
    po[f] = (uint32_t)e << 2 | (uint32_t)f | (neg ? kFaceNeg : 0u);
  }
  ulonglong2* kd = reinterpret_cast<ulonglong2*>(keys + 4 * (size_t)e);  // 32 bytes per thread, contiguous over the wavefront
  kd[0] = make_ulonglong2(ko[0], ko[1]);
  kd[1] = make_ulonglong2(ko[2], ko[3]);
  *reinterpret_cast<uint4*>(pay + 4 * (size_t)e) = make_uint4(po[0], po[1], po[2], po[3]);
}

// wide path, between the passes: the entries stand sorted by their largest id; key = smallest << 32 | middle
__global__ __launch_bounds__(kB) void k_face_keys_ab(long long n, const int4* __restrict__ tets, const int* __restrict__ caller_of, const uint32_t* __restrict__ pay,
                                                     unsigned long long* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  int n0, n1, n2;
  payload_face(tets, pay[i], &n0, &n1, &n2);
  unsigned x = (unsigned)(caller_of ? caller_of[n0] : n0), y = (unsigned)(caller_of ? caller_of[n1] : n1), z = (unsigned)(caller_of ? caller_of[n2] : n2);
  sort3(x, y, z);
  keys[i] = (unsigned long long)x << 32 | y;
}

// ... and after them: the largest id of every sorted entry, the third word of the comparison in k_face_ends
__global__ __launch_bounds__(kB) void k_face_largest(long long n, const int4* __restrict__ tets, const int* __restrict__ caller_of, const uint32_t* __restrict__ pay,
                                                     uint32_t* __restrict__ csort) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  int n0, n1, n2;
  payload_face(tets, pay[i], &n0, &n1, &n2);
  unsigned x = (unsigned)(caller_of ? caller_of[n0] : n0), y = (unsigned)(caller_of ? caller_of[n1] : n1), z = (unsigned)(caller_of ? caller_of[n2] : n2);
  sort3(x, y, z);
  csort[i] = z;
}

// A thread per sorted entry: the last entry of a run of equal faces counts the run backwards and flags itself when it is odd.
// (Runs are 1 or 2 long on a valid mesh; a face shared by more elements is walked by one thread.)
__global__ __launch_bounds__(kB) void k_face_ends(long long n, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ csort,
                                                  unsigned char* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  const uint32_t c = csort ? csort[i] : 0u;
  unsigned char out = 0;
  if (i + 1 == n || keys[i + 1] != k || (csort && csort[i + 1] != c)) {
    long long cnt = 1;
    while (i - cnt >= 0 && keys[i - cnt] == k && (!csort || csort[i - cnt] == c)) cnt++;
    out = (unsigned char)(cnt & 1);
  }
  flag[i] = out;
}

// A thread per surviving face: its ids in both numberings, its element, a bit per node it uses.
__global__ __launch_bounds__(kB) void k_face_emit(int n_faces, const int4* __restrict__ tets, const int* __restrict__ caller_of, const uint32_t* __restrict__ sel,
                                                  int* __restrict__ faces, int* __restrict__ faces_int, int* __restrict__ face_tets, unsigned int* __restrict__ bitmap) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_faces) return;
  const uint32_t pay = sel[i];
  int n[3];
  payload_face(tets, pay, &n[0], &n[1], &n[2]);
  face_tets[i] = (int)((pay & ~kFaceNeg) >> 2);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int c = caller_of ? caller_of[n[k]] : n[k];
    faces_int[3 * (size_t)i + k] = n[k];
    faces[3 * (size_t)i + k] = c;
    // (integer OR: the result does not depend on the order.  A node lies in ~6 faces and a word holds 32 neighbours: most bits are set
    // already when a face arrives, and a plain load spares the atomic)
    const unsigned bit = 1u << (c & 31);
    if (!(bitmap[c >> 5] & bit)) atomicOr(&bitmap[c >> 5], bit);
  }
}

__global__ __launch_bounds__(kB) void k_word_counts(int n_words, const unsigned int* __restrict__ bitmap, int* __restrict__ cnt) {
  const int w = blockIdx.x * kB + threadIdx.x;
  if (w <= n_words) cnt[w] = w < n_words ? __popc(bitmap[w]) : 0;  // (one past the end: the scan leaves the total there)
}

// A thread per bitmap word: the caller ids of its bits, ascending, and the internal id of each
__global__ __launch_bounds__(kB) void k_vertex_ids(int n_words, const unsigned int* __restrict__ bitmap, const int* __restrict__ word_off,
                                                   const int* __restrict__ internal_of, int* __restrict__ vertex_ids, int* __restrict__ vnode, int* __restrict__ counts) {
  const int w = blockIdx.x * kB + threadIdx.x;
  if (w == 0) counts[1] = word_off[n_words];
  if (w >= n_words) return;
  unsigned int m = bitmap[w];
  int o = word_off[w];
  while (m) {
    const int id = (w << 5) + (__ffs((int)m) - 1);
    m &= m - 1;
    vertex_ids[o] = id;
    vnode[o] = internal_of ? internal_of[id] : id;
    o++;
  }
}

// A thread per face corner: its compact vertex (the rank of its bit in the bitmap) as sort key, 3 * face + corner as value
__global__ __launch_bounds__(kB) void k_corner_keys(int n_corners, const int* __restrict__ faces, const unsigned int* __restrict__ bitmap,
                                                    const int* __restrict__ word_off, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_corners) return;
  const int c = faces[j];
  keys[j] = (uint32_t)(word_off[c >> 5] + __popc(bitmap[c >> 5] & ((1u << (c & 31)) - 1u)));
  vals[j] = (uint32_t)j;
}

// first entry of every vertex in the sorted corner list (every surface vertex has one: no scan is needed)
__global__ __launch_bounds__(kB) void k_corner_heads(int n_corners, const uint32_t* __restrict__ keys_s, const int* __restrict__ counts, int* __restrict__ inc_off) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_corners) return;
  if (j == 0 || keys_s[j] != keys_s[j - 1]) inc_off[keys_s[j]] = j;
  if (j == 0) inc_off[counts[1]] = n_corners;
}

// A thread per surface vertex.  NORMALS = false: positions and box only (the rest box of fb_fem_surface, q == nullptr).
// The box goes to a per-workgroup partial; k_box_final folds the partials (workgroup.hip.h).
template <bool NORMALS>
__global__ __launch_bounds__(kB) void k_surface_update(int n_max, const int* __restrict__ n_dev, const int* __restrict__ vnode, const int* __restrict__ inc_off, const uint32_t* __restrict__ inc,
                                                       const int* __restrict__ faces_int, const double* __restrict__ x0, const double* __restrict__ q,
                                                       float* __restrict__ xyz, float* __restrict__ normals, float* __restrict__ part) {
  const int v = blockIdx.x * kB + threadIdx.x;
  const int n_vertices = n_dev ? min(*n_dev, n_max) : n_max;  // (the build's rest box runs before the host knows the count)
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (v < n_vertices) {
    const size_t i = 3 * (size_t)vnode[v];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float p = (float)(q ? x0[i + k] + q[i + k] : x0[i + k]);
      lo[k] = hi[k] = p;
      xyz[3 * (size_t)v + k] = p;
    }
    if (NORMALS) {
      double sum[3] = {0.0, 0.0, 0.0};
      for (int j = inc_off[v]; j < inc_off[v + 1]; j++) {
        const int* f = faces_int + 3 * (size_t)(inc[j] / 3u);
        double p[3][3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const size_t b = 3 * (size_t)f[c];
#pragma unroll
          for (int k = 0; k < 3; k++) p[c][k] = x0[b + k] + q[b + k];
        }
        const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (len > 0.0) { sum[0] += n[0] / len; sum[1] += n[1] / len; sum[2] += n[2] / len; }  // (a face without area has no normal)
      }
      const double len = sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
#pragma unroll
      for (int k = 0; k < 3; k++) normals[3 * (size_t)v + k] = len > 0.0 ? (float)(sum[k] / len) : 0.0f;
    }
  }
  wg_box(lo, hi, part + 6 * (size_t)blockIdx.x);
}

}  // namespace

int surface_build(hipStream_t s, SurfaceWork& S, int n_nodes, int n_tets, const int4* tets, const double* x0, const int* caller_of, const int* internal_of,
                  bool force_wide, PlanWorkspace& W) {
  S.valid = false;
  const size_t ne = (size_t)4 * n_tets;
  const int nb = bits_of(n_nodes);
  const bool wide = force_wide || 3 * nb > 63;
  S.wide = wide;
  // the sort's arrays are the plan builder's (it is not running: every build is an entry point of its own on the handle's stream)
  FB_TRY(W.keys.reserve(ne)); FB_TRY(W.keys_s.reserve(ne)); FB_TRY(W.vals.reserve(ne)); FB_TRY(W.vals_s.reserve(ne));
  FB_TRY(S.flag.alloc(ne));
  FB_TRY(S.counts.alloc(2));
  FB_TRY(launch_1d(k_face_keys, n_tets, s, n_tets, tets, x0, caller_of, wide ? 0 : nb, W.keys.p, W.vals.p));
  const unsigned long long* keys_sorted = W.keys_s.p;
  const uint32_t* pay_sorted = W.vals_s.p;
  if (!wide) {
    FB_TRY(sort_pairs(W.temp, s, W.keys.p, W.keys_s.p, W.vals.p, W.vals_s.p, ne, (unsigned)(3 * nb)));
  } else {
    // two stable passes: by the largest id, then by smallest << 32 | middle
    FB_TRY(sort_pairs(W.temp, s, W.keys.p, W.keys_s.p, W.vals.p, W.vals_s.p, ne, (unsigned)nb));
    FB_TRY(launch_1d(k_face_keys_ab, (long long)ne, s, ne, tets, caller_of, W.vals_s.p, W.keys_s.p));
    FB_TRY(sort_pairs(W.temp, s, W.keys_s.p, W.keys.p, W.vals_s.p, W.vals.p, ne, (unsigned)(32 + nb)));
    keys_sorted = W.keys.p;
    pay_sorted = W.vals.p;
    FB_TRY(S.csort.alloc(ne));
    FB_TRY(launch_1d(k_face_largest, (long long)ne, s, ne, tets, caller_of, pay_sorted, S.csort.p));
  }
  FB_TRY(launch_1d(k_face_ends, (long long)ne, s, ne, keys_sorted, wide ? S.csort.p : nullptr, S.flag.p));
  FB_TRY(S.sel.alloc(ne));  // (a mesh of separate elements keeps every face)
  FB_TRY(select_flagged(W.temp, s, pay_sorted, S.flag.p, S.sel.p, S.counts.p, ne));
  int nf = 0;
  FB_HIP(hipMemcpyAsync(&nf, S.counts.p, sizeof(int), hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));  // the first host wait
  if (nf < 0 || (size_t)nf > ne) return fail(FB_EDEVICE, "surface build: face count %d out of range", nf);
  S.n_faces = nf;
  S.n_nodes = n_nodes;
  S.n_vertices = 0;
  const int n_words = (n_nodes + 31) / 32;
  const int nc = 3 * nf;
  const int nv_max = std::min(nc, n_nodes);
  FB_TRY(S.faces.alloc((size_t)std::max(nc, 1))); FB_TRY(S.faces_int.alloc((size_t)std::max(nc, 1))); FB_TRY(S.face_tets.alloc((size_t)std::max(nf, 1)));
  FB_TRY(S.bitmap.alloc((size_t)n_words)); FB_TRY(S.word_cnt.alloc((size_t)n_words + 1)); FB_TRY(S.word_off.alloc((size_t)n_words + 1));
  FB_TRY(S.vertex_ids.alloc((size_t)std::max(nv_max, 1))); FB_TRY(S.vnode.alloc((size_t)std::max(nv_max, 1)));
  FB_TRY(S.inc.alloc((size_t)std::max(nc, 1))); FB_TRY(S.inc_off.alloc((size_t)nv_max + 1));
  FB_TRY(S.out.alloc((size_t)6 * nv_max + 6));  // (the rest box of this build sits in the last six)
  FB_TRY(S.part.alloc((size_t)6 * blocks_for(nv_max)));
  FB_TRY(S.bitmap.zero(s));
  if (nf) FB_TRY(launch_1d(k_face_emit, nf, s, nf, tets, caller_of, S.sel.p, S.faces.p, S.faces_int.p, S.face_tets.p, S.bitmap.p));
  FB_TRY(launch_1d(k_word_counts, n_words + 1, s, n_words, S.bitmap.p, S.word_cnt.p));
  FB_TRY(exclusive_scan(W.temp, s, S.word_cnt.p, S.word_off.p, 0, (size_t)n_words + 1));
  FB_TRY(launch_1d(k_vertex_ids, n_words, s, n_words, S.bitmap.p, S.word_off.p, internal_of, S.vertex_ids.p, S.vnode.p, S.counts.p));
  if (nf) {
    // incidence: the corners sorted stably by compact vertex keep their ascending face order
    // (the face sort's arrays are free again: the surviving payloads are in S.sel)
    FB_TRY(W.keys.reserve(((size_t)nc + 1) / 2)); FB_TRY(W.keys_s.reserve(((size_t)nc + 1) / 2)); FB_TRY(W.vals.reserve((size_t)nc));
    uint32_t* ck = reinterpret_cast<uint32_t*>(W.keys.p);
    uint32_t* ck_s = reinterpret_cast<uint32_t*>(W.keys_s.p);
    uint32_t* cv = W.vals.p;
    FB_TRY(launch_1d(k_corner_keys, nc, s, nc, S.faces.p, S.bitmap.p, S.word_off.p, ck, cv));
    FB_TRY(sort_pairs(W.temp, s, ck, ck_s, cv, S.inc.p, (size_t)nc, (unsigned)bits_of(nv_max)));
    FB_TRY(launch_1d(k_corner_heads, nc, s, nc, ck_s, S.counts.p, S.inc_off.p));
  }
  // the rest box: the grid covers the most vertices there can be and the kernel reads the count on the device, so the count and the box
  // leave together in the second (and last) host wait
  float* rest_box_dev = S.out.p + 6 * (size_t)nv_max;
  FB_TRY(launch_1d(k_surface_update<false>, nv_max, s, nv_max, S.counts.p + 1, S.vnode.p, S.inc_off.p, S.inc.p, S.faces_int.p, x0, nullptr, S.out.p, S.out.p, S.part.p));
  FB_TRY(launch_grid(k_box_final<float>, dim3(1), s, blocks_for(nv_max), S.part.p, rest_box_dev));
  int nv = 0;
  FB_HIP(hipMemcpyAsync(&nv, S.counts.p + 1, sizeof(int), hipMemcpyDeviceToHost, s));
  FB_HIP(hipMemcpyAsync(S.rest_box, rest_box_dev, 6 * sizeof(float), hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  if (nv < 0 || nv > nv_max) return fail(FB_EDEVICE, "surface build: vertex count %d out of range", nv);
  if (!nv)
    for (int k = 0; k < 6; k++) S.rest_box[k] = 0.0f;
  S.n_vertices = nv;
  S.valid = true;
  S.n_builds++;
  return FB_OK;
}

int surface_update(hipStream_t s, SurfaceWork& S, const double* x0, const double* q, bool copy_out) {
  const int nv = S.n_vertices;
  if (!nv) return FB_OK;
  float* xyz = S.out.p;
  float* nrm = S.out.p + 3 * (size_t)nv;
  float* box = S.out.p + 6 * (size_t)nv;
  FB_TRY(launch_1d(k_surface_update<true>, nv, s, nv, nullptr, S.vnode.p, S.inc_off.p, S.inc.p, S.faces_int.p, x0, q, xyz, nrm, S.part.p));
  FB_TRY(launch_grid(k_box_final<float>, dim3(1), s, blocks_for(nv), S.part.p, box));
  if (copy_out) {
    S.host.resize((size_t)6 * nv + 6);
    FB_HIP(hipMemcpyAsync(S.host.data(), S.out.p, sizeof(float) * S.host.size(), hipMemcpyDeviceToHost, s));  // 24 n_vertices + 24 bytes
    FB_HIP(hipStreamSynchronize(s));
  }
  return FB_OK;
}

}  // namespace fb
