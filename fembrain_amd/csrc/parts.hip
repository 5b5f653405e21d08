// Disjoint parts of the handle's tet mesh (parts.h), hand-written for gfx950.
//
// Labels: a face is a 64-bit key (its three node ids in the handle's internal order, ascending -- equality is all that counts, and the
// renumbering is a bijection) and a 32-bit payload (element, local face).  The 4 n_tets pairs are sorted by one stable radix sort (two
// passes above 2^21 nodes), and every run of equal keys links its consecutive entries: two elements are adjacent exactly when they share
// a face, and a face that three or more elements carry connects all of them.
//
// The links go through a lock-free union-find in ONE launch (k_parts_hook).  A root is an element that is its own parent; hooking
// always puts the root with the LARGER id under the smaller one by a compare-and-swap on the larger root's own word.  The invariant:
// parent[e] is always an ancestor of e (or e itself) and <= e.  So every walk descends and ends, and the root of a finished tree is its
// smallest element whatever order the workgroups ran
// in.  Nothing waits for another workgroup: every loop ends through its own progress (a failed swap means somebody else hooked that
// root, of which there are fewer than n_tets, and the walk goes on from the value the swap returned).
// Coherence: an XCD's L2 is private and a CU's L1 is never refreshed by other CUs' stores, so inside the hooking launch the parent array
// is touched through agent-scope atomics only (relaxed loads and stores, atomicCAS).  The words of non-roots are not monotone: two racing
// shortening stores of uf_find may leave the older, higher grandparent in place of a newer, deeper one.  That keeps the invariant -- an
// ancestor stays an ancestor for good, since trees only ever join at roots -- and for the same reason even a stale word would only make a
// walk longer or a swap on a former root fail; no wrong tree can form.  A root's own word changes once, through the compare-and-swap.  The flatten runs in a launch of its own, behind the kernel boundary that makes every parent final.
//
// Ahead of the hooking a seed forest (k_parts_seed: every element under its smallest face neighbour) is flattened behind kernel boundaries;
// pairs inside one seed tree are skipped on plain loads of an array the hooking launch does not write, which keeps most walks off the
// parts' root words (speed only: the hooking decides every other pair, and the result does not depend on the seed).
//
// Part k is the k-th root in ascending element order (VolMesh::get_disjoint_parts starts every part at *setCells.begin()): a flag per
// root, an exclusive scan, element_part[e] = rank[root[e]].  The per-part figures come from the elements sorted stably by part: counts
// from the run heads, volumes from fixed chunks of 1024 sorted elements summed in a fixed tree and a fixed-order sum of a part's chunks --
// fp64, no float atomics, the same bits from call to call.  Node labels are atomicMin of the part index, "shared" an integer OR.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/fembrain_hip_testing.h"
#include "device_prims.hip.h"
#include "fem_handle.h"
#include "launch.hip.h"
#include "mesh_device.hip.h"
#include "parts.h"
#include "workgroup.hip.h"

namespace fb {
namespace {

constexpr int kNone = 0x7f7f7f7f;  // a node nobody uses (what a byte fill of 0x7f leaves; above every part index and corner key)
constexpr int kChunk = 1024;       // sorted elements per volume chunk: 4 per thread of a workgroup

// local face f of an element: its three nodes other than corner f, ascending
__device__ __forceinline__ void face_ids(const int4& t, int f, unsigned* x, unsigned* y, unsigned* z) {
  unsigned a = (unsigned)tet_node(t, f == 0 ? 1 : 0), b = (unsigned)tet_node(t, f <= 1 ? 2 : 1), c = (unsigned)tet_node(t, f <= 2 ? 3 : 2);
  sort3(a, b, c);
  *x = a; *y = b; *z = c;
}

// A thread per element: four keys and payloads (element << 2 | face), and the element as its own parent.
// shift > 0: key = a << 2 shift | b << shift | c.  shift == 0 (wide path): key = c only; k_parts_keys_ab makes the second pass's keys.
__global__ __launch_bounds__(kB) void k_parts_face_keys(int n_tets, const int4* __restrict__ tets, int shift, unsigned long long* __restrict__ keys, uint32_t* __restrict__ pay,
                                                        int* __restrict__ parent) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  const int4 t = tets[e];
  unsigned long long ko[4];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    unsigned x, y, z;
    face_ids(t, f, &x, &y, &z);
    ko[f] = shift ? ((unsigned long long)x << (2 * shift) | (unsigned long long)y << shift | z) : (unsigned long long)z;
  }
  ulonglong2* kd = reinterpret_cast<ulonglong2*>(keys + 4 * (size_t)e);
  kd[0] = make_ulonglong2(ko[0], ko[1]);
  kd[1] = make_ulonglong2(ko[2], ko[3]);
  const uint32_t p = (uint32_t)e << 2;
  *reinterpret_cast<uint4*>(pay + 4 * (size_t)e) = make_uint4(p, p | 1u, p | 2u, p | 3u);
  parent[e] = e;
}

// wide path, between the passes: the entries stand sorted by their largest id; key = smallest << 32 | middle
__global__ __launch_bounds__(kB) void k_parts_keys_ab(long long n, const int4* __restrict__ tets, const uint32_t* __restrict__ pay, unsigned long long* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  unsigned x, y, z;
  face_ids(tets[pay[i] >> 2], (int)(pay[i] & 3u), &x, &y, &z);
  keys[i] = (unsigned long long)x << 32 | y;
}

// ---- the union-find of the hooking launch: every access of `parent` is an agent-scope atomic ----

__device__ __forceinline__ int uf_load(int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// walks to the root; a non-root on the way is pointed at a grandparent it read (an ancestor stays an ancestor; racing stores may put an
// older one back, which is as valid; a root's own word is never written here: only the swap of uf_union changes it)
__device__ __forceinline__ int uf_find(int* parent, int x) {
  int p = uf_load(parent, x);
  while (p != x) {
    const int g = uf_load(parent, p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
  a = uf_load(parent, a);
  b = uf_load(parent, b);
  if (a == b) return;  // (one parent: one tree, and the root's word, which every walk of the part ends in, is left alone)
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;  // hi was hooked meanwhile: on from where it points
    b = lo;
  }
}

// entries i and i + 1 of the sorted list hold one face: their two elements
__device__ __forceinline__ bool linked_pair(long long i, long long n, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ pay, const int4* __restrict__ tets,
                                            int wide, int* a, int* b) {
  if (i + 1 >= n) return false;
  if (keys[i] != keys[i + 1]) return false;
  const uint32_t pa = pay[i], pb = pay[i + 1];
  if (wide) {  // (the key holds the smallest and the middle id: the largest decides)
    unsigned x, y, za, zb;
    face_ids(tets[pa >> 2], (int)(pa & 3u), &x, &y, &za);
    face_ids(tets[pb >> 2], (int)(pb & 3u), &x, &y, &zb);
    if (za != zb) return false;
  }
  *a = (int)(pa >> 2); *b = (int)(pb >> 2);
  return true;
}

// Ahead of the hooking, two launches of their own that make its walks short.  k_parts_seed: a thread per sorted entry puts the smaller
// element of a linked pair into the larger one's word with an integer atomicMin (no load depends on another workgroup), so every element
// points at its smallest face neighbour below it, or at itself: a forest that obeys the invariant.  k_parts_seed_roots: behind the kernel
// boundary, plain loads walk that forest and every element gets the root it reaches, in a second array, which is the forest the hooking
// starts from, and in a copy that nobody writes again.  Two elements with one seed root are in one tree from the start, so the hooking
// skips their pair on two plain loads of that copy; on a mesh numbered cell by cell that is nearly every pair.  (It matters: every walk
// ends in a load of its root's own word, and a part has ONE root -- without the skip two million walks queue on a handful of words; the
// kernel trace showed 1.2 ms of hooking at 1M tets, 1.9 ms when all walks were short but still ended there.)  Pairs across seed trees go
// through the union as before, so the result does not rest on the seed.
__global__ __launch_bounds__(kB) void k_parts_seed(long long n, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ pay, const int4* __restrict__ tets,
                                                   int wide, int* parent) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  int a, b;
  if (!linked_pair(i, n, keys, pay, tets, wide, &a, &b) || a == b) return;
  atomicMin(parent + (a > b ? a : b), a > b ? b : a);
}
// (between the two, four rounds of out[e] = in[in[e]] from one array into another: a chain towards the smallest neighbour is hundreds of
// elements long on a 56^3 cube, and sixteen times fewer dependent loads are left for the walk)
__global__ __launch_bounds__(kB) void k_parts_seed_jump(int n_tets, const int* __restrict__ in, int* __restrict__ out) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e < n_tets) out[e] = in[in[e]];
}
__global__ __launch_bounds__(kB) void k_parts_seed_roots(int n_tets, const int* __restrict__ seed, int* __restrict__ parent, int* __restrict__ seed_root) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  int x = e, p = seed[x];
  while (p != x) { x = p; p = seed[x]; }
  parent[e] = x;
  seed_root[e] = x;
}

// A thread per sorted entry but the last: entries i and i + 1 of one face link their elements.
__global__ __launch_bounds__(kB) void k_parts_hook(long long n, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ pay, const int4* __restrict__ tets,
                                                   int wide, const int* __restrict__ seed_root, int* parent) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  int a, b;
  if (!linked_pair(i, n, keys, pay, tets, wide, &a, &b)) return;
  if (seed_root[a] == seed_root[b]) return;  // (one tree since before this launch; seed_root is not written in it)
  uf_union(parent, a, b);
}

// ... and in a launch of its own, where every parent is final: every element to its root, a flag per root
__global__ __launch_bounds__(kB) void k_parts_flatten(int n_tets, const int* __restrict__ parent, int* __restrict__ root, int* __restrict__ flag) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e == 0) flag[n_tets] = 0;  // (one past the end: the scan leaves the number of parts there)
  if (e >= n_tets) return;
  int x = e, p = parent[x];
  while (p != x) { x = p; p = parent[x]; }
  root[e] = x;
  flag[e] = x == e;
}

__global__ __launch_bounds__(kB) void k_parts_label(int n_tets, const int* __restrict__ root, const int* __restrict__ flag, const int* __restrict__ rank,
                                                    int* __restrict__ element_part, int* __restrict__ part_first) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  const int p = rank[root[e]];
  element_part[e] = p;
  if (flag[e]) part_first[p] = e;
}

// first entry of every part in the list sorted by part (every part has an element: no scan is needed)
__global__ __launch_bounds__(kB) void k_parts_heads(int n_tets, const uint32_t* __restrict__ keys_s, int n_parts, int* __restrict__ part_off) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_tets) return;
  if (j == 0 || keys_s[j] != keys_s[j - 1]) part_off[keys_s[j]] = j;
  if (j == 0) part_off[n_parts] = n_tets;
}

// A thread per part: its volume chunks, and the largest part (most elements, lowest index of equals) as one integer maximum
__global__ __launch_bounds__(kB) void k_parts_chunks(int n_parts, const int* __restrict__ part_off, int* __restrict__ chunk_cnt, unsigned long long* __restrict__ best) {
  const int k = blockIdx.x * kB + threadIdx.x;
  if (k > n_parts) return;
  if (k == n_parts) { chunk_cnt[k] = 0; return; }
  const int cnt = part_off[k + 1] - part_off[k];
  chunk_cnt[k] = (cnt + kChunk - 1) / kChunk;
  atomicMax(best, (unsigned long long)cnt << 32 | (0xffffffffu - (unsigned)k));
}

// fb_fem_volume's expression on the rest positions
__device__ __forceinline__ double rest_volume(const int4& t, const double* __restrict__ x0) {
  double p[4][3];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double* s = x0 + 3 * (size_t)tet_node(t, k);
    p[k][0] = s[0]; p[k][1] = s[1]; p[k][2] = s[2];
  }
  return tet_volume(p);
}

// A workgroup per chunk (the grid covers the most chunks there can be): thread t adds the chunk's sorted elements t, t + 256, ... in
// that order, then the tree.  The chunk's part: the last k with chunk_off[k] <= chunk.
__global__ __launch_bounds__(kB) void k_parts_chunk_volumes(int n_parts, const int* __restrict__ chunk_off, const int* __restrict__ part_off, const uint32_t* __restrict__ sorted,
                                                            const int4* __restrict__ tets, const double* __restrict__ x0, double* __restrict__ chunk_vol) {
  const int c = blockIdx.x;
  if (c >= chunk_off[n_parts]) return;  // (the whole workgroup)
  int lo = 0, hi = n_parts - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_off[mid] <= c) lo = mid; else hi = mid - 1;
  }
  const int j0 = part_off[lo] + (c - chunk_off[lo]) * kChunk, j1 = min(j0 + kChunk, part_off[lo + 1]);
  double v = 0.0;
  for (int j = j0 + (int)threadIdx.x; j < j1; j += kB) v += rest_volume(tets[sorted[j]], x0);
  const double s = wg_sum(v);
  if (threadIdx.x == 0) chunk_vol[c] = s;
}

// A wavefront per part: lane l adds the part's chunks l, l + 64, ... in that order, then the shuffles
__global__ __launch_bounds__(kB) void k_parts_volumes(int n_parts, const int* __restrict__ chunk_off, const double* __restrict__ chunk_vol, double* __restrict__ part_volume) {
  const int k = blockIdx.x * (kB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= n_parts) return;
  double v = 0.0;
  for (int c = chunk_off[k] + lane; c < chunk_off[k + 1]; c += 64) v += chunk_vol[c];
  v = wf_sum(v);
  if (lane == 0) part_volume[k] = v;
}

// arr[key] += 1 for every lane with `on`: one integer add for the wavefront where its lanes agree on the key (neighbours mostly lie in one
// part, and a million adds to a handful of words would queue up), one per lane otherwise.  Called by every lane of the wavefront.
__device__ __forceinline__ void wave_count(int* arr, int key, bool on) {
  const unsigned long long m = __ballot(on);
  if (!m) return;
  const int src = __ffsll((long long)m) - 1;
  const int k0 = __shfl(key, src);
  if (__all(!on || key == k0)) {
    if ((int)(threadIdx.x & 63) == src) atomicAdd(arr + k0, __popcll(m));
  } else if (on) {
    atomicAdd(arr + key, 1);
  }
}
// ... the same for a whole workgroup of kB threads where its wavefronts agree (a thread per node: thousands of wavefronts would otherwise
// queue on the words of a few parts).  Called by every thread of the workgroup.
__device__ __forceinline__ void block_count(int* arr, int key, bool on) {
  __shared__ int sh_key[kB / 64], sh_cnt[kB / 64];
  const unsigned long long m = __ballot(on);
  const int src = m ? __ffsll((long long)m) - 1 : 0;
  const int k0 = __shfl(key, src);
  const bool agree = m != 0 && __all(!on || key == k0);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh_key[wave] = agree ? k0 : -1; sh_cnt[wave] = agree ? __popcll(m) : 0; }
  if (m != 0 && !agree && on) atomicAdd(arr + key, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < kB / 64; w++) {
      if (sh_key[w] < 0) continue;
      int c = sh_cnt[w];
      for (int v = w + 1; v < kB / 64; v++)
        if (sh_key[v] == sh_key[w]) { c += sh_cnt[v]; sh_key[v] = -1; }
      atomicAdd(arr + sh_key[w], c);
    }
  }
}
__device__ __forceinline__ void wave_total(int* word, bool on) {
  const unsigned long long m = __ballot(on);
  if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(word, __popcll(m));
}

// A thread per element: the lowest part of each of its nodes
__global__ __launch_bounds__(kB) void k_parts_node_min(int n_tets, const int4* __restrict__ tets, const int* __restrict__ element_part, int* __restrict__ node_part) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  const int4 t = tets[e];
  const int p = element_part[e];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int* w = node_part + tet_node(t, k);
    if (*w > p) atomicMin(w, p);  // (a stale word is only larger: the atomic decides)
  }
}

// ... and behind it: a corner whose node carries another part's label is foreign, its node shared
__global__ __launch_bounds__(kB) void k_parts_node_shared(int n_tets, const int4* __restrict__ tets, const int* __restrict__ element_part, const int* __restrict__ node_part,
                                                          int* __restrict__ node_flag, unsigned char* __restrict__ foreign) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  const int4 t = tets[e];
  const int p = element_part[e];
  unsigned f4 = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int n = tet_node(t, k);
    if (node_part[n] != p) {
      f4 |= 1u << (8 * k);
      atomicOr(node_flag + n, 1);
    }
  }
  *reinterpret_cast<unsigned*>(foreign + 4 * (size_t)e) = f4;
}

// A thread per node (internal order): its label in the caller's order, a node for its lowest part, the two counts
__global__ __launch_bounds__(kB) void k_parts_node_out(int n_nodes, const int* __restrict__ node_part, const int* __restrict__ node_flag, const int* __restrict__ caller_of,
                                                       int* __restrict__ node_part_out, int* __restrict__ part_nodes, int* __restrict__ counts) {
  const int n = blockIdx.x * kB + threadIdx.x;
  const bool in = n < n_nodes;
  const int lab = in ? node_part[n] : kNone;
  const bool used = lab < kNone;
  if (in) node_part_out[caller_of ? caller_of[n] : n] = used ? lab : -1;
  block_count(part_nodes, lab, used);
  wave_total(counts + 1, in && node_flag[n] != 0);
  wave_total(counts + 2, in && !used);
}

// shared nodes count in each of their parts: part << 32 | node of every corner (the foreign ones are selected, sorted and counted once each)
__global__ __launch_bounds__(kB) void k_parts_corner_keys(int n_tets, const int4* __restrict__ tets, const int* __restrict__ element_part, unsigned long long* __restrict__ keys) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  const int4 t = tets[e];
  const unsigned long long p = (unsigned long long)element_part[e] << 32;
#pragma unroll
  for (int k = 0; k < 4; k++) keys[4 * (size_t)e + k] = p | (unsigned)tet_node(t, k);
}
__global__ __launch_bounds__(kB) void k_parts_foreign_count(int n, const unsigned long long* __restrict__ keys_s, int* __restrict__ part_nodes) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n) return;
  if (j == 0 || keys_s[j] != keys_s[j - 1]) atomicAdd(part_nodes + (int)(keys_s[j] >> 32), 1);
}

// ---- the split ----
struct Vec3 { double v[3]; };

// A thread per element: in front when dot(centroid(x0 + q) - c, n) > 0 (CuttableMesh.cpp:584-588), counted per part
__global__ __launch_bounds__(kB) void k_split_front(int n_tets, const int4* __restrict__ tets, const double* __restrict__ x0, const double* __restrict__ q, Vec3 c, Vec3 nrm,
                                                    const int* __restrict__ element_part, int* __restrict__ part_front) {
  const int e = blockIdx.x * kB + threadIdx.x;
  bool front = false;
  int p = 0;
  if (e < n_tets) {
    const int4 t = tets[e];
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const size_t b = 3 * (size_t)tet_node(t, k);
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double pos = x0[b + a] + q[b + a];
        s[a] = k == 0 ? pos : s[a] + pos;
      }
    }
    const double d[3] = {s[0] * 0.25 - c.v[0], s[1] * 0.25 - c.v[1], s[2] * 0.25 - c.v[2]};
    front = d[0] * nrm.v[0] + d[1] * nrm.v[1] + d[2] * nrm.v[2] > 0.0;
    p = element_part[e];
  }
  wave_count(part_front, p, front);
}

// A thread per part: 1 front (every element in front), 2 back (none), 0 straddling
__global__ __launch_bounds__(kB) void k_split_classify(int n_parts, const int* __restrict__ part_front, const int* __restrict__ part_off, int* __restrict__ part_class,
                                                       int* __restrict__ counts) {
  const int k = blockIdx.x * kB + threadIdx.x;
  int cls = -1;
  if (k < n_parts) {
    const int f = part_front[k];
    cls = f == part_off[k + 1] - part_off[k] ? 1 : f == 0 ? 2 : 0;
    part_class[k] = cls;
  }
  wave_total(counts + 4, cls == 1);
  wave_total(counts + 5, cls == 2);
  wave_total(counts + 6, cls == 0);
}

// A thread per element of a front or back part: its side's bit into each of its nodes (the reference's two std::sets)
__global__ __launch_bounds__(kB) void k_split_nodes(int n_tets, const int4* __restrict__ tets, const int* __restrict__ element_part, const int* __restrict__ part_class,
                                                    int* __restrict__ node_flag) {
  const int e = blockIdx.x * kB + threadIdx.x;
  if (e >= n_tets) return;
  const int cls = part_class[element_part[e]];
  if (!cls) return;
  const int4 t = tets[e];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int* w = node_flag + tet_node(t, k);
    if (!(*w & cls)) atomicOr(w, cls);  // (a stale word only lacks bits: the atomic decides)
  }
}

// A thread per node: + shift for a front node, - shift for a back node, both for a node of both (it stays)
__global__ __launch_bounds__(kB) void k_split_move(int n_nodes, const int* __restrict__ node_flag, double* __restrict__ x0, Vec3 shift, int apply, int* __restrict__ counts) {
  const int n = blockIdx.x * kB + threadIdx.x;
  bool moved = false;
  if (n < n_nodes) {
    const int m = node_flag[n];
    if (m == 1 || m == 2) {
      double* p = x0 + 3 * (size_t)n;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double was = p[a], now = m == 1 ? was + shift.v[a] : was - shift.v[a];
        moved = moved || now != was;
        if (apply) p[a] = now;
      }
    }
  }
  wave_total(counts + 7, moved);
}

// ---- a part as a mesh ----

// A thread per element of the part (rank j in ascending order): 4 j + corner as the key of each of its nodes
__global__ __launch_bounds__(kB) void k_part_node_keys(int n_el, const uint32_t* __restrict__ ids, const int4* __restrict__ tets, int* __restrict__ node_key) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_el) return;
  const int4 t = tets[ids[j]];
#pragma unroll
  for (int k = 0; k < 4; k++) atomicMin(node_key + tet_node(t, k), 4 * j + k);
}
// ... behind it, a thread per corner: the corner that holds its node's key is the node's first use (the order mapNodes assigns)
__global__ __launch_bounds__(kB) void k_part_first_use(int n_corners, const uint32_t* __restrict__ ids, const int4* __restrict__ tets, const int* __restrict__ node_key,
                                                       int* __restrict__ cflag) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i > n_corners) return;
  cflag[i] = i < n_corners ? node_key[tet_node(tets[ids[i >> 2]], i & 3)] == i : 0;
}
__global__ __launch_bounds__(kB) void k_part_emit_nodes(int n_corners, const uint32_t* __restrict__ ids, const int4* __restrict__ tets, const int* __restrict__ cflag,
                                                        const int* __restrict__ cpos, const int* __restrict__ caller_of, const double* __restrict__ x0,
                                                        int* __restrict__ node_local, int* __restrict__ out_nodes, double* __restrict__ out_xyz) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_corners || !cflag[i]) return;
  const int n = tet_node(tets[ids[i >> 2]], i & 3), pos = cpos[i];
  node_local[n] = pos;
  out_nodes[pos] = caller_of ? caller_of[n] : n;
#pragma unroll
  for (int a = 0; a < 3; a++) out_xyz[3 * (size_t)pos + a] = x0[3 * (size_t)n + a];
}
__global__ __launch_bounds__(kB) void k_part_emit_tets(int n_corners, const uint32_t* __restrict__ ids, const int4* __restrict__ tets, const int* __restrict__ node_local,
                                                       int* __restrict__ out_tets) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_corners) return;
  out_tets[i] = node_local[tet_node(tets[ids[i >> 2]], i & 3)];
}

int fill_bytes(hipStream_t s, void* p, int byte, size_t bytes) {
  if (bytes) FB_HIP(hipMemsetAsync(p, byte, bytes, s));
  return FB_OK;
}

}  // namespace

int parts_volumes(hipStream_t s, PartsWork& P, const PartsMesh& M) {
  const int n_chunk_max = M.n_tets / kChunk + P.n_parts;  // (a part has at most one chunk that is not full)
  FB_TRY(P.chunk_vol.reserve((size_t)n_chunk_max));
  FB_TRY(launch_grid(k_parts_chunk_volumes, dim3((unsigned)n_chunk_max), s, P.n_parts, P.chunk_off.p, P.part_off.p, P.sorted.p, M.tets, M.x0, P.chunk_vol.p));
  return launch_waves(k_parts_volumes, P.n_parts, s, P.n_parts, P.chunk_off.p, P.chunk_vol.p, P.part_volume.p);
}

int parts_build(hipStream_t s, PartsWork& P, const PartsMesh& M, bool force_wide, PlanWorkspace& W) {
  P.valid = false;
  const int nt = M.n_tets, nn = M.n_nodes;
  const size_t ne = (size_t)4 * nt;
  const int nb = bits_of(nn);
  const bool wide = force_wide || 3 * nb > 63;
  P.wide = wide;
  // the sort's arrays are the plan builder's (it is not running: every build is an entry point of its own on the handle's stream)
  FB_TRY(W.keys.reserve(ne)); FB_TRY(W.keys_s.reserve(ne)); FB_TRY(W.vals.reserve(ne)); FB_TRY(W.vals_s.reserve(ne));
  FB_TRY(P.parent.alloc((size_t)nt)); FB_TRY(P.root.alloc((size_t)nt)); FB_TRY(P.flag.alloc((size_t)nt + 1)); FB_TRY(P.rank.alloc((size_t)nt + 1));
  FB_TRY(P.element_part.alloc((size_t)nt)); FB_TRY(P.sorted.alloc((size_t)nt)); FB_TRY(P.foreign.alloc(ne));
  FB_TRY(P.node_part.alloc((size_t)nn)); FB_TRY(P.node_part_out.alloc((size_t)nn)); FB_TRY(P.node_flag.alloc((size_t)nn));
  FB_TRY(P.counts.alloc(8)); FB_TRY(P.best.alloc(1));
  // ---- the face list and the links ----
  FB_TRY(launch_1d(k_parts_face_keys, nt, s, nt, M.tets, wide ? 0 : nb, W.keys.p, W.vals.p, P.root.p));
  const unsigned long long* keys_sorted = W.keys_s.p;
  const uint32_t* pay_sorted = W.vals_s.p;
  if (!wide) {
    FB_TRY(sort_pairs(W.temp, s, W.keys.p, W.keys_s.p, W.vals.p, W.vals_s.p, ne, (unsigned)(3 * nb)));
  } else {
    // two stable passes: by the largest id, then by smallest << 32 | middle
    FB_TRY(sort_pairs(W.temp, s, W.keys.p, W.keys_s.p, W.vals.p, W.vals_s.p, ne, (unsigned)nb));
    FB_TRY(launch_1d(k_parts_keys_ab, (long long)ne, s, ne, M.tets, W.vals_s.p, W.keys_s.p));
    FB_TRY(sort_pairs(W.temp, s, W.keys_s.p, W.keys.p, W.vals_s.p, W.vals.p, ne, (unsigned)(32 + nb)));
    keys_sorted = W.keys.p;
    pay_sorted = W.vals.p;
  }
  // (the seed forest in `root`, the hooking's forest in `parent`, the flattened roots in `root` again)
  FB_TRY(launch_1d(k_parts_seed, (long long)ne, s, ne, keys_sorted, pay_sorted, M.tets, wide ? 1 : 0, P.root.p));
  // (... and the seed roots once more in `rank`, which is free until the scan behind the flatten and takes the jump rounds' turns too)
  for (int r = 0; r < 2; r++) {
    FB_TRY(launch_1d(k_parts_seed_jump, nt, s, nt, P.root.p, P.rank.p));
    FB_TRY(launch_1d(k_parts_seed_jump, nt, s, nt, P.rank.p, P.root.p));
  }
  FB_TRY(launch_1d(k_parts_seed_roots, nt, s, nt, P.root.p, P.parent.p, P.rank.p));
  FB_TRY(launch_1d(k_parts_hook, (long long)ne, s, ne, keys_sorted, pay_sorted, M.tets, wide ? 1 : 0, P.rank.p, P.parent.p));
  FB_TRY(launch_1d(k_parts_flatten, nt, s, nt, P.parent.p, P.root.p, P.flag.p));
  // ---- the parts ----
  FB_TRY(exclusive_scan(W.temp, s, P.flag.p, P.rank.p, 0, (size_t)nt + 1));
  int np = 0;
  FB_HIP(hipMemcpyAsync(&np, P.rank.p + nt, sizeof(int), hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));  // the first host wait
  if (np < 1 || np > nt) return fail(FB_EDEVICE, "parts: %d parts of %d elements", np, nt);
  P.n_parts = np;
  P.n_nodes = nn;
  P.n_tets = nt;
  FB_TRY(P.part_off.alloc((size_t)np + 1)); FB_TRY(P.part_first.alloc((size_t)np)); FB_TRY(P.part_nodes.alloc((size_t)np)); FB_TRY(P.part_front.alloc((size_t)np));
  FB_TRY(P.part_class.alloc((size_t)np)); FB_TRY(P.chunk_cnt.alloc((size_t)np + 1)); FB_TRY(P.chunk_off.alloc((size_t)np + 1)); FB_TRY(P.part_volume.alloc((size_t)np));
  FB_TRY(launch_1d(k_parts_label, nt, s, nt, P.root.p, P.flag.p, P.rank.p, P.element_part.p, P.part_first.p));
  // the elements grouped by part: stable, so ascending inside a part (the face sort's arrays are free again)
  uint32_t* pk_s = reinterpret_cast<uint32_t*>(W.keys_s.p);
  FB_TRY(sort_pairs(W.temp, s, reinterpret_cast<const uint32_t*>(P.element_part.p), pk_s, rocprim::counting_iterator<uint32_t>(0u), P.sorted.p, (size_t)nt, (unsigned)bits_of(np)));
  FB_TRY(launch_1d(k_parts_heads, nt, s, nt, pk_s, np, P.part_off.p));
  FB_TRY(P.best.zero(s));
  FB_TRY(launch_1d(k_parts_chunks, np + 1, s, np, P.part_off.p, P.chunk_cnt.p, P.best.p));
  FB_TRY(exclusive_scan(W.temp, s, P.chunk_cnt.p, P.chunk_off.p, 0, (size_t)np + 1));
  FB_TRY(parts_volumes(s, P, M));
  // ---- the nodes ----
  FB_TRY(fill_bytes(s, P.node_part.p, 0x7f, sizeof(int) * (size_t)nn));
  FB_TRY(P.node_flag.zero(s)); FB_TRY(P.part_nodes.zero(s)); FB_TRY(P.counts.zero(s));
  FB_TRY(launch_1d(k_parts_node_min, nt, s, nt, M.tets, P.element_part.p, P.node_part.p));
  FB_TRY(launch_1d(k_parts_node_shared, nt, s, nt, M.tets, P.element_part.p, P.node_part.p, P.node_flag.p, P.foreign.p));
  FB_TRY(launch_1d(k_parts_node_out, nn, s, nn, P.node_part.p, P.node_flag.p, M.caller_of, P.node_part_out.p, P.part_nodes.p, P.counts.p));
  int cnt[3] = {0, 0, 0};
  unsigned long long best = 0;
  FB_HIP(hipMemcpyAsync(cnt, P.counts.p, sizeof(cnt), hipMemcpyDeviceToHost, s));
  FB_HIP(hipMemcpyAsync(&best, P.best.p, sizeof(best), hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));  // the second host wait
  if (cnt[1] < 0 || cnt[1] > nn || cnt[2] < 0 || cnt[2] > nn) return fail(FB_EDEVICE, "parts: node counts %d, %d out of range", cnt[1], cnt[2]);
  P.n_shared_nodes = cnt[1];
  P.n_unused_nodes = cnt[2];
  P.largest_part = (int)(0xffffffffu - (unsigned)(best & 0xffffffffu));
  if (P.largest_part < 0 || P.largest_part >= np) return fail(FB_EDEVICE, "parts: largest part %d of %d", P.largest_part, np);
  if (cnt[1]) {
    // parts that touch at a node or an edge: the node counts once more in every further part that uses it
    FB_TRY(launch_1d(k_parts_corner_keys, nt, s, nt, M.tets, P.element_part.p, W.keys.p));
    FB_TRY(select_flagged(W.temp, s, W.keys.p, P.foreign.p, W.keys_s.p, P.counts.p + 3, ne));
    int nf = 0;
    FB_HIP(hipMemcpyAsync(&nf, P.counts.p + 3, sizeof(int), hipMemcpyDeviceToHost, s));
    FB_HIP(hipStreamSynchronize(s));
    if (nf < 1 || (size_t)nf > ne) return fail(FB_EDEVICE, "parts: %d foreign corners", nf);
    FB_TRY(sort_pairs(W.temp, s, W.keys_s.p, W.keys.p, W.vals.p, W.vals_s.p, (size_t)nf, (unsigned)(32 + bits_of(np))));
    FB_TRY(launch_1d(k_parts_foreign_count, nf, s, nf, W.keys.p, P.part_nodes.p));
  }
  P.valid = true;
  P.n_builds++;
  return FB_OK;
}

int parts_split(hipStream_t s, PartsWork& P, const PartsMesh& M, const double c[3], const double n[3], const double shift[3], bool apply, int out4[4]) {
  const int nt = M.n_tets, nn = M.n_nodes, np = P.n_parts;
  Vec3 vc, vn, vs;
  for (int k = 0; k < 3; k++) { vc.v[k] = c[k]; vn.v[k] = n[k]; vs.v[k] = shift[k]; }
  FB_TRY(P.part_front.zero(s)); FB_TRY(P.node_flag.zero(s));
  FB_TRY(fill_bytes(s, P.counts.p + 4, 0, 4 * sizeof(int)));
  FB_TRY(launch_1d(k_split_front, nt, s, nt, M.tets, M.x0, M.q, vc, vn, P.element_part.p, P.part_front.p));
  FB_TRY(launch_1d(k_split_classify, np, s, np, P.part_front.p, P.part_off.p, P.part_class.p, P.counts.p));
  FB_TRY(launch_1d(k_split_nodes, nt, s, nt, M.tets, P.element_part.p, P.part_class.p, P.node_flag.p));
  FB_TRY(launch_1d(k_split_move, nn, s, nn, P.node_flag.p, M.x0, vs, apply ? 1 : 0, P.counts.p));
  return P.counts.download(out4, 4, s, 4);
}

int parts_extract(hipStream_t s, PartsWork& P, const PartsMesh& M, int part, int* n_el, int* n_nd, int* first, PlanWorkspace& W) {
  int off[2] = {0, 0};
  FB_TRY(P.part_off.download(off, 2, s, (size_t)part));
  const int ne = off[1] - off[0];
  if (off[0] < 0 || ne < 1 || off[1] > M.n_tets) return fail(FB_EDEVICE, "parts: part %d spans [%d, %d)", part, off[0], off[1]);
  const int nc = 4 * ne;
  const uint32_t* ids = P.sorted.p + off[0];
  FB_TRY(P.node_key.reserve((size_t)M.n_nodes)); FB_TRY(P.node_local.reserve((size_t)M.n_nodes));
  FB_TRY(P.cflag.reserve((size_t)nc + 1)); FB_TRY(P.cpos.reserve((size_t)nc + 1));
  FB_TRY(P.out_nodes.reserve((size_t)std::min(nc, M.n_nodes))); FB_TRY(P.out_xyz.reserve((size_t)3 * std::min(nc, M.n_nodes))); FB_TRY(P.out_tets.reserve((size_t)nc));
  FB_TRY(fill_bytes(s, P.node_key.p, 0x7f, sizeof(int) * (size_t)M.n_nodes));
  FB_TRY(launch_1d(k_part_node_keys, ne, s, ne, ids, M.tets, P.node_key.p));
  FB_TRY(launch_1d(k_part_first_use, nc + 1, s, nc, ids, M.tets, P.node_key.p, P.cflag.p));
  FB_TRY(exclusive_scan(W.temp, s, P.cflag.p, P.cpos.p, 0, (size_t)nc + 1));
  // (a node has one first use: the positions are below min(4 n_el, n_nodes) whatever the count read back below says)
  FB_TRY(launch_1d(k_part_emit_nodes, nc, s, nc, ids, M.tets, P.cflag.p, P.cpos.p, M.caller_of, M.x0, P.node_local.p, P.out_nodes.p, P.out_xyz.p));
  FB_TRY(launch_1d(k_part_emit_tets, nc, s, nc, ids, M.tets, P.node_local.p, P.out_tets.p));
  int nd = 0;
  FB_TRY(P.cpos.download(&nd, 1, s, (size_t)nc));
  if (nd < 1 || nd > std::min(nc, M.n_nodes)) return fail(FB_EDEVICE, "parts: part %d uses %d nodes", part, nd);
  *n_el = ne; *n_nd = nd; *first = off[0];
  return FB_OK;
}

}  // namespace fb

// ---- the C ABI ----

namespace fb {  // (for detach.hip too)
PartsMesh parts_mesh(fb_fem_s* h) {
  PartsMesh M;
  M.n_nodes = h->plan.n_global; M.n_tets = h->plan.n_tets;
  M.tets = h->tets.p; M.x0 = h->x0.p; M.q = h->q.p;
  M.caller_of = h->ren.active ? h->ren.d_old_of_new.p : nullptr;
  return M;
}
int parts_current(fb_fem_s* h, bool force) {
  if (h->parts.valid && !force) return FB_OK;
  SlackScope slack(handle_slack_now(h));
  const char* wk = getenv("FEMBRAIN_PARTS_WIDE_KEYS");  // read at every build, like FEMBRAIN_SURFACE_WIDE_KEYS
  return parts_build(h->stream, h->parts, parts_mesh(h), wk && atoi(wk) != 0, h->plan_ws);
}
}  // namespace fb

namespace {

int parts_ready(fb_fem_s* h, const char* who, bool force) {
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "%s is for unsharded handles", who);
  return fb::parts_current(h, force);
}

// the plane of a swept quad (CuttableMesh.cpp:555-564) and the shift; FB_EINVAL for a quad without a normal or a number that is none
int split_plane(const double* quad, double dist, double c[3], double n[3], double shift[3]) {
  if (!quad) return fail(FB_EINVAL, "fb_fem_split_parts: null quad");
  for (int k = 0; k < 12; k++)
    if (!std::isfinite(quad[k])) return fail(FB_EINVAL, "fb_fem_split_parts: quad coordinate %d is not finite", k);
  if (!std::isfinite(dist)) return fail(FB_EINVAL, "fb_fem_split_parts: dist is not finite");
  const double a[3] = {quad[3] - quad[0], quad[4] - quad[1], quad[5] - quad[2]}, b[3] = {quad[6] - quad[0], quad[7] - quad[1], quad[8] - quad[2]};
  const double cr[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double len = std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
  if (!(len > 0.0) || !std::isfinite(len)) return fail(FB_EINVAL, "fb_fem_split_parts: the quad's first three points span no plane");
  for (int k = 0; k < 3; k++) {
    n[k] = cr[k] / len;
    shift[k] = n[k] * dist;
    c[k] = (((quad[k] + quad[3 + k]) + quad[6 + k]) + quad[9 + k]) * 0.25;
    if (!std::isfinite(shift[k])) return fail(FB_EINVAL, "fb_fem_split_parts: the shift is not finite");
  }
  return FB_OK;
}

}  // namespace

extern "C" {

int fb_fem_parts(fb_fem_t h, fb_fem_parts_info* out) {
  CHECK_HANDLE(h);
  FB_TRY(parts_ready(h, "fb_fem_parts", false));
  const PartsWork& P = h->parts;
  if (out) {
    out->n_parts = P.n_parts; out->n_builds = P.n_builds; out->largest_part = P.largest_part;
    out->n_shared_nodes = P.n_shared_nodes; out->n_unused_nodes = P.n_unused_nodes;
  }
  return FB_OK;
}

int fb_fem_read_parts(fb_fem_t h, int* element_part, int* node_part, int* part_elements, int* part_nodes, int* part_first_element, double* part_volume) {
  CHECK_HANDLE(h);
  FB_TRY(parts_ready(h, "fb_fem_read_parts", false));
  const PartsWork& P = h->parts;
  hipStream_t s = h->stream;
  const size_t np = (size_t)P.n_parts;
  if (element_part) FB_TRY(P.element_part.download(element_part, (size_t)P.n_tets, s));
  if (node_part) FB_TRY(P.node_part_out.download(node_part, (size_t)P.n_nodes, s));
  if (part_elements) {
    std::vector<int> off(np + 1);
    FB_TRY(P.part_off.download(off.data(), np + 1, s));
    for (size_t k = 0; k < np; k++) part_elements[k] = off[k + 1] - off[k];
  }
  if (part_nodes) FB_TRY(P.part_nodes.download(part_nodes, np, s));
  if (part_first_element) FB_TRY(P.part_first.download(part_first_element, np, s));
  if (part_volume) FB_TRY(P.part_volume.download(part_volume, np, s));
  return FB_OK;
}

int fb_fem_split_parts(fb_fem_t h, const double quad_xyz[12], double dist, fb_fem_split_info* out) {
  CHECK_HANDLE(h);
  if (h->plan.n_ranks > 1) return fail(FB_EINVAL, "fb_fem_split_parts is for unsharded handles");
  double c[3], n[3], shift[3];
  FB_TRY(split_plane(quad_xyz, dist, c, n, shift));
  FB_TRY(parts_ready(h, "fb_fem_split_parts", false));
  int got[4] = {0, 0, 0, 0};
  const PartsMesh M = parts_mesh(h);
  FB_TRY(parts_split(h->stream, h->parts, M, c, n, shift, true, got));
  // the rest shape has changed: element rest data as fb_fem_rebuild_elements leaves them, surface and stress stale; the labels stay.
  // (h->x0 is the one copy a later re-sync reads: xyz_in and x0_stage are filled anew from its input by every build)
  // A renumbered handle derived its node order (and the keys later cuts merge new nodes by) from the old positions: it is built again
  // from its own mesh, which is what makes it the handle a caller would create from fb_fem_read_mesh's arrays; state and forces are carried.
  h->system_valid = false;
  h->surf.valid = h->stress.valid = false;
  h->embed.grid.valid = false;  // (fb_fem_embed: bindings hold, ids and weights; a later search needs a grid over the moved positions)
  if (h->ren.active) FB_TRY(refresh_node_order(h));  // (an unsharded handle with an internal order has a device-built plan: the host builder works in the caller's order)
  else FB_TRY(launch_rest(h));
  FB_TRY(parts_volumes(h->stream, h->parts, parts_mesh(h)));
  if (out) {
    out->n_front_parts = got[0]; out->n_back_parts = got[1]; out->n_straddling_parts = got[2]; out->n_nodes_moved = got[3];
    for (int k = 0; k < 3; k++) out->shift[k] = shift[k];
  }
  return FB_OK;
}

int fb_fem_read_part(fb_fem_t h, int part, int* element_ids, int* node_ids, double* rest_xyz, int* tets_local) {
  CHECK_HANDLE(h);
  FB_TRY(parts_ready(h, "fb_fem_read_part", false));
  PartsWork& P = h->parts;
  if (part < 0 || part >= P.n_parts) return fail(FB_EINVAL, "fb_fem_read_part: part %d outside [0, %d)", part, P.n_parts);
  hipStream_t s = h->stream;
  SlackScope slack(handle_slack_now(h));
  int ne = 0, nd = 0, first = 0;
  FB_TRY(parts_extract(s, P, parts_mesh(h), part, &ne, &nd, &first, h->plan_ws));
  if (element_ids) FB_TRY(P.sorted.download(reinterpret_cast<uint32_t*>(element_ids), (size_t)ne, s, (size_t)first));
  if (node_ids) FB_TRY(P.out_nodes.download(node_ids, (size_t)nd, s));
  if (rest_xyz) FB_TRY(P.out_xyz.download(rest_xyz, (size_t)3 * nd, s));
  if (tets_local) FB_TRY(P.out_tets.download(tets_local, (size_t)4 * ne, s));
  return FB_OK;
}

int fb_fem_parts_wide(struct fb_fem_s* h) { return h && h->parts.n_builds ? (h->parts.wide ? 1 : 0) : -1; }

int fb_fem_time_parts(fb_fem_t h, int reps, double* seconds_label, double* seconds_split) {
  CHECK_HANDLE(h);
  if (reps < 1) return fail(FB_EINVAL, "reps must be positive");
  FB_TRY(parts_ready(h, "fb_fem_time_parts", false));  // warm: the buffers exist
  if (seconds_label) FB_TRY(timed_median(h, reps, [&] { return parts_ready(h, "fb_fem_time_parts", true); }, seconds_label));
  if (seconds_split) {
    // a split's device work without its stores: the plane x = 0, a zero shift, the element rest data and the volumes behind it
    const double c[3] = {0, 0, 0}, n[3] = {1, 0, 0}, shift[3] = {0, 0, 0};
    int got[4];
    const PartsMesh M = parts_mesh(h);
    FB_TRY(timed_median(h, reps, [&] {
      FB_TRY(parts_split(h->stream, h->parts, M, c, n, shift, false, got));
      FB_TRY(launch_rest(h));
      return parts_volumes(h->stream, h->parts, M);
    }, seconds_split));
    h->system_valid = false;  // (launch_rest: the mass entries are made again at the next assembly)
  }
  return FB_OK;
}

}  // extern "C"
