// fb_fem_cut's device pipeline (subdivide.h): cut codes, compaction, unique cut edges, new nodes and pieces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_prims.hip.h"
#include "launch.hip.h"
#include "subdivide.h"

namespace fb {
namespace {

// EPSILON is a float constant (base/MathBase.h:92) that IntersectRayTriangle compares a double against
constexpr double kCutEps = (double)0.0001f;
constexpr unsigned long long kNoEdge = ~0ULL;

struct D3 { double x, y, z; };
__host__ __device__ __forceinline__ D3 sub3(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ __forceinline__ double dot3(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ __forceinline__ D3 cross3(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__host__ __device__ __forceinline__ double len2(D3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }

// local edges of a tet: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
__device__ __forceinline__ int edge_a(int e) { return e < 3 ? 0 : (e < 5 ? 1 : 2); }
__device__ __forceinline__ int edge_b(int e) { return e < 3 ? e + 1 : (e < 5 ? e - 1 : 3); }
__device__ __forceinline__ int edge_of(int i, int j) {  // i != j, any order
  const int a = i < j ? i : j, b = i < j ? j : i;
  return a == 0 ? b - 1 : (a == 1 ? b + 1 : 5);
}
// case A: the three edges at one node; case B: four edges, the uncut two opposite
__device__ __forceinline__ int code_at(int n) { int c = 0; for (int e = 0; e < 6; e++) if (edge_a(e) == n || edge_b(e) == n) c |= 1 << e; return c; }
__device__ __forceinline__ int case_a_node(int code) { for (int n = 0; n < 4; n++) if (code == code_at(n)) return n; return -1; }
__device__ __forceinline__ int case_b_partner(int code) {  // the node that shares the uncut edge with node 0, -1 if not case B
  for (int x = 1; x < 4; x++) {
    const int e1 = edge_of(0, x), e2 = 5 - e1;  // (0,x) and its opposite edge: indices add up to 5
    if (code == (63 ^ (1 << e1) ^ (1 << e2))) return x;
  }
  return -1;
}

// IntersectRayTriangle (Intersections.cpp:95-130)
__device__ __forceinline__ bool ray_triangle(D3 ro, D3 rd, D3 p0, D3 p1, D3 p2, double* t) {
  const D3 e1 = sub3(p1, p0), e2 = sub3(p2, p0);
  const D3 q = cross3(rd, e2);
  const double a = dot3(e1, q);
  if (fabs(a) < kCutEps) return false;
  const double f = 1.0 / a;
  const D3 s = sub3(ro, p0);
  const double u = f * dot3(s, q);
  if (u < 0.0) return false;
  const D3 r = cross3(s, e1);
  const double v = f * dot3(rd, r);
  if ((v < 0.0) || ((u + v) > 1.0)) return false;
  *t = f * dot3(e2, r);
  return true;
}

// IntersectSegmentTriangle (Intersections.cpp:69-93) with the segment prepared once: rd = delta * (1 / |delta|) (Vec3::normalize)
struct Seg { D3 s0, rd; double len; };
__device__ __forceinline__ Seg make_seg(D3 s0, D3 s1) {
  Seg g;
  g.s0 = s0;
  D3 d = sub3(s1, s0);
  g.len = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
  if (g.len != 0.0) {
    const double inv = 1.0 / g.len;
    d.x *= inv; d.y *= inv; d.z *= inv;
  }
  g.rd = d;
  return g;
}
__device__ __forceinline__ bool segment_triangle(const Seg& g, D3 p0, D3 p1, D3 p2, double* t) {
  double tt;
  if (!ray_triangle(g.s0, g.rd, p0, p1, p2, &tt)) return false;
  if (!(tt >= 0.0 && tt <= g.len)) return false;
  *t = tt;
  return true;
}

__device__ __forceinline__ D3 quad_pt(const double* __restrict__ q, int k) { return {q[3 * k], q[3 * k + 1], q[3 * k + 2]}; }

// the edge lo -> hi against every quad: {q0,q2,q1}, then {q2,q3,q1} if that missed (CuttableMesh.cpp:166-199); cut iff an odd number of
// quads hit it; t of the last hit (the one that put the edge into the reference's map)
__device__ bool edge_cut(D3 plo, D3 phi, int n_quads, const double* __restrict__ quads, double* t_out) {
  const Seg g = make_seg(plo, phi);
  bool odd = false;
  double tl = 0.0;
  for (int k = 0; k < n_quads; k++) {
    const double* q = quads + 12 * k;
    const D3 q0 = quad_pt(q, 0), q1 = quad_pt(q, 1), q2 = quad_pt(q, 2), q3 = quad_pt(q, 3);
    double t;
    if (segment_triangle(g, q0, q2, q1, &t) || segment_triangle(g, q2, q3, q1, &t)) { odd = !odd; tl = t; }
  }
  *t_out = tl;
  return odd;
}

struct TetView { int g[4]; int in[4]; };  // caller ids, internal ids
__device__ __forceinline__ TetView tet_view(int4 t, const int* __restrict__ caller_of) {
  TetView v;
  v.in[0] = t.x; v.in[1] = t.y; v.in[2] = t.z; v.in[3] = t.w;
  for (int i = 0; i < 4; i++) v.g[i] = caller_of ? caller_of[v.in[i]] : v.in[i];
  return v;
}
__device__ __forceinline__ D3 cur_pos(int i, const double* __restrict__ x0, const double* __restrict__ q) {
  return {x0[3 * (size_t)i] + q[3 * (size_t)i], x0[3 * (size_t)i + 1] + q[3 * (size_t)i + 1], x0[3 * (size_t)i + 2] + q[3 * (size_t)i + 2]};
}

// counts: cut, case A, case B, unhandled
__global__ __launch_bounds__(kB) void k_cut_codes(int n_tets, const int4* __restrict__ tets, const int* __restrict__ caller_of, const double* __restrict__ x0,
                                                  const double* __restrict__ q, int n_quads, const double* __restrict__ quads, unsigned char* __restrict__ code,
                                                  int* __restrict__ counts) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n_tets) return;
  const TetView v = tet_view(tets[i], caller_of);
  D3 p[4];
  for (int k = 0; k < 4; k++) p[k] = cur_pos(v.in[k], x0, q);
  int c = 0;
  for (int e = 0; e < 6; e++) {
    const int a = edge_a(e), b = edge_b(e);
    const bool a_lo = v.g[a] < v.g[b];
    double t;
    if (edge_cut(a_lo ? p[a] : p[b], a_lo ? p[b] : p[a], n_quads, quads, &t)) c |= 1 << e;
  }
  code[i] = (unsigned char)c;
  if (c) {
    atomicAdd(counts, 1);
    if (case_a_node(c) >= 0) atomicAdd(counts + 1, 1);
    else if (case_b_partner(c) >= 0) atomicAdd(counts + 2, 1);
    else atomicAdd(counts + 3, 1);
  }
}

// the six edges of every cut element, (lo << 32 | hi) and t; and its piece count
__global__ __launch_bounds__(kB) void k_cut_edges(int n_cut, const int* __restrict__ cut_tets, const int4* __restrict__ tets, const int* __restrict__ caller_of,
                                                  const double* __restrict__ x0, const double* __restrict__ q, int n_quads, const double* __restrict__ quads,
                                                  const unsigned char* __restrict__ code, unsigned long long* __restrict__ keys, double* __restrict__ ts,
                                                  int* __restrict__ pieces) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_cut) return;
  const int id = cut_tets[j];
  const TetView v = tet_view(tets[id], caller_of);
  D3 p[4];
  for (int k = 0; k < 4; k++) p[k] = cur_pos(v.in[k], x0, q);
  const int c = code[id];
  for (int e = 0; e < 6; e++) {
    const int a = edge_a(e), b = edge_b(e);
    const bool a_lo = v.g[a] < v.g[b];
    const int lo = a_lo ? v.g[a] : v.g[b], hi = a_lo ? v.g[b] : v.g[a];
    double t = 0.0;
    unsigned long long key = kNoEdge;
    if ((c >> e) & 1) {
      (void)edge_cut(a_lo ? p[a] : p[b], a_lo ? p[b] : p[a], n_quads, quads, &t);  // (the same operations on the same inputs as pass 1)
      key = ((unsigned long long)(unsigned)lo << 32) | (unsigned)hi;
    }
    keys[6 * (size_t)j + e] = key;
    ts[6 * (size_t)j + e] = t;
  }
  pieces[j] = case_a_node(c) >= 0 ? 4 : 6;
}

__global__ __launch_bounds__(kB) void k_cut_heads(long long n, const unsigned long long* __restrict__ keys, int* __restrict__ head) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  head[i] = (k != kNoEdge && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

__global__ __launch_bounds__(kB) void k_cut_unique(long long n, const unsigned long long* __restrict__ keys, const double* __restrict__ ts,
                                                   const int* __restrict__ head, const int* __restrict__ pos, unsigned long long* __restrict__ ukeys,
                                                   double* __restrict__ ut, int* __restrict__ n_unique) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  if (head[i]) { ukeys[pos[i]] = keys[i]; ut[pos[i]] = ts[i]; }
  if (i == n - 1) *n_unique = pos[i] + head[i];
}

__device__ __forceinline__ int find_edge(int n_edges, const unsigned long long* __restrict__ ukeys, unsigned long long key) {
  int lo = 0, hi = n_edges - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ukeys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// new nodes: 2 per cut edge, lo's side then hi's side, at p_lo + normalize(p_hi - p_lo) * t (VolMesh::cut_edge, VolMesh.cpp:1636) in BAKE
// mode; at r_lo + f (r_hi - r_lo), f = t / |p_hi - p_lo|, in CARRY mode
__global__ __launch_bounds__(kB) void k_cut_nodes(int n_edges, const unsigned long long* __restrict__ ukeys, const double* __restrict__ ut, const int* __restrict__ internal_of,
                                                  const double* __restrict__ x0, const double* __restrict__ q, int carry, double* __restrict__ frac,
                                                  double* __restrict__ new_xyz) {
  const int k = blockIdx.x * kB + threadIdx.x;
  if (k >= n_edges) return;
  const int lo = (int)(ukeys[k] >> 32), hi = (int)(ukeys[k] & 0xffffffffu);
  const int il = internal_of ? internal_of[lo] : lo, ih = internal_of ? internal_of[hi] : hi;
  const D3 pl = cur_pos(il, x0, q), ph = cur_pos(ih, x0, q);
  const Seg g = make_seg(pl, ph);
  const double t = ut[k], f = t / g.len;
  frac[k] = f;
  D3 x;
  if (carry) {
    const D3 rl = {x0[3 * (size_t)il], x0[3 * (size_t)il + 1], x0[3 * (size_t)il + 2]}, rh = {x0[3 * (size_t)ih], x0[3 * (size_t)ih + 1], x0[3 * (size_t)ih + 2]};
    x = {rl.x + f * (rh.x - rl.x), rl.y + f * (rh.y - rl.y), rl.z + f * (rh.z - rl.z)};
  } else {
    x = {pl.x + g.rd.x * t, pl.y + g.rd.y * t, pl.z + g.rd.z * t};
  }
  for (int s = 0; s < 2; s++) {
    new_xyz[6 * (size_t)k + 3 * s] = x.x;
    new_xyz[6 * (size_t)k + 3 * s + 1] = x.y;
    new_xyz[6 * (size_t)k + 3 * s + 2] = x.z;
  }
}

// a piece vertex: an old local node (0..3) or the split point of local edge e on the side of local node n (8 + 4 e + n)
__device__ __forceinline__ int split_tok(int i, int j, int side) { return 8 + 4 * edge_of(i, j) + side; }

struct PieceCtx {
  const TetView* v;
  int n_nodes, n_edges;
  const unsigned long long* ukeys;
};
__device__ __forceinline__ int tok_id(const PieceCtx& c, int tok) {
  if (tok < 4) return c.v->g[tok];
  const int e = (tok - 8) >> 2, side = (tok - 8) & 3;
  const int ga = c.v->g[edge_a(e)], gb = c.v->g[edge_b(e)];
  const int lo = ga < gb ? ga : gb, hi = ga < gb ? gb : ga;
  const int k = find_edge(c.n_edges, c.ukeys, ((unsigned long long)(unsigned)lo << 32) | (unsigned)hi);
  return c.n_nodes + 2 * k + (c.v->g[side] == hi ? 1 : 0);
}
// barycentric coordinates in the parent (split points at their edge's midpoint), coordinates 1..3
__device__ __forceinline__ D3 tok_bary(int tok) {
  double b[4] = {0.0, 0.0, 0.0, 0.0};
  if (tok < 4) b[tok] = 1.0;
  else { const int e = (tok - 8) >> 2; b[edge_a(e)] = 0.5; b[edge_b(e)] = 0.5; }
  return {b[1], b[2], b[3]};
}
__device__ __forceinline__ double det3(D3 a, D3 b, D3 c) { return dot3(a, cross3(b, c)); }

struct PieceOut {
  int4* out;
  double* ratio;
  double* vol;
  double parent_vol;
  const double* x0;
  const double* new_xyz;
  const int* internal_of;
  int carry;
  const double* q;
};
__device__ __forceinline__ D3 rest_of(const PieceOut& o, const PieceCtx& c, int id) {
  if (id >= c.n_nodes) { const double* p = o.new_xyz + 3 * (size_t)(id - c.n_nodes); return {p[0], p[1], p[2]}; }
  const int i = o.internal_of ? o.internal_of[id] : id;
  if (o.carry) return {o.x0[3 * (size_t)i], o.x0[3 * (size_t)i + 1], o.x0[3 * (size_t)i + 2]};
  return cur_pos(i, o.x0, o.q);
}
// one piece: the vertex order with a positive barycentric volume (exact: the entries are 0, 1/2 and 1), its node ids, its volume ratio
__device__ void emit_piece(const PieceCtx& c, const PieceOut& o, int slot, int t0, int t1, int t2, int t3) {
  const D3 b0 = tok_bary(t0);
  if (det3(sub3(tok_bary(t1), b0), sub3(tok_bary(t2), b0), sub3(tok_bary(t3), b0)) < 0.0) { const int w = t2; t2 = t3; t3 = w; }
  const int4 id = {tok_id(c, t0), tok_id(c, t1), tok_id(c, t2), tok_id(c, t3)};
  o.out[slot] = id;
  const D3 p0 = rest_of(o, c, id.x);
  const double det = det3(sub3(rest_of(o, c, id.y), p0), sub3(rest_of(o, c, id.z), p0), sub3(rest_of(o, c, id.w), p0));
  o.ratio[slot] = det / o.parent_vol;
  o.vol[slot] = fabs(det) * (1.0 / 6);
}
// prism v0 v1 v2 | v3 v4 v5 (vi - v(i+3) lateral edges) into 3 tets by the lowest-global-id rule
__device__ void emit_prism(const PieceCtx& c, const PieceOut& o, int slot, const int v[6]) {
  int id[6], m = 0;
  for (int i = 0; i < 6; i++) { id[i] = tok_id(c, v[i]); if (id[i] < id[m]) m = i; }
  // the prism turned (rotation of the triangles, exchange of the two) so that the lowest id is w0
  int w[6], wid[6];
  const int layer = m / 3, rot = m % 3;
  for (int j = 0; j < 6; j++) {
    const int src = ((j / 3 + layer) & 1) * 3 + (j % 3 + rot) % 3;
    w[j] = v[src];
    wid[j] = id[src];
  }
  // the quad face w1 w2 w5 w4 not at w0: its diagonal through its lowest id
  if (min(wid[1], wid[5]) < min(wid[2], wid[4])) {
    emit_piece(c, o, slot, w[0], w[1], w[2], w[5]);
    emit_piece(c, o, slot + 1, w[0], w[1], w[5], w[4]);
  } else {
    emit_piece(c, o, slot, w[0], w[1], w[2], w[4]);
    emit_piece(c, o, slot + 1, w[0], w[4], w[2], w[5]);
  }
  emit_piece(c, o, slot + 2, w[0], w[4], w[5], w[3]);
}

__global__ __launch_bounds__(kB) void k_cut_pieces(int n_cut, const int* __restrict__ cut_tets, const int4* __restrict__ tets, const int* __restrict__ caller_of,
                                                   const int* __restrict__ internal_of, const double* __restrict__ x0, const double* __restrict__ q, int carry,
                                                   const unsigned char* __restrict__ code, const int* __restrict__ piece_off, int n_nodes, int n_edges,
                                                   const unsigned long long* __restrict__ ukeys, const double* __restrict__ new_xyz, int4* __restrict__ out,
                                                   double* __restrict__ ratio, int n_ratio) {
  const int j = blockIdx.x * kB + threadIdx.x;
  if (j >= n_cut) return;
  const int id = cut_tets[j];
  const TetView v = tet_view(tets[id], caller_of);
  const PieceCtx c = {&v, n_nodes, n_edges, ukeys};
  PieceOut o = {out, ratio, ratio + n_ratio, 0.0, x0, new_xyz, internal_of, carry, q};
  {
    D3 p[4];
    for (int k = 0; k < 4; k++) p[k] = rest_of(o, c, v.g[k]);
    o.parent_vol = det3(sub3(p[1], p[0]), sub3(p[2], p[0]), sub3(p[3], p[0]));
  }
  const int cc = code[id], slot = piece_off[j];
  const int a = case_a_node(cc);
  if (a >= 0) {
    int r[3], n = 0;
    for (int k = 0; k < 4; k++) if (k != a) r[n++] = k;
    emit_piece(c, o, slot, a, split_tok(a, r[0], a), split_tok(a, r[1], a), split_tok(a, r[2], a));
    const int prism[6] = {split_tok(a, r[0], r[0]), split_tok(a, r[1], r[1]), split_tok(a, r[2], r[2]), r[0], r[1], r[2]};
    emit_prism(c, o, slot + 1, prism);
  } else {
    // case B: uncut edges (a, b) with a = 0 and (c, d); the side of a b, then the side of c d
    const int pa = 0, pb = case_b_partner(cc);
    int rest[2], n = 0;
    for (int k = 1; k < 4; k++) if (k != pb) rest[n++] = k;
    const int pc = rest[0], pd = rest[1];
    const int side1[6] = {pa, split_tok(pa, pc, pa), split_tok(pa, pd, pa), pb, split_tok(pb, pc, pb), split_tok(pb, pd, pb)};
    const int side2[6] = {pc, split_tok(pa, pc, pc), split_tok(pb, pc, pc), pd, split_tok(pa, pd, pd), split_tok(pb, pd, pd)};
    emit_prism(c, o, slot, side1);
    emit_prism(c, o, slot + 3, side2);
  }
}

__global__ __launch_bounds__(kB) void k_cut_interp(int n_edges, const unsigned long long* __restrict__ ukeys, const double* __restrict__ frac, int n_nodes,
                                                   double* __restrict__ v) {
  const int k = blockIdx.x * kB + threadIdx.x;
  if (k >= n_edges) return;
  const int lo = (int)(ukeys[k] >> 32), hi = (int)(ukeys[k] & 0xffffffffu);
  const double f = frac[k];
  for (int c = 0; c < 3; c++) {
    const double a = v[3 * (size_t)lo + c], b = v[3 * (size_t)hi + c];
    const double x = a + f * (b - a);
    v[3 * ((size_t)n_nodes + 2 * k) + c] = x;
    v[3 * ((size_t)n_nodes + 2 * k + 1) + c] = x;
  }
}

__global__ __launch_bounds__(kB) void k_cut_bake(long long n3, double* __restrict__ x0, const double* __restrict__ q) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i < n3) x0[i] = x0[i] + q[i];
}

struct IsCut {
  __host__ __device__ int operator()(unsigned char c) const { return c != 0 ? 1 : 0; }
};
struct Unhandled {
  __device__ int operator()(unsigned char c) const { return (c != 0 && case_a_node(c) < 0 && case_b_partner(c) < 0) ? 1 : 0; }
};

}  // namespace

int cut_quads(int n_points, const double* strip, std::vector<double>& quads) {
  quads.clear();
  if (n_points < 4 || (n_points & 1) || !strip) return fail(FB_EINVAL, "a quad strip needs an even number of points, at least 4 (got %d)", n_points);
  // CuttableMesh::cut: quad i is strip points 2i .. 2i+3 (ctQuads = (size - 2) / 2); computeCutEdgesKernel skips a degenerate one
  for (int i = 0; 2 * i + 3 < n_points; i++) {
    const double* p = strip + 6 * (size_t)i;
    const D3 q0 = {p[0], p[1], p[2]}, q1 = {p[3], p[4], p[5]}, q2 = {p[6], p[7], p[8]}, q3 = {p[9], p[10], p[11]};
    for (int k = 0; k < 12; k++)
      if (!std::isfinite(p[k])) return fail(FB_EINVAL, "strip point %d is not finite", 2 * i + k / 3);
    const double area = len2(sub3(q1, q0)) * len2(sub3(q2, q0));
    if (area < kCutEps) continue;
    if (len2(sub3(q3, q2)) < kCutEps) continue;
    quads.insert(quads.end(), p, p + 12);
  }
  return FB_OK;
}

int cut_classify(hipStream_t s, CutWork& C, int n_tets, const int4* tets, const int* caller_of, const double* x0, const double* q, PlanWorkspace& W) {
  C.n_tets = n_tets;
  FB_TRY(C.code.reserve((size_t)std::max(1, n_tets)));
  FB_TRY(C.counts.reserve(8));
  FB_TRY(C.cut_tets.reserve((size_t)std::max(1, n_tets / 16)));
  FB_HIP(hipMemsetAsync(C.counts.p, 0, 8 * sizeof(int), s));
  FB_TRY(launch_1d(k_cut_codes, n_tets, s, n_tets, tets, caller_of, x0, q, C.n_quads, C.quads.p, C.code.p, C.counts.p));
  int h[4];
  FB_HIP(hipMemcpyAsync(h, C.counts.p, sizeof(h), hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  C.n_cut = h[0]; C.n_a = h[1]; C.n_b = h[2]; C.n_unhandled = h[3];
  if (C.n_cut == 0) return FB_OK;
  // the cut elements, ascending
  FB_TRY(C.cut_tets.reserve((size_t)C.n_cut));
  const auto flags = rocprim::make_transform_iterator(static_cast<const unsigned char*>(C.code.p), IsCut());
  rocprim::counting_iterator<int> ids(0);
  return select_flagged(W.temp, s, ids, flags, C.cut_tets.p, C.counts.p + 5, (size_t)n_tets);
}

int cut_read_unhandled(hipStream_t s, CutWork& C, PlanWorkspace& W) {
  C.unhandled_ids.clear();
  C.unhandled_codes.clear();
  if (C.n_unhandled == 0) return FB_OK;
  FB_TRY(C.sel.reserve((size_t)C.n_unhandled));
  const auto flags = rocprim::make_transform_iterator(static_cast<const unsigned char*>(C.code.p), Unhandled());
  rocprim::counting_iterator<int> ids(0);
  FB_TRY(select_flagged(W.temp, s, ids, flags, C.sel.p, C.counts.p + 6, (size_t)C.n_tets));
  const int n = std::min(C.n_unhandled, kCutUnhandledIds);
  C.unhandled_ids.resize(n);
  std::vector<unsigned char> all((size_t)C.n_tets);
  FB_HIP(hipMemcpyAsync(C.unhandled_ids.data(), C.sel.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
  FB_HIP(hipMemcpyAsync(all.data(), C.code.p, (size_t)C.n_tets, hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < n; k++) C.unhandled_codes.push_back(all[(size_t)C.unhandled_ids[k]]);
  return FB_OK;
}

int cut_emit(hipStream_t s, CutWork& C, int n_nodes, const int4* tets, const int* caller_of, const int* internal_of, const double* x0, const double* q,
             PlanWorkspace& W) {
  C.n_nodes = n_nodes;
  const int m = C.n_cut;
  const size_t ne = 6 * (size_t)m;
  FB_TRY(C.ekeys.reserve(ne)); FB_TRY(C.ekeys_s.reserve(ne));
  FB_TRY(C.et.reserve(ne)); FB_TRY(C.et_s.reserve(ne));
  FB_TRY(C.head.reserve(ne)); FB_TRY(C.hpos.reserve(ne));
  FB_TRY(C.piece_off.reserve((size_t)m + 1));
  FB_TRY(C.pcount.reserve((size_t)m + 1));
  FB_TRY(launch_1d(k_cut_edges, m, s, m, C.cut_tets.p, tets, caller_of, x0, q, C.n_quads, C.quads.p, C.code.p, C.ekeys.p, C.et.p, C.pcount.p));
  FB_TRY(sort_pairs(W.temp, s, C.ekeys.p, C.ekeys_s.p, C.et.p, C.et_s.p, ne, 64u));
  FB_TRY(launch_1d(k_cut_heads, (long long)ne, s, ne, C.ekeys_s.p, C.head.p));
  FB_TRY(exclusive_scan(W.temp, s, C.head.p, C.hpos.p, 0, ne));
  FB_TRY(C.ukeys.reserve(ne)); FB_TRY(C.ut.reserve(ne));
  FB_TRY(launch_1d(k_cut_unique, (long long)ne, s, ne, C.ekeys_s.p, C.et_s.p, C.head.p, C.hpos.p, C.ukeys.p, C.ut.p, C.counts.p + 4));
  FB_TRY(exclusive_scan(W.temp, s, C.pcount.p, C.piece_off.p, 0, (size_t)m));
  FB_HIP(hipMemcpyAsync(&C.n_edges, C.counts.p + 4, sizeof(int), hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  C.n_added = 4 * C.n_a + 6 * C.n_b;
  FB_TRY(C.frac.reserve((size_t)std::max(1, C.n_edges)));
  FB_TRY(C.new_xyz.reserve((size_t)std::max(1, 6 * C.n_edges)));
  FB_TRY(C.added.reserve((size_t)std::max(1, C.n_added)));
  FB_TRY(C.ratio.reserve(2 * ((size_t)std::max(1, C.n_added) + 1)));  // ratios, their minimum, absolute volumes, their minimum
  const int carry = C.mode == FB_CUT_CARRY ? 1 : 0;
  FB_TRY(launch_1d(k_cut_nodes, C.n_edges, s, C.n_edges, C.ukeys.p, C.ut.p, internal_of, x0, q, carry, C.frac.p, C.new_xyz.p));
  FB_TRY(launch_1d(k_cut_pieces, m, s, m, C.cut_tets.p, tets, caller_of, internal_of, x0, q, carry, C.code.p, C.piece_off.p, n_nodes, C.n_edges, C.ukeys.p, C.new_xyz.p, C.added.p,
                   C.ratio.p, C.n_added + 1));
  // the smallest piece-to-parent volume ratio (read back with the result)
  double* out = C.ratio.p + C.n_added;
  FB_TRY(min_reduce(W.temp, s, C.ratio.p, out, (size_t)C.n_added));
  FB_HIP(hipMemcpyAsync(&C.min_ratio, out, sizeof(double), hipMemcpyDeviceToHost, s));
  // ... and the smallest piece volume itself: what the fp32 records have to hold (fb_fem_cut refuses a cut they cannot)
  const double* vol = C.ratio.p + C.n_added + 1;
  double* vout = C.ratio.p + 2 * (size_t)C.n_added + 1;
  FB_TRY(min_reduce(W.temp, s, vol, vout, (size_t)C.n_added));
  FB_HIP(hipMemcpyAsync(&C.min_volume, vout, sizeof(double), hipMemcpyDeviceToHost, s));
  FB_HIP(hipStreamSynchronize(s));
  return FB_OK;
}

int cut_interpolate(hipStream_t s, const CutWork& C, int n_nodes, double* v) {
  if (C.n_edges == 0) return FB_OK;
  return launch_1d(k_cut_interp, C.n_edges, s, C.n_edges, C.ukeys.p, C.frac.p, n_nodes, v);
}

int cut_bake(hipStream_t s, long long n3, double* x0, const double* q) {
  if (n3 == 0) return FB_OK;
  return launch_1d(k_cut_bake, n3, s, n3, x0, q);
}

}  // namespace fb
