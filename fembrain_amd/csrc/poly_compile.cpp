// The polygonizer's host compiler (see poly_program.h).  Pure C++, no device calls: the evaluation program of a BlobTree under the three
// field semantics, the support boxes of its primitives, and the marching-cubes triangle table.
#include "poly_program.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace fb {

int fail(int code, const char* fmt, ...);  // fem_plan.cpp

#define FB_TRY(expr) do { int _r = (expr); if (_r != FB_OK) return _r; } while (0)  // (common.h's)

namespace {

// Emulates the operator stack walk of FieldComputer::fieldValue (Polygonizer.cpp:1938-2080) once on the host and records
// the order in which operators get evaluated.  Operator results go to numbered slots (the reference keeps one float per
// operator; here a slot is recycled as soon as its consumer has been emitted).  An instance of an operator
// (computePrimitiveField :1879-1901 calls fieldValue on the original subtree at the mapped point) is expanded in place:
// ENTER (save point and running field, map the point, cull against the original's box) .. subtree .. LEAVE (result to a
// slot, restore).  Instances of primitives are followed by prim_field on the device.
struct TreeCompiler {
  const TreeSource& t;
  std::vector<Instr> prog;
  std::vector<char> used;
  int depth = 1, nest = 0;

  int alloc(int n) {
    for (int base = 0;; base++) {
      bool ok = true;
      for (int k = 0; k < n && ok; k++) ok = base + k >= (int)used.size() || !used[base + k];
      if (!ok) continue;
      if ((int)used.size() < base + n) used.resize(base + n, 0);
      for (int k = 0; k < n; k++) used[base + k] = 1;
      depth = std::max(depth, base + n);
      return base;
    }
  }
  void add_slot(int slot, int ca, int cb) {  // ADDSLOT
    Instr add = {};
    add.kind = 4; add.a = slot; add.dst = -1; add.ca = ca; add.cb = cb;
    prog.push_back(add);
  }
  void release(int base, int n) { for (int k = 0; k < n; k++) used[base + k] = 0; }
  const float* prim(int i) const { return t.prims + 20 * (size_t)i; }
  const float* op(int i) const { return t.ops + 16 * (size_t)i; }

  // does primitive i, followed through instances of primitives, end in an instance of an operator?
  int resolves_to_op(int i, bool* yes) const {
    for (int hop = 0; hop < 8; hop++) {
      const float* P = prim(i);
      if ((int)P[0] != primInstance) { *yes = false; return FB_OK; }
      const int origin = (int)P[12], is_op = (int)P[14];
      if (is_op) {
        if (origin < 0 || origin >= t.n_ops) return fail(FB_EINVAL, "primitive %d instances operator %d of %d", i, origin, t.n_ops);
        *yes = true;
        return FB_OK;
      }
      if (origin < 0 || origin >= t.n_prims) return fail(FB_EINVAL, "primitive %d instances primitive %d of %d", i, origin, t.n_prims);
      i = origin;
    }
    return fail(FB_EINVAL, "instance chain of primitive %d does not end", i);
  }

  // value of primitive i (known to resolve to an operator instance) -> new slot
  int emit_instance(int i, int* slot) {
    if (++nest > 8) return fail(FB_EINVAL, "instanced subtrees nest deeper than 8 (primitive %d): an instance of its own ancestor?", i);
    const float* P = prim(i);
    const int origin = (int)P[12], is_op = (int)P[14];
    Instr in = {};
    in.kind = 2; in.a = (int)P[1]; in.b = alloc(5); in.dst = -1; in.ca = i;
    for (int a = 0; a < 3; a++) { in.lo[a] = -FLT_MAX; in.hi[a] = FLT_MAX; }
    if (is_op)
      for (int a = 0; a < 3; a++) { in.lo[a] = op(origin)[8 + a]; in.hi[a] = op(origin)[12 + a]; }
    const size_t enter = prog.size();
    const int frame = in.b;
    prog.push_back(in);
    if (is_op) {
      FB_TRY(subtree(origin));
    } else {  // instance of a primitive that is itself an instance of an operator
      int inner = -1;
      FB_TRY(emit_instance(origin, &inner));
      add_slot(inner, origin, 1);  // computeInstancedNodeFieldAndColor: the colour of the original primitive node
      release(inner, 1);
    }
    Instr out = {};
    out.kind = 3; out.a = frame;
    release(frame, 5);
    out.dst = *slot = alloc(1);
    prog[enter].skip = (int)prog.size();
    prog.push_back(out);
    if (prog.size() > (1u << 20)) return fail(FB_EINVAL, "instanced BlobTree expands to more than 2^20 evaluation steps");
    --nest;
    return FB_OK;
  }

  // primitive whose colour an operand primitive shows: itself, or -- for an instance of a primitive -- its immediate
  // original (computeInstancedNodeFieldAndColor, Polygonizer.cpp:2403-2409)
  int color_source(int i) const { return ((int)prim(i)[0] == primInstance && (int)prim(i)[14] == 0) ? (int)prim(i)[12] : i; }

  // operand reference of a primitive child: the primitive itself, or the slot of its expanded instance
  int operand(int i, int* ref, int* slot) {
    bool yes = false;
    FB_TRY(resolves_to_op(i, &yes));
    *slot = -1;
    if (!yes) { *ref = i; return FB_OK; }
    FB_TRY(emit_instance(i, slot));
    *ref = -1 - *slot;
    return FB_OK;
  }

  // the walk of fieldValue(.., idxRootNode = root); on return the root's value is the running field
  int subtree(int root) {
    const int nops = t.n_ops;
    std::vector<char> computed(nops, 0);
    std::vector<int> where(nops, -1);  // slot of a computed operator
    std::vector<int> stk{root};
    size_t guard = 0;
    while (!stk.empty()) {
      if (++guard > (size_t)4 * nops + 16) return fail(FB_EINVAL, "BlobTree operator graph is not a tree");
      const int n = stk.back();
      const float* o = op(n);
      const int type = (int)o[0], lc = (int)o[1], rc = (int)o[2], fl = (int)o[7];
      const bool unary = fl & ofIsUnaryOp, range = fl & ofChildIndexIsRange, lop = fl & ofLeftChildIsOp, rop = fl & ofRightChildIsOp;
      Instr in = {};
      in.dst = -1;
      if (range) {
        if (lc < 0 || rc >= t.n_prims || lc > rc) return fail(FB_EINVAL, "operator %d: bad primitive range [%d,%d]", n, lc, rc);
        stk.pop_back();
        int first = lc;  // runs of plain primitives, split at operator instances (same summation order)
        for (int i = lc; i <= rc; i++) {
          bool yes = false;
          FB_TRY(resolves_to_op(i, &yes));
          if (!yes) continue;
          if (first < i) { in.kind = 0; in.a = first; in.b = i - 1; prog.push_back(in); }
          int s = -1;
          FB_TRY(emit_instance(i, &s));
          add_slot(s, i, 0);  // inside a range the instance counts with its own node colour
          release(s, 1);
          first = i + 1;
        }
        if (first <= rc) { in.kind = 0; in.a = first; in.b = rc; prog.push_back(in); }
      } else {
        if ((lop && (lc < 0 || lc >= nops)) || (!lop && (lc < 0 || lc >= t.n_prims))) return fail(FB_EINVAL, "operator %d: bad left child %d", n, lc);
        if (!unary && ((rop && (rc < 0 || rc >= nops)) || (!rop && (rc < 0 || rc >= t.n_prims)))) return fail(FB_EINVAL, "operator %d: bad right child %d", n, rc);
        const bool ready = unary ? !(lop && !computed[lc]) : !((lop && !computed[lc]) || (rop && !computed[rc]));
        if (!ready) {
          if (lop && !computed[lc]) stk.push_back(lc);
          if (!unary && rop && !computed[rc]) stk.push_back(rc);
          continue;
        }
        stk.pop_back();
        int sa = -1, sb = -1;
        if (lop) { in.a = -1 - where[lc]; sa = where[lc]; } else FB_TRY(operand(lc, &in.a, &sa));
        if (unary) in.b = 0;
        else if (rop) { in.b = -1 - where[rc]; sb = where[rc]; } else FB_TRY(operand(rc, &in.b, &sb));
        in.kind = 1; in.optype = type; in.unary = unary ? 1 : 0;
        in.p0 = o[4]; in.p1 = o[5];
        in.ca = in.a >= 0 ? color_source(in.a) : 0;
        in.cb = (!unary && in.b >= 0) ? color_source(in.b) : 0;
        if (sa >= 0) release(sa, 1);
        if (sb >= 0 && sb != sa) release(sb, 1);
        prog.push_back(in);
      }
      computed[n] = 1;
      if (n != root) {  // the result of an inner operator is kept for its parent
        where[n] = alloc(1);
        prog.back().dst = where[n];
        // a RANGE that ended in an instance has an ADDSLOT last: give the store its own step
        if (prog.back().kind == 4) {
          prog.back().dst = -1;
          Instr keep = {};
          keep.kind = 0; keep.a = 0; keep.b = -1; keep.dst = where[n];  // empty range: only stores the running field
          prog.push_back(keep);
        }
      }
    }
    return FB_OK;
  }
};

// LinearBlobTree::setTraversalRoute (LinearBlobTree.cpp:333-429): start operator and `next` links of the stackless walk.
// The reference loop re-examines an operator after its operator children have been linked and pushes them again, so it
// never ends on an operator with two operator children; that (and a malformed graph) is reported instead of spinning.
int traversal_route(const TreeSource& t, std::vector<int>* next, int* start) {
  const int n = t.n_ops;
  next->assign(n, kNullBlob);
  *start = kNullBlob;
  std::vector<int> ops{0}, brk{kNullBlob};
  auto flags = [&](int o) { return (int)t.ops[16 * (size_t)o + 7]; };
  auto child = [&](int o, int k) { return (int)t.ops[16 * (size_t)o + 1 + k]; };
  auto is_op_id = [&](int c) { return c >= 0 && c < n; };
  size_t guard = 0;
  while (!ops.empty()) {
    if (++guard > (size_t)8 * n + 16) return fail(FB_EINVAL, "OpenCL field semantics: the reference's traversal-route builder does not terminate on this tree (an operator with two operator children)");
    int o = ops.back(), fl = flags(o);
    bool is_break = fl & ofBreak, lop = fl & ofLeftChildIsOp, rop = fl & ofRightChildIsOp;
    if (!lop && !rop) {
      if (brk.empty()) return fail(FB_EINVAL, "OpenCL field semantics: no traversal route (operator %d)", o);
      ops.pop_back();
      const int b = brk.back();
      brk.pop_back();
      if (b == kNullBlob) *start = o; else (*next)[b] = o;
      if (is_break) brk.push_back(o);
      while (!is_break && !ops.empty()) {
        o = ops.back();
        ops.pop_back();
        fl = flags(o);
        is_break = fl & ofBreak; lop = fl & ofLeftChildIsOp; rop = fl & ofRightChildIsOp;
        if (is_break) brk.push_back(o);
        if (lop) { if (!is_op_id(child(o, 0))) return fail(FB_EINVAL, "operator %d: bad left child", o); (*next)[child(o, 0)] = o; }
        if (rop) { if (!is_op_id(child(o, 1))) return fail(FB_EINVAL, "operator %d: bad right child", o); (*next)[child(o, 1)] = o; }
      }
    } else {
      if (lop) { if (!is_op_id(child(o, 0))) return fail(FB_EINVAL, "operator %d: bad left child", o); ops.push_back(child(o, 0)); }
      if (rop) { if (!is_op_id(child(o, 1))) return fail(FB_EINVAL, "operator %d: bad right child", o); ops.push_back(child(o, 1)); }
    }
  }
  if ((*next)[0] != kNullBlob) return fail(FB_EINVAL, "OpenCL field semantics: root operator has a next link (LinearBlobTree.cpp:408-412)");
  for (int i = 1; i < n; i++)
    if ((*next)[i] < 0 || (*next)[i] >= n) return fail(FB_EINVAL, "OpenCL field semantics: operator %d is not on the traversal route", i);
  return FB_OK;
}

// SEM_OPENCL: runs ComputeField / ComputeBranchField (Polygonizer.cl:781-886) symbolically.  The kernel keeps the values of
// finished subtrees in two registers per level (lf, rf: the outer pair of ComputeField, and the by-value copies of
// ComputeBranchField); which register an operator reads and writes depends on flags alone.  A register holds the constant 0,
// the value of a primitive at the query point (re-evaluated where it is read -- same value), or the result of an earlier step,
// which then lives in a slot for as long as a register names it.
int compile_tree_cl(const TreeSource& t, TreeProgram* out) {
  if (t.n_ops == 0) return FB_OK;
  std::vector<int> next;
  int start = kNullBlob;
  FB_TRY(traversal_route(t, &next, &start));
  const int n = t.n_ops;
  struct Val { int kind, id; };  // kind 0: constant 0, 1: primitive id, 2: slot id
  auto ref = [](const Val& v) { return v.kind == 0 ? kZeroOperand : (v.kind == 1 ? v.id : -1 - v.id); };
  Val OL{0, 0}, OR{0, 0}, IL{0, 0}, IR{0, 0};
  std::vector<char> used;
  auto new_slot = [&]() {
    const Val* regs[4] = {&OL, &OR, &IL, &IR};
    for (size_t k = 0; k < used.size(); k++) used[k] = 0;
    for (auto* r : regs)
      if (r->kind == 2) used[r->id] = 1;
    for (size_t k = 0; k < used.size(); k++)
      if (!used[k]) return (int)k;
    used.push_back(1);
    return (int)used.size() - 1;
  };
  size_t guard = 0;
  for (int op = start; op != kNullBlob;) {
    IL = OL; IR = OR;
    int next_op = kNullBlob;
    bool is_right = false;
    Val field{0, 0};
    for (int b = op; b != kNullBlob;) {
      if (++guard > (size_t)4 * n + 16) return fail(FB_EINVAL, "OpenCL field semantics: traversal route does not end");
      const float* o = t.ops + 16 * (size_t)b;
      const int type = (int)o[0], lc = (int)o[1], rc = (int)o[2], fl = (int)o[7];
      next_op = next[b];
      const bool is_break = fl & ofBreak, unary = fl & ofIsUnaryOp, range = fl & ofChildIndexIsRange, lop = fl & ofLeftChildIsOp, rop = fl & ofRightChildIsOp;
      is_right = fl & ofIsRightOp;
      Instr in = {};
      in.p0 = o[4]; in.p1 = o[5];
      if (range) {
        if (lc < 0 || rc >= t.n_prims || lc > rc) return fail(FB_EINVAL, "operator %d: bad primitive range [%d,%d]", b, lc, rc);
        in.kind = 5; in.optype = type; in.a = lc; in.b = rc;
      } else {
        if (!lop) { if (lc < 0 || lc >= t.n_prims) return fail(FB_EINVAL, "operator %d: bad left child %d", b, lc); IL = Val{1, lc}; }
        if (!unary && !rop) { if (rc < 0 || rc >= t.n_prims) return fail(FB_EINVAL, "operator %d: bad right child %d", b, rc); IR = Val{1, rc}; }
        in.kind = 6; in.optype = b;  // sic: ComputeOpField(idxBranchOp, ..), Polygonizer.cl:825
        in.a = ref(IL); in.b = ref(IR);
      }
      in.dst = new_slot();
      out->prog.push_back(in);
      field = Val{2, in.dst};
      if (is_right) IR = field; else IL = field;
      if (is_break) break;
      b = next_op;
    }
    if (is_right) OR = field; else OL = field;
    IL = OL; IR = OR;  // the by-value copies of the finished branch are gone
    op = next_op;
  }
  out->depth = std::max(1, (int)used.size());
  return FB_OK;
}

}  // namespace

int compile_tree(const TreeSource& t, TreeProgram* out) {
  out->prog.clear();
  out->depth = 1;
  if (t.sem == SEM_OPENCL) return compile_tree_cl(t, out);
  for (int i = 0; i < t.n_prims; i++) {  // validates every instance chain, used or not
    bool yes = false;
    TreeCompiler probe{t};
    FB_TRY(probe.resolves_to_op(i, &yes));
    if (yes && t.n_ops == 0) return fail(FB_EINVAL, "primitive %d instances an operator but the tree has none", i);
  }
  if (t.n_ops == 0) return FB_OK;
  TreeCompiler c{t};
  FB_TRY(c.subtree(0));
  out->prog = std::move(c.prog);
  out->depth = c.depth;
  if (out->depth > 60) return fail(FB_EINVAL, "BlobTree needs %d value slots per point (limit 60)", out->depth);
  return FB_OK;
}

// World-space box outside which primitive i contributes exactly 0.0f (see SegBox, poly.hip).  Local support = skeleton grown by the
// Wyvill radius 1 (field = max(0, (1 - d^2)^3)); mapped with the forward matrix (inverse of the stored matrix node) and
// padded generously against fp32 rounding of the distance and of the affine maps.  Anything not provably bounded
// (infinite line, instances, non-unit directions, singular matrices) gets an infinite box = is never culled.
void support_boxes(const TreeSource& t, TreeProgram* built) {
  const float inf = FLT_MAX;
  built->pbox.assign(6 * (size_t)t.n_prims, 0.0f);
  for (int i = 0; i < t.n_prims; i++) {
    const float* P = t.prims + 20 * (size_t)i;
    const int type = (int)P[0], im = (int)P[1];
    const double pos[3] = {P[4], P[5], P[6]}, dir[3] = {P[8], P[9], P[10]};
    const double r0 = P[12], r1 = P[13];
    double lo[3], hi[3];
    bool bounded = true, empty = false;
    const double dlen = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    const bool unit = std::fabs(dlen - 1.0) < 1e-3;
    auto ball = [&](double rad) { for (int a = 0; a < 3; a++) { lo[a] = pos[a] - rad; hi[a] = pos[a] + rad; } };
    switch (type) {
      case primPoint: ball(1.0); break;
      case primCylinder:
        if (!unit || !(r0 >= 0) || !(r1 >= 0)) { bounded = false; break; }
        for (int a = 0; a < 3; a++) {
          const double e0 = pos[a] - dir[a], e1 = pos[a] + dir[a] * (r1 + 1.0);
          lo[a] = std::min(e0, e1) - (r0 + 1.0); hi[a] = std::max(e0, e1) + (r0 + 1.0);
        }
        break;
      case primDisc: case primRing:
        if (!unit || !(r0 >= 0)) { bounded = false; break; }
        ball(r0 + 1.0);
        break;
      case primCube:
        if (!(r0 >= 0)) { bounded = false; break; }
        ball(r0 + 1.0);
        break;
      case primQuadricPoint:
        if (t.sem == SEM_OPENCL) { ball(std::max(1.0, std::sqrt(std::max(0.0, (double)P[10])))); break; }  // Wyvill value outside the radius
        if (!(P[10] >= 0)) { empty = true; break; }
        ball(std::sqrt((double)P[10]));
        break;
      case primTriangle: case primNULL: empty = true; break;  // wyvill(FLT_MAX) = wyvill(10) = 0
      case primInstance:
        if (t.sem == SEM_OPENCL) empty = true; else bounded = false;  // the kernel returns 0 for instanced nodes
        break;
      case primLine: bounded = false; break;
      default: empty = true; break;                           // unknown types evaluate to 0
    }
    float* out = built->pbox.data() + 6 * (size_t)i;
    if (empty) { out[0] = out[1] = out[2] = inf; out[3] = out[4] = out[5] = -inf; continue; }
    if (bounded && im != 0) {  // forward map of the 8 corners
      const float* m = t.mtx + 12 * (size_t)im;
      const double A[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]}, tr[3] = {m[3], m[7], m[11]};
      const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
      if (!(std::fabs(det) > 1e-12) || !std::isfinite(det)) bounded = false;
      else {
        double I[9];
        I[0] = (A[4] * A[8] - A[5] * A[7]) / det; I[1] = (A[2] * A[7] - A[1] * A[8]) / det; I[2] = (A[1] * A[5] - A[2] * A[4]) / det;
        I[3] = (A[5] * A[6] - A[3] * A[8]) / det; I[4] = (A[0] * A[8] - A[2] * A[6]) / det; I[5] = (A[2] * A[3] - A[0] * A[5]) / det;
        I[6] = (A[3] * A[7] - A[4] * A[6]) / det; I[7] = (A[1] * A[6] - A[0] * A[7]) / det; I[8] = (A[0] * A[4] - A[1] * A[3]) / det;
        double wlo[3] = {1e300, 1e300, 1e300}, whi[3] = {-1e300, -1e300, -1e300};
        for (int c = 0; c < 8; c++) {
          const double q[3] = {((c & 1) ? hi[0] : lo[0]) - tr[0], ((c & 2) ? hi[1] : lo[1]) - tr[1], ((c & 4) ? hi[2] : lo[2]) - tr[2]};
          for (int a = 0; a < 3; a++) {
            const double w = I[3 * a] * q[0] + I[3 * a + 1] * q[1] + I[3 * a + 2] * q[2];  // world = A^-1 (local - tr)
            wlo[a] = std::min(wlo[a], w); whi[a] = std::max(whi[a], w);
          }
        }
        for (int a = 0; a < 3; a++) { lo[a] = wlo[a]; hi[a] = whi[a]; }
      }
    }
    for (int a = 0; a < 3; a++) {
      if (!bounded || !std::isfinite(lo[a]) || !std::isfinite(hi[a])) { out[a] = -inf; out[3 + a] = inf; continue; }
      const double pad = 1e-2 + 1e-4 * std::max(std::fabs(lo[a]), std::fabs(hi[a]));
      out[a] = (float)(lo[a] - pad); out[3 + a] = (float)(hi[a] + pad);
    }
  }
}

// Triangle table: the cube table of Bloomenthal's polygonizer ("An implicit surface polygonizer", Graphics Gems IV),
// whose edge/corner/face naming the reference's _CellConfigTable.h carries: walk the crossed edges of each of the 256
// sign configurations clockwise around the faces into polygons, then fan every polygon around its last vertex.
// Generated at library load; tests pin it to the hash of the reference's own array (tests/golden/mc_table.json).
enum { eLB, eLT, eLN, eLF, eRB, eRT, eRN, eRF, eBN, eBF, eTN, eTF };
enum { fL, fR, fB, fT, fN, fF };
// corner = 4*dx + 2*dy + dz (LBN LBF LTN LTF RBN RBF RTN RTF)
const int kEdgeCorner1[12] = {0, 2, 0, 1, 4, 6, 4, 5, 0, 1, 2, 3};
const int kEdgeCorner2[12] = {1, 3, 2, 3, 5, 7, 6, 7, 4, 5, 6, 7};
const int kEdgeAxis[12] = {2, 2, 1, 1, 2, 2, 1, 1, 0, 0, 0, 0};

static int next_cw_edge(int edge, int face) {
  // the next edge clockwise around `face` (seen from outside the cube)
  static const int on_first[12] = {fL, fL, fL, fL, fR, fR, fR, fR, fB, fB, fT, fT};
  static const int if_first[12] = {eLF, eLN, eLB, eLT, eRN, eRF, eRT, eRB, eRB, eLB, eLT, eRT};
  static const int if_other[12] = {eBN, eTF, eTN, eBF, eBF, eTN, eBN, eTF, eLN, eRF, eRN, eLF};
  return face == on_first[edge] ? if_first[edge] : if_other[edge];
}

const CubeTable& cube_table() {
  static const CubeTable T = [] {
    static const int left_face[12] = {fB, fL, fL, fF, fR, fT, fN, fR, fN, fB, fT, fF};
    static const int right_face[12] = {fL, fT, fN, fL, fB, fR, fR, fF, fB, fF, fN, fT};
    CubeTable t;
    memset(t.tri, 255, sizeof t.tri);
    memset(t.edge_info, 0, sizeof t.edge_info);
    for (int e = 0; e < 12; e++) t.edge_info[e] = (unsigned char)(kEdgeCorner1[e] | (kEdgeAxis[e] << 4));
    for (int cfg = 0; cfg < 256; cfg++) {
      auto in = [cfg](int corner) { return (cfg >> corner) & 1; };
      bool done[12] = {false};
      int n = 0;
      for (int e0 = 0; e0 < 12; e0++) {
        if (done[e0] || in(kEdgeCorner1[e0]) == in(kEdgeCorner2[e0])) continue;
        int walk[12], nw = 0, e = e0, face = in(kEdgeCorner1[e0]) ? right_face[e0] : left_face[e0];
        do {
          e = next_cw_edge(e, face);
          done[e] = true;
          if (in(kEdgeCorner1[e]) != in(kEdgeCorner2[e])) {
            walk[nw++] = e;
            if (e != e0) face = face == left_face[e] ? right_face[e] : left_face[e];
          }
        } while (e != e0);
        // Bloomenthal prepends to his polygon list, so list order = reverse walk order; the fan apex is the list's last
        // entry (= first edge met) and the triangles come out from the far end of the list
        for (int k = nw - 3; k >= 0; k--) {
          t.tri[cfg][n++] = (unsigned char)walk[nw - 1 - k];
          t.tri[cfg][n++] = (unsigned char)walk[nw - 2 - k];
          t.tri[cfg][n++] = (unsigned char)walk[0];
        }
      }
      t.nvert[cfg] = (unsigned char)n;
    }
    return t;
  }();
  return T;
}

}  // namespace fb
