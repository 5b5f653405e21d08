// The BlobTree as the polygonizer evaluates it: the node types of the model arrays, the compiled evaluation program, and the compiler that makes
// one from the other (poly_compile.cpp).  Plain C++: the compiler builds and runs without the HIP runtime.
#pragma once
#include <vector>

#include "../../include/fembrain_hip.h"

namespace fb {

enum PrimType { primPoint, primLine, primCylinder, primDisc, primRing, primCube, primTriangle, primQuadricPoint, primNULL, primInstance, primRBF };
enum OpType { opUnion, opIntersect, opDif, opSmoothDif, opBlend, opRicciBlend, opGradientBlend, opFastQuadricPointSet, opCache,
              opWarpTwist, opWarpTaper, opWarpBend, opWarpShear };
enum OpFlags { ofRightChildIsOp = 1, ofLeftChildIsOp = 2, ofChildIndexIsRange = 4, ofIsUnaryOp = 8, ofIsRightOp = 16, ofBreak = 32 };
enum { SEM_CPU = FB_FIELD_CPU, SEM_CPU_BOX = FB_FIELD_CPU_BOX, SEM_OPENCL = FB_FIELD_OPENCL };
constexpr int kNullBlob = 0xFFFF;         // NULL_BLOB, LinearBlobTree.h:18
constexpr int kZeroOperand = -0x7fffffff;  // OpenCL program: an operand register that still holds its initial 0.0f

// one step of the compiled evaluation order.  Values live in numbered slots of a per-thread LDS column; the running
// field `out` and the query point are registers.
struct Instr {
  int kind;    // 0 RANGE: out += prims a..b.  1 OP.  2 ENTER an instanced subtree.  3 LEAVE it.  4 ADDSLOT: out += slot a
               // OpenCL program (SEM_OPENCL) only: 5 CL_RANGE: out = fold of prims a..b by optype.  6 CL_OP: out = op(a, b)
  int a, b;    // OP: left / right operand, >= 0 primitive index, < 0 slot -1-k.  ENTER: a = matrix node, b = first of the
               // 5 frame slots (x, y, z, out, inside).  LEAVE: a = frame slots
  int optype;  // OP only
  int unary;
  int dst;     // slot that receives the result (RANGE, OP, LEAVE); -1 = only `out`
  int skip;    // ENTER: index of the matching LEAVE (taken when the mapped point is outside the box)
  int ca, cb;  // colour pass: OP: primitive whose colour a primitive operand carries (an instance of a primitive shows the
               // original's colour).  ADDSLOT: ca = primitive whose colour weighs the slot, cb = 1 if the slot REPLACES the colour
               // ENTER: ca = the instance primitive itself (its own box is tested under SEM_CPU_BOX)
  float p0, p1;
  float lo[3], hi[3];  // ENTER: box of the original operator (isOutsideOp, Polygonizer.cpp:1464-1483)
};

// the marching-cubes triangle table (cube_table)
struct CubeTable {
  unsigned char tri[256][16];  // edge ids, 255 = end
  unsigned char nvert[256];
  unsigned char edge_info[16];  // per edge: bits 0-2 first corner, bits 4-5 axis
};

// what the compiler reads: the model arrays as fb_poly_create takes them (16 floats per operator, 20 per primitive, 12 per matrix node)
struct TreeSource {
  const float *ops, *prims, *mtx;  // mtx: support_boxes only
  int n_ops, n_prims, n_mtx;  // n_mtx is not read here: the caller has checked every primitive's matrix index against it (fb_poly_create)
  int sem;
};
// ... and what it writes
struct TreeProgram {
  std::vector<Instr> prog;
  int depth = 1;            // value slots per point
  std::vector<float> pbox;  // support box of every primitive (support_boxes)
};

int compile_tree(const TreeSource& t, TreeProgram* out);     // all three semantics; a refused tree leaves its message in fb_last_error
void support_boxes(const TreeSource& t, TreeProgram* built);  // built->pbox
const CubeTable& cube_table();

}  // namespace fb
