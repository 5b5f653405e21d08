// fb_fem_cut: the subdivision of CuttableMesh::cut (src/deformable/CuttableMesh.cpp:283-505, TetSubdivider.cpp:209-403) on the device.
//
// A blade's swept quad strip cuts every mesh edge an odd number of its quads cross (CuttableMesh.cpp:166-212: a second hit on an edge
// erases it), tested in fp64 against the CURRENT positions (VolMesh::pos = rest + q) with IntersectSegmentTriangle
// (src/graphics/Intersections.cpp:69-130), operation for operation.  Every element with a cut edge is case A (the three edges at one
// node cut: a corner tet and a prism, 4 pieces) or case B (four edges cut, the two uncut ones opposite: two prisms, 6 pieces); any other
// pattern refuses the whole cut (CUT_ERR_UNHANDLED_CUT_STATE).  Each cut edge gets two coincident nodes (VolMesh::cut_edge,
// VolMesh.cpp:1624-1660), one on either side, so the two sides come apart.
//
// Where this differs from the reference:
//  - every edge is tested from its lower to its higher caller node id (the reference: from -> to in VolMesh creation order);
//  - the unique cut edges are sorted by (lo, hi); cut edge k gets node N + 2k on lo's side and N + 2k + 1 on hi's side (N: nodes before
//    the cut); pieces are appended by ascending parent id in a fixed local order;
//  - a prism is split into 3 tets by the lowest-global-id rule (Dompierre et al., "How to subdivide pyramids, prisms and hexahedra into
//    tetrahedra"): each quad face is cut by the diagonal through its lowest-id vertex, so a face two cells share is split alike from both;
//    piece vertex order is fixed combinatorially (the sign of the piece in the parent's barycentric frame with every split point at its
//    edge's midpoint), so a piece has its parent's orientation whenever every split point lies strictly inside its edge.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"
#include "plan_device.h"

namespace fb {

constexpr int kCutUnhandledIds = 64;  // unhandled elements whose ids and codes a read-back returns (the lowest ids)

struct CutWork {
  int n_tets = 0, n_nodes = 0, mode = FB_CUT_BAKE, n_quads = 0;
  int n_cut = 0, n_a = 0, n_b = 0, n_unhandled = 0, n_edges = 0, n_added = 0;
  double min_ratio = 0.0;
  double min_volume = 0.0;                  // smallest piece volume in the new rest shape
  bool valid = false;                       // the read-back describes the last fb_fem_cut of the handle
  std::vector<int> unhandled_ids, unhandled_codes;
  DevBuf<double> quads;                     // usable quads, 12 doubles each (q0 q1 q2 q3)
  DevBuf<unsigned char> code;               // per element: its 6-bit cut code
  DevBuf<int> counts;                       // cut, case A, case B, unhandled, unique cut edges
  DevBuf<int> cut_tets;                     // ascending ids of the cut elements: the delta's `removed`
  DevBuf<int> pcount, piece_off;            // per cut element: its pieces (4 or 6), its first piece
  DevBuf<unsigned long long> ekeys, ekeys_s;  // (lo << 32 | hi) of the six edges of every cut element, ~0 where not cut; sorted
  DevBuf<double> et, et_s;                  // their t
  DevBuf<int> head, hpos;                   // first copy of a key in the sorted list; its rank
  DevBuf<unsigned long long> ukeys;         // the unique cut edges, ascending
  DevBuf<double> ut, frac;                  // their t and t / |current edge|
  DevBuf<int4> added;                       // the pieces, in the caller's numbering
  DevBuf<double> new_xyz;                   // rest positions of the 2 n_edges new nodes
  DevBuf<double> ratio;                     // per piece: its volume / its parent's (new rest shape)
  DevBuf<int> sel;                          // unhandled ids
};

// the usable quads of a strip (CuttableMesh.cpp:154-164: degenerate ones are skipped); FB_EINVAL for < 4 or an odd number of points
int cut_quads(int n_points, const double* strip, std::vector<double>& quads);
// Pass 1 on the handle's element list (node ids through caller_of when renumbered, nullptr otherwise; positions x0 + q): the code of
// every element, the cut ones compacted, the counts read back (the one host wait of the decision).  C.quads uploaded already.
int cut_classify(hipStream_t s, CutWork& C, int n_tets, const int4* tets, const int* caller_of, const double* x0, const double* q, PlanWorkspace& W);
// the first kCutUnhandledIds unhandled elements (ids ascending) and their codes into C.unhandled_ids / _codes
int cut_read_unhandled(hipStream_t s, CutWork& C, PlanWorkspace& W);
// Pass 2 on the cut elements: unique cut edges (read back: C.n_edges), new nodes (BAKE: the split point of the current shape; CARRY: the
// same edge fraction on the rest edge), the pieces and their volume ratio.  internal_of: caller id -> internal id (nullptr: identity).
int cut_emit(hipStream_t s, CutWork& C, int n_nodes, const int4* tets, const int* caller_of, const int* internal_of, const double* x0, const double* q,
             PlanWorkspace& W);
// CARRY: a 3-vector per node in the caller's numbering (n_nodes old ones filled) gets its 2 n_edges new entries by the edge fractions
int cut_interpolate(hipStream_t s, const CutWork& C, int n_nodes, double* v);
// BAKE: x0 += q over n3 entries
int cut_bake(hipStream_t s, long long n3, double* x0, const double* q);

}  // namespace fb
