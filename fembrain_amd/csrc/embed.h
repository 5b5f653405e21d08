// Point sets bound to the elements of the handle's tet mesh (embed.hip): fb_fem_embed / fb_fem_read_embedding / fb_fem_embed_update.
// What VolumetricMesh::generateInterpolationWeights with TetMesh::computeBarycentricWeights (src/3rdparty/vegafem/volumetricMesh/
// volumetricMesh.cpp:971-1134, tetMesh.cpp:233-305) compute on the host of the reference with a linear scan per point, and what
// Deformable::setDeformCallback's receiver does with them every frame.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.h"
#include "delta.h"
#include "plan_device.h"
#include "subdivide.h"

namespace fb {

constexpr int kEmbedSlots = 8;       // live embeddings of a handle
constexpr int kEmbedWideCells = 64;  // an element whose box covers more cells goes to the overflow list

// the handle's arrays the calls below work on: element list and fp64 rest positions in its internal order, the renumbering's maps
// (null: the caller's order is the internal one)
struct EmbedMesh {
  int n_nodes = 0, n_tets = 0;
  const int4* tets = nullptr;
  const double* x0 = nullptr;
  const int* caller_of = nullptr;
  const int* internal_of = nullptr;
};

// The search grid over the rest box of one mesh generation, shared by the handle's embeddings.
struct EmbedGrid {
  bool valid = false;
  int n_builds = 0;
  int dim[3] = {1, 1, 1};
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, inv[3] = {0, 0, 0}, pad = 0;  // the padded box, cells per unit length, the padding
  int n_wide = 0;
  long long n_pairs = 0;
  DevBuf<double> box_part;          // per-workgroup boxes of the nodes, the mesh box in the last six
  DevBuf<int> cnt, off;             // [n_tets + 1] cells of every element (0: overflow list) | their prefix sums
  DevBuf<unsigned char> wide_flag;  // [n_tets]
  DevBuf<int> wide, wide_count;     // ascending ids of the overflow list | its length
  DevBuf<int> cell_lo, cell_hi;     // [cells] the cell's run in cell_elem (both 0: empty)
  DevBuf<int> cell_elem;            // [n_pairs] elements grouped by cell, ascending inside a cell
};

// The grid of the element CENTRES over the same box and dim[3] (embed_closest.hip), for the points no element contains.  Nothing of it
// exists before a search takes the ring path; embed_mesh_changed retires it with the element grid.
struct EmbedCentreGrid {
  bool valid = false;
  int n_builds = 0;
  DevBuf<int> cell_cnt;     // [cells + 1] centres per cell, 0 in the last
  DevBuf<int> cell_start;   // [cells + 1] their exclusive prefix sums: a run of cells along x is one range of the arrays below
  DevBuf<double> centre;    // [3 n_tets] the centres grouped by cell, elements ascending inside a cell: 24 bytes each
  DevBuf<int> elem;         // [n_tets] ... and their elements
};

// what the external pass of an embedding's last search did (fb_fem_embed_search_info)
struct EmbedSearchStats {
  int path = FB_EMBED_CLOSEST_NONE, n_outside = 0, n_far = 0, max_one = 0;
  long long tested = 0;
};

// One embedding.  Nothing is allocated before fb_fem_embed.
struct Embedding {
  bool live = false;
  bool orphan_all = false;  // the mesh under it was replaced (fb_fem_resync): every point is searched again, from loc, when next read
  bool lost = false;        // a change of the mesh in place has begun and embed_follow has not (yet) carried the binding across it
  int n_orphans = 0;        // points whose element a change in place took away: searched again, from loc, when next read
  int n_points = 0, n_triangles = 0, n_external = 0, n_zeroed = 0, n_locates = 0, n_rebound = 0;
  double zero_threshold = 0.0;
  EmbedSearchStats search;
  float rest_box[6] = {0, 0, 0, 0, 0, 0};
  DevBuf<double> loc;              // [3 n] the point in the handle's rest shape: what a search looks for
  DevBuf<double> w;                // [4 n]
  DevBuf<int> elem, elem_old;      // [n] | the binding before the running search
  DevBuf<int> vert, vert_int;      // [4 n] node ids: the caller's | the handle's internal order (what the update gathers through)
  DevBuf<unsigned char> ext, zeroed, need;  // [n] external | weights zeroed | the running search found no containing element
  DevBuf<unsigned char> changed;   // [n] the running search or change moved the point to another element
  DevBuf<unsigned char> orphan;    // [n] the point waits for a search (allocated by the first change in place)
  DevBuf<int> tris;                // [3 n_triangles]
  DevBuf<uint32_t> inc;            // [3 n_triangles] 3 * triangle + corner grouped by point, triangles ascending inside a group
  DevBuf<int> inc_lo, inc_hi;      // [n] the point's run in inc (both 0: no triangle)
  DevBuf<double> cur;              // [3 n] fp64 positions of the last update (what the normals are made of)
  DevBuf<float> out;               // [6 n + 6] xyz, normals, box of the last update
  DevBuf<float> part;              // per-workgroup boxes
  std::vector<float> host;         // staging of `out`
  // The transpose of the binding (embed_touch.hip): nothing of it exists before the first fb_fem_embed_add_forces; it is stale whenever the
  // binding changes (a search, embed_follow, a release) and built again by the next add.
  bool tr_valid = false;
  int tr_builds = 0, tr_longest = 0, tr_touched = 0;  // builds since creation | longest run | nodes with a run, of the last build
  DevBuf<uint32_t> tr_corner;      // [4 n] corners 4 p + k grouped by internal node, ascending inside a group
  DevBuf<int> tr_lo, tr_hi;        // [n_nodes] the node's run in tr_corner (both 0: none)
  DevBuf<int> tr_nodes;            // [tr_touched] the nodes with a run, ascending
  DevBuf<unsigned char> tr_flag;   // [n_nodes] the node has a run (what tr_nodes is compacted from)
  DevBuf<double> f_stage;          // [3 n] the force on every point of the running add
  DevBuf<unsigned char> f_mask;    // [n] the points of the running add's list; zero between calls
  void release_all();
};

// what a pick on an embedding brings back in one copy: ray (t, u, v, the hit, the triangle) | point (dist2 in t, the point, its id)
struct EmbedPick {
  double t, u, v, xyz[3];
  int index, pad;
};

struct EmbedWork {
  int n_live = 0;
  Embedding slot[kEmbedSlots];
  EmbedGrid grid;
  DevBuf<int> ext_ids;   // points of the running search without a containing element
  DevBuf<double> close_d;  // [chunks][such points] the closest centre of every chunk of the element list: its distance
  DevBuf<int> close_e;     // ... and its element
  DevBuf<int> counts;    // [0] such points, [1] external, [2] zeroed, [3] changed element
  // embed_closest.hip; empty until a search takes the ring path
  EmbedCentreGrid cgrid;
  DevBuf<unsigned char> far_flag;  // [such points] the ring search gave the point up at its budget
  DevBuf<int> far_ids;             // those points, compacted: the full scan's list
  DevBuf<long long> ring_part;     // [3 workgroups + 4] per-workgroup far points | centres tested | most of one point; the folded three, the list's length
  // embed_touch.hip; empty until one of its entry points is called
  DevBuf<unsigned char> touch_args;  // one upload per add with a list: forces3[3 n] | ids[n]
  DevBuf<int> tr_stats;              // [0] nodes with a run, [1] the longest run of the table being built
  DevBuf<double> pick_d;             // per-workgroup minima of a pick ...
  DevBuf<int> pick_i;                // ... and their triangles / points
  DevBuf<EmbedPick> pick_out;
  DevBuf<float> vm_out;              // [n] fb_fem_embed_stress
};

// The grid of the mesh: count, scan, emit, one stable sort by cell.  Two host waits (the mesh box; pairs and overflow length).
int embed_grid_build(hipStream_t s, EmbedGrid& G, const EmbedMesh& M, PlanWorkspace& W);
// Every point of E from E.loc by the binding rule: element, vertices in both numberings, weights, flags and counts.  The grid must be
// valid.  count_rebound: E.elem holds a binding to compare with.  One host wait (the points without a containing element).
int embed_locate(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, bool count_rebound, PlanWorkspace& W);
// ... in its two halves: up to the host wait for the number of points without a containing element | the external pass, weights, counts
int embed_locate_search(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, bool count_rebound, PlanWorkspace& W, int* n_ext);
int embed_locate_finish(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, bool count_rebound, PlanWorkspace& W, int n_ext);
// The external pass alone: E.elem of the n_ext points of EW.ext_ids from the closest centre, E.search filled.  path: FB_EMBED_CLOSEST_SCAN
// (every centre for every point) or _RING (through the centre grid, built here if this mesh generation has none; the points past
// `budget` centres go to the scan).  One host wait on the ring path (the far points and the counters), none on the scan's.
int embed_closest(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, PlanWorkspace& W, int n_ext, int path, long long budget);
// the path a search with n_ext outside points takes, and its budget: FEMBRAIN_EMBED_CLOSEST / FEMBRAIN_EMBED_RING_BUDGET, else the rule
int embed_closest_choice(const EmbedWork& EW, const EmbedMesh& M, int n_ext, long long* budget);
// embed_closest.hip: the centre grid over EW.grid's box (no host wait) | the ring search (the host wait); n_far points are left in EW.far_ids
int embed_centre_grid_build(hipStream_t s, EmbedWork& EW, const EmbedMesh& M, PlanWorkspace& W);
int embed_closest_ring(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, PlanWorkspace& W, int n_ext, long long budget, int* n_far);
// false where a coordinate's rounding is not far below a cell of the grid (a box 2^30 of its extents from the origin): the ring's proof
// does not cover such a mesh and its searches scan
bool embed_ring_covers(const EmbedGrid& G);
// the incidence list of E.tris, grouped by point
int embed_incidence(hipStream_t s, Embedding& E, PlanWorkspace& W);
// Positions, normals and box into E.out (q null: the rest shape); copy_out: one copy of all three into E.host.
int embed_update(hipStream_t s, Embedding& E, int n_nodes, const double* x0, const double* q, bool copy_out);
// The handle's mesh is about to change: the grid is stale; every live embedding is searched again when next read (a replaced mesh), or
// -- a change in place -- unusable until embed_follow has run for it.
void embed_mesh_changed(EmbedWork& EW, bool in_place);
// A change in place (D: its marks and new element ids, still on the device; C: the cut behind it, null for any other change) has been
// applied to the handle, whose NEW arrays M describes.  Per point: in a kept element the new id, the same weights, internal ids derived
// again; in an element the cut subdivided the lowest-numbered piece that contains its location (the weighted sum of the parent's nodes
// in the new rest shape), else the piece with the closest centre; in any other removed or changed element an orphan.  bake: the rest
// shape moved under every point (FB_CUT_BAKE), loc is refreshed.  One launch and a count per embedding.
int embed_follow(hipStream_t s, EmbedWork& EW, Embedding& E, const EmbedMesh& M, const MeshDelta& D, const CutWork* C, bool bake);

// ---- embed_touch.hip: the way back from the drawn points to the tets ----
// The transposed table of E's binding: one stable sort of the 4 n corners by internal node, the runs, the nodes that have one.  One host wait.
int embed_table_build(hipStream_t s, EmbedWork& EW, Embedding& E, int n_nodes, PlanWorkspace& W);
// fext[3 v + c] += w * f for the corners of the points in `ids` (strictly ascending, validated by the caller; null: every point, n = n_points),
// per node in table order, the value of fext first.  The table must be valid.
int embed_scatter(hipStream_t s, EmbedWork& EW, Embedding& E, int n_nodes, int n, const int* ids, const double* forces3, double* fext);
// E.cur at the state q, as embed_update forms it
int embed_positions(hipStream_t s, Embedding& E, int n_nodes, const double* x0, const double* q);
// the nearest hit of the ray on E's triangles at E.cur (index -1: none) | the point of E.cur closest to wpos
int embed_pick_ray(hipStream_t s, EmbedWork& EW, Embedding& E, const double origin[3], const double dir[3], double t_max, EmbedPick* out);
int embed_pick_point(hipStream_t s, EmbedWork& EW, Embedding& E, const double wpos[3], EmbedPick* out);
// per point (float) vm[element of the point]
int embed_stress(hipStream_t s, EmbedWork& EW, const Embedding& E, int n_elements, const double* vm, float* per_point);

}  // namespace fb
