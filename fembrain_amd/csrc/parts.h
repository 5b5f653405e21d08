// Disjoint parts of the handle's tet mesh on the device (parts.hip): fb_fem_parts / fb_fem_read_parts / fb_fem_split_parts /
// fb_fem_read_part / fb_fem_time_parts.  What VolMesh::get_disjoint_parts (src/deformable/VolMesh.cpp:915-965),
// CuttableMesh::splitParts (src/deformable/CuttableMesh.cpp:553-626) and one iteration of convertDisjointPartsToMeshes (:628-698)
// compute on the host of the reference.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "plan_device.h"

namespace fb {

// Everything the labelling of one handle owns.  Nothing is allocated before the first build.
struct PartsWork {
  bool valid = false;      // the labels below belong to the handle's current mesh
  int n_builds = 0;
  int n_parts = 0, largest_part = 0, n_shared_nodes = 0, n_unused_nodes = 0;
  int n_nodes = 0, n_tets = 0;      // of the mesh it was built on
  bool wide = false;                // the last build took the two-pass (wide key) path
  DevBuf<int> parent;               // [n_tets] the union-find forest of the hooking launch
  DevBuf<int> root;                 // [n_tets] smallest element id of every element's part (the flatten launch); before the hooking, the seed forest
  DevBuf<int> flag, rank;           // [n_tets + 1] element is a root | roots before it (rank[n_tets]: the number of parts; during the hooking, every element's seed root)
  DevBuf<int> element_part;         // [n_tets]
  DevBuf<uint32_t> sorted;          // [n_tets] the elements grouped by part, ascending inside a part
  DevBuf<int> part_off;             // [n_parts + 1] first entry of every part in `sorted`
  DevBuf<int> part_first, part_nodes, part_front;  // [n_parts] smallest element | nodes used | elements in front of the last split's plane
  DevBuf<int> part_class;           // [n_parts] the last split's verdict: 1 front, 2 back, 0 straddling
  DevBuf<unsigned long long> best;  // elements << 32 | ~index of the largest part
  DevBuf<int> chunk_cnt, chunk_off; // [n_parts + 1] volume chunks of every part | chunks before it
  DevBuf<double> chunk_vol;         // a partial volume per chunk
  DevBuf<double> part_volume;       // [n_parts]
  // (node_part and node_flag are in the handle's INTERNAL node order and are scratch of the call that fills them: the build, a split.  They
  // do not survive refresh_node_order, which changes that order and keeps `valid`; nothing may read them across calls.)
  DevBuf<int> node_part;            // [n_nodes] internal order: lowest part using the node, kNone for none
  DevBuf<int> node_part_out;        // [n_nodes] caller order, -1 for none
  DevBuf<int> node_flag;            // [n_nodes] used by more than one part | the split's front / back bits
  DevBuf<unsigned char> foreign;    // [4 n_tets] the corner's node carries another part's label
  DevBuf<int> counts;               // [0] parts, [1] shared, [2] unused, [3] foreign corners, [4..7] the split's front / back / straddling / moved
  // fb_fem_read_part
  DevBuf<int> node_key;             // [n_nodes] first corner (4 rank + corner) of the part that uses the node
  DevBuf<int> node_local;           // [n_nodes] the node's index in the part
  DevBuf<int> cflag, cpos;          // [4 n_elements + 1] the corner is its node's first use | first uses before it
  DevBuf<int> out_nodes, out_tets;  // [n_part_nodes] caller ids | [4 n_elements] local ids
  DevBuf<double> out_xyz;           // [3 n_part_nodes]
};

struct PartsMesh {  // the handle's arrays a call works on (internal node order; the maps are null where the caller's order is the internal one)
  int n_nodes, n_tets;
  const int4* tets;
  double* x0;
  const double* q;
  const int* caller_of;
};

// Labels, node labels and the per-part table.  force_wide: two stable sort passes whatever the node count.  Two host waits (the number of
// parts; the counts at the end), a third where parts share nodes.
int parts_build(hipStream_t s, PartsWork& P, const PartsMesh& M, bool force_wide, PlanWorkspace& W);
// part_volume of the current rest positions (the build's last stage; again after a split)
int parts_volumes(hipStream_t s, PartsWork& P, const PartsMesh& M);
// CuttableMesh::splitParts on the rest positions: plane through c with unit normal n, shift = n * dist.  apply == false: everything but the
// store (the timing entry point).  out4: front, back and straddling parts, nodes moved.
int parts_split(hipStream_t s, PartsWork& P, const PartsMesh& M, const double c[3], const double n[3], const double shift[3], bool apply, int out4[4]);
// One part as a mesh into out_nodes / out_xyz / out_tets; its element ids are sorted[part_off[part] ..).  n_el, n_nd: its sizes
int parts_extract(hipStream_t s, PartsWork& P, const PartsMesh& M, int part, int* n_el, int* n_nd, int* first, PlanWorkspace& W);

}  // namespace fb
