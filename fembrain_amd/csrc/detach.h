// A part of the cut mesh detached into a handle of its own on the device (detach.hip): fb_fem_detach_part, and the constrained-DOF list
// of a handle (fb_fem_num_constrained_dofs / fb_fem_read_constrained_dofs).  What CuttableMesh::convertDisjointPartsToMeshes
// (src/deformable/CuttableMesh.cpp:628-698) does with a part on the host of the reference: a mesh object of its own, its cells erased
// from the original.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "plan_device.h"

namespace fb {

// The scratch of a parent's detach calls (its own stream).  Nothing is allocated before the first call.
struct DetachWork {
  DevBuf<unsigned char> dof_flag;  // [3 n_part_nodes] the parent constrains the DOF of the part's local node
  DevBuf<int> dof_list;            // [3 n_part_nodes] the flagged local DOFs, ascending
  DevBuf<int> count;               // their number
};

// The node maps between two handles (device pointers; a null map: that handle works in the caller's order).  Piece internal id ->
// the part's local id (piece_local_of) -> the parent's caller id (part_nodes = PartsWork::out_nodes) -> the parent's internal id
// (parent_internal_of).
struct DetachMaps {
  int n_nodes;                    // of the piece
  const int* piece_local_of;      // the piece's old_of_new
  const int* part_nodes;
  const int* parent_internal_of;  // the parent's new_of_old
};

// dst[v][3 i + a] = src[v][3 parent(i) + a] for the n_vec vectors (q, qvel, fext, qacc), one launch
int detach_gather_state(hipStream_t s, const DetachMaps& M, int n_vec, const double* const src[4], double* const dst[4]);
// out[j] = bytes[element_ids[j]] (the material ids of the part's elements)
int detach_gather_bytes(hipStream_t s, int n_el, const uint32_t* element_ids, const unsigned char* bytes, unsigned char* out);
// The constrained DOFs of the part in its local ids, ascending, from the parent's DOF mask (0 = constrained, internal order): flags, a
// select, one download of the count and one of the list.  One host wait each.
int detach_fixed_dofs(hipStream_t s, DetachWork& D, int n_nd, const int* part_nodes, const int* parent_internal_of, const unsigned char* dofmask, PlanWorkspace& W,
                      std::vector<int>* out);

}  // namespace fb
