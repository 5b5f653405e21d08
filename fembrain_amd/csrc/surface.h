// Boundary surface of the handle's tet mesh on the device (surface.hip): fb_fem_surface / fb_fem_read_surface / fb_fem_surface_update.
// What SurfaceMesh::setupFromTetMesh (src/deformable/SurfaceMesh.cpp:141-213), applyDisplacements + updateAABB (:338-373) and
// VolMeshRender::sync (src/deformable/VolMeshRender.cpp:74-112) compute on the host of the reference.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.h"
#include "plan_device.h"

namespace fb {

// Everything the surface of one handle owns.  Nothing is allocated before the first build.
struct SurfaceWork {
  bool valid = false;      // the topology below belongs to the handle's current mesh
  int n_builds = 0;
  int n_faces = 0, n_vertices = 0;
  int n_nodes = 0;         // nodes of the mesh it was built on
  bool wide = false;       // the last build took the two-pass (wide key) path
  float rest_box[6] = {0, 0, 0, 0, 0, 0};  // lo[3], hi[3] of the surface vertices' rest positions
  DevBuf<unsigned char> flag;       // [4 n_tets] the sorted entry is the last of a run of odd length
  DevBuf<uint32_t> csort;           // wide path: largest id of every sorted entry
  DevBuf<uint32_t> sel;             // [n_faces] payloads of the surviving faces in output order
  DevBuf<int> counts;               // [0] faces, [1] vertices
  DevBuf<int> faces, faces_int;     // [3 n_faces] node ids: the caller's | the handle's internal order (what the update gathers through)
  DevBuf<int> face_tets;            // [n_faces]
  DevBuf<unsigned int> bitmap;      // a bit per node (caller id): some face uses it
  DevBuf<int> word_cnt, word_off;   // [words + 1] bits of every bitmap word | surface vertices before it
  DevBuf<int> vertex_ids, vnode;    // [n_vertices] ascending caller ids | internal id of each
  DevBuf<uint32_t> inc;             // [3 n_faces] 3 * face + corner, grouped by surface vertex, faces ascending inside a group
  DevBuf<int> inc_off;              // [n_vertices + 1]
  DevBuf<float> out;                // [6 n_vertices + 6] xyz, normals, box of the last update
  DevBuf<float> part;               // per-workgroup boxes
  std::vector<float> host;          // staging of `out`
};

// payload of a face: bit 31 the element's determinant is negative, bits 2..29 the element, bits 0..1 the local face
constexpr uint32_t kFaceNeg = 0x80000000u;

// Topology of the boundary.  tets / x0: the handle's element list and fp64 rest positions in its internal order; caller_of / internal_of:
// the renumbering's maps (null: the caller's order is the internal one).  force_wide: two stable passes whatever the node count.
// Two host waits: the face count, and at the end the vertex count with the rest box.
int surface_build(hipStream_t s, SurfaceWork& S, int n_nodes, int n_tets, const int4* tets, const double* x0, const int* caller_of, const int* internal_of,
                  bool force_wide, PlanWorkspace& W);

// Positions (float)(x0 + q), normals and box of the surface vertices into S.out; copy_out: one copy of all three into S.host.
int surface_update(hipStream_t s, SurfaceWork& S, const double* x0, const double* q, bool copy_out);

}  // namespace fb
