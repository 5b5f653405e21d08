// PS::FEM::EmbeddedMesh: the mesh a host draws INSTEAD of the boundary triangles -- the marching-cubes surface of the BlobTree, an organ
// mesh -- bound to the tets of a HipIntegrator / Deformable and moved with them on the device, over fb_fem_embed / fb_fem_read_embedding /
// fb_fem_embed_update (fembrain_hip.h).  Header-only.  In the reference this is the receiver of Deformable::setDeformCallback with
// the weights of VolumetricMesh::generateInterpolationWeights (vegafem volumetricMesh.cpp:1059-1134); here the displacements never
// reach the host: what arrives per frame is positions, normals and box of the embedded points (24 bytes each).
//
// The binding follows Deformable::cut, syncForceModelDelta, syncForceModel and the removal of a detached part by itself (fembrain_hip.h,
// "Mesh changes"); the points and triangles of the drawn mesh never change.  Made by Deformable::embed, which owns it, or directly over an
// integrator that outlives it.
#pragma once
#include <vector>

#include "Deformable.h"

namespace PS {
namespace FEM {

class EmbeddedMesh {
 public:
  // xyz: 3 doubles per point in the rest frame; triangles: 3 point indices each (may be empty); zeroThreshold <= 0: off
  EmbeddedMesh(HipIntegrator* integrator, const std::vector<double>& xyz, const std::vector<int>& triangles, double zeroThreshold = 0.0)
      : m_lpIntegrator(integrator), m_id(-1), m_triangles(triangles) {
    fb_fem_embed_params prm;
    prm.zero_threshold = zeroThreshold;
    HipIntegrator::check(fb_fem_embed(integrator->handle(), (int)(xyz.size() / 3), xyz.data(), (int)(triangles.size() / 3), triangles.empty() ? nullptr : triangles.data(), &prm,
                                      &m_id, &m_info));
    m_xyz.assign((size_t)3 * m_info.n_points, 0.0f);
    m_normals.assign((size_t)3 * m_info.n_points, 0.0f);
  }
  ~EmbeddedMesh() {
    if (m_id >= 0) (void)fb_fem_embed_release(m_lpIntegrator->handle(), m_id);
  }
  EmbeddedMesh(const EmbeddedMesh&) = delete;
  EmbeddedMesh& operator=(const EmbeddedMesh&) = delete;

  int id() const { return m_id; }
  U32 countVertices() const { return (U32)m_info.n_points; }
  U32 countTriangles() const { return (U32)m_info.n_triangles; }
  U32 countExternal() const { return (U32)m_info.n_external; }  // points no element contained when they were last searched
  const fb_fem_embed_info& info() const { return m_info; }
  const std::vector<int>& triangles() const { return m_triangles; }

  // what the deformation callback's receiver did: the current positions, normals and box of the points
  void applyDisplacements() { HipIntegrator::check(fb_fem_embed_update(m_lpIntegrator->handle(), m_id, m_xyz.data(), m_normals.data(), &m_info)); }
  vec3d vertexAt(U32 idx) const { return vec3d(m_xyz[3 * idx], m_xyz[3 * idx + 1], m_xyz[3 * idx + 2]); }
  vec3d normalAt(U32 idx) const { return vec3d(m_normals[3 * idx], m_normals[3 * idx + 1], m_normals[3 * idx + 2]); }
  const std::vector<float>& positions() const { return m_xyz; }
  const std::vector<float>& normals() const { return m_normals; }
  vec3d aabbLower() const { return vec3d(m_info.aabb_lo[0], m_info.aabb_lo[1], m_info.aabb_lo[2]); }
  vec3d aabbUpper() const { return vec3d(m_info.aabb_hi[0], m_info.aabb_hi[1], m_info.aabb_hi[2]); }

  // the binding as the device holds it now: per point its element, 4 node ids (the caller's), 4 weights, its place in the rest shape
  void readBinding(std::vector<int>& elements, std::vector<int>& vertices4, std::vector<double>& weights4, std::vector<double>& restXYZ) {
    const size_t n = (size_t)m_info.n_points;
    elements.assign(n, 0); vertices4.assign(4 * n, 0); weights4.assign(4 * n, 0.0); restXYZ.assign(3 * n, 0.0);
    HipIntegrator::check(fb_fem_read_embedding(m_lpIntegrator->handle(), m_id, elements.data(), vertices4.data(), weights4.data(), restXYZ.data()));
  }

 private:
  HipIntegrator* m_lpIntegrator;  // not owned
  int m_id;
  fb_fem_embed_info m_info;
  std::vector<int> m_triangles;
  std::vector<float> m_xyz, m_normals;
};

// the members of Deformable that need the class above (Deformable.h declares them)
inline EmbeddedMesh* Deformable::embed(const std::vector<double>& xyz, const std::vector<int>& triangles, double zeroThreshold) {
  if (!m_lpIntegrator) syncForceModel();
  m_vEmbedded.push_back(new EmbeddedMesh(m_lpIntegrator, xyz, triangles, zeroThreshold));
  return m_vEmbedded.back();
}
inline void Deformable::releaseEmbedded() {
  for (size_t i = 0; i < m_vEmbedded.size(); i++) delete m_vEmbedded[i];
  m_vEmbedded.clear();
}

}  // namespace FEM
}  // namespace PS
