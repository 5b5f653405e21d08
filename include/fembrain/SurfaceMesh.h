// PS::FEM::SurfaceMesh <-> class SurfaceMesh (reference src/deformable/SurfaceMesh.h:24-110): the boundary triangles of the tet mesh a
// HipIntegrator / Deformable simulates and cuts, with the reference's accessor names, over fb_fem_surface / fb_fem_read_surface /
// fb_fem_surface_update (fembrain_hip.h).  Header-only.  draw() stays in the host application: it fills its vertex buffer from
// vertexAt / normalAt and its index buffer from faceCompactAt.
//
// Where it differs from the reference: the reference keeps EVERY tet vertex in the surface mesh (SurfaceMesh.cpp:147-148) and copies all
// of u to it after every step (:338-352); here the host holds the surface vertices only -- countVertices() of them, in ascending node id,
// vertexIdAt(i) naming the node.  faceAt(f) returns node ids exactly as the reference's m_faces do; faceCompactAt(f) the same face as
// indices into the vertex list.  After Deformable::cut (or any re-sync) the next access re-reads the topology from the device.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "Deformable.h"

namespace PS {
namespace FEM {

struct vec3u32 {
  U32 x, y, z;
  vec3u32(U32 x_ = 0, U32 y_ = 0, U32 z_ = 0) : x(x_), y(y_), z(z_) {}
};

class SurfaceMesh {
 public:
  explicit SurfaceMesh(HipIntegrator* integrator) : m_lpIntegrator(integrator), m_builds(-1), m_stale(true) {}
  explicit SurfaceMesh(const Deformable& d) : m_lpIntegrator(d.getIntegrator()), m_builds(-1), m_stale(true) {}

  // the topology may have changed (Deformable::cut and syncForceModel call it); applyDisplacements notices a change by itself
  void invalidate() { m_stale = true; }

  U32 countVertices() { sync(); return (U32)m_ids.size(); }
  U32 countFaceElements() { sync(); return (U32)(m_faces.size() / 3); }
  vec3u32 faceAt(U32 idx) { sync(); return vec3u32((U32)m_faces[3 * idx], (U32)m_faces[3 * idx + 1], (U32)m_faces[3 * idx + 2]); }
  vec3u32 faceCompactAt(U32 idx) { sync(); return vec3u32((U32)m_compact[3 * idx], (U32)m_compact[3 * idx + 1], (U32)m_compact[3 * idx + 2]); }
  U32 faceElementAt(U32 idx) { sync(); return (U32)m_faceTets[idx]; }  // the element the face belongs to (not in the reference)
  U32 vertexIdAt(U32 idx) { sync(); return (U32)m_ids[idx]; }
  vec3d vertexAt(U32 idx) { sync(); return vec3d(m_xyz[3 * idx], m_xyz[3 * idx + 1], m_xyz[3 * idx + 2]); }
  vec3d normalAt(U32 idx) { sync(); return vec3d(m_normals[3 * idx], m_normals[3 * idx + 1], m_normals[3 * idx + 2]); }
  vec3d faceVertexAt(U32 idxFace, unsigned char idxWhichCorner) { sync(); return vertexAt((U32)m_compact[3 * idxFace + idxWhichCorner]); }
  const std::vector<float>& positions() { sync(); return m_xyz; }
  const std::vector<float>& normals() { sync(); return m_normals; }
  const std::vector<int>& faces() { sync(); return m_faces; }
  const std::vector<int>& vertexIds() { sync(); return m_ids; }

  // SurfaceMesh::applyDisplacements (SurfaceMesh.cpp:338-352) + VolMeshRender::sync's normals (VolMeshRender.cpp:74-112): the reference is
  // handed u by the deformation callback; here the state is on the device, and what arrives is positions, normals and box of the surface
  // vertices (24 bytes each)
  void applyDisplacements() {
    fb_fem_surface_info info;
    HipIntegrator::check(fb_fem_surface(m_lpIntegrator->handle(), &info));
    if (m_stale || info.n_builds != m_builds) readTopology(info);
    if (m_ids.empty()) return;
    HipIntegrator::check(fb_fem_surface_update(m_lpIntegrator->handle(), m_xyz.data(), m_normals.data(), &info));
    setBox(info);
  }
  // The scalar to draw on the vertices: mean von Mises stress behind each vertex's faces (fb_fem_surface_stress), from the last
  // HipIntegrator::ComputeStress / Deformable::computeStress of the current mesh; throws where there is none.  vertexStressAt(i) goes
  // with vertexAt(i).
  const std::vector<float>& applyStress() {
    sync();
    m_lpIntegrator->SurfaceStress(m_stress);
    return m_stress;
  }
  float vertexStressAt(U32 idx) const { return m_stress[idx]; }
  const std::vector<float>& vertexStress() const { return m_stress; }
  void updateAABB() { applyDisplacements(); }  // (SurfaceMesh.cpp:354-373: the box travels with the positions)
  vec3d aabbLower() { sync(); return m_lo; }
  vec3d aabbUpper() { sync(); return m_hi; }

  // SurfaceMesh::findClosestVertex (SurfaceMesh.cpp:300-320) over the surface vertices of the host copy: returns the NODE id, -1 on an
  // empty mesh
  int findClosestVertex(const vec3d& query, double& dist, vec3d& outP) {
    sync();
    int best = -1;
    double bd = 0.0;
    for (size_t i = 0; i < m_ids.size(); i++) {
      const double dx = m_xyz[3 * i] - query.x, dy = m_xyz[3 * i + 1] - query.y, dz = m_xyz[3 * i + 2] - query.z;
      const double d2 = dx * dx + dy * dy + dz * dz;
      if (best < 0 || d2 < bd) { best = (int)i; bd = d2; }
    }
    if (best < 0) return -1;
    dist = std::sqrt(bd);
    outP = vertexAt((U32)best);
    return m_ids[(size_t)best];
  }

 private:
  void sync() {
    if (m_stale) applyDisplacements();
  }
  void readTopology(const fb_fem_surface_info& info) {
    m_faces.assign((size_t)3 * info.n_faces, 0);
    m_faceTets.assign((size_t)info.n_faces, 0);
    m_ids.assign((size_t)info.n_vertices, 0);
    HipIntegrator::check(fb_fem_read_surface(m_lpIntegrator->handle(), m_faces.data(), m_ids.data(), m_faceTets.data()));
    m_compact.resize(m_faces.size());
    for (size_t k = 0; k < m_faces.size(); k++) m_compact[k] = (int)(std::lower_bound(m_ids.begin(), m_ids.end(), m_faces[k]) - m_ids.begin());
    m_xyz.assign((size_t)3 * info.n_vertices, 0.0f);
    m_normals.assign((size_t)3 * info.n_vertices, 0.0f);
    m_builds = info.n_builds;
    m_stale = false;
    setBox(info);
  }
  void setBox(const fb_fem_surface_info& info) {
    m_lo = vec3d(info.aabb_lo[0], info.aabb_lo[1], info.aabb_lo[2]);
    m_hi = vec3d(info.aabb_hi[0], info.aabb_hi[1], info.aabb_hi[2]);
  }
  HipIntegrator* m_lpIntegrator;  // not owned
  int m_builds;
  bool m_stale;
  std::vector<int> m_faces, m_compact, m_faceTets, m_ids;
  std::vector<float> m_xyz, m_normals, m_stress;
  vec3d m_lo, m_hi;
};

// the members of Deformable that need the class above (Deformable.h declares them)
inline Deformable::~Deformable() {
  releaseEmbedded();
  delete m_lpSurface;
  delete m_lpIntegrator;
}
inline SurfaceMesh* Deformable::surfaceMesh() {
  if (!m_lpSurface) m_lpSurface = new SurfaceMesh(m_lpIntegrator);
  return m_lpSurface;
}
inline void Deformable::surfaceChanged() {
  if (m_lpSurface) m_lpSurface->invalidate();
}

}  // namespace FEM
}  // namespace PS
