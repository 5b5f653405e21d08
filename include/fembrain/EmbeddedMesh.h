// PS::FEM::EmbeddedMesh: the mesh a host draws INSTEAD of the boundary triangles -- the marching-cubes surface of the BlobTree, an organ
// mesh -- bound to the tets of a HipIntegrator / Deformable and moved with them on the device, over fb_fem_embed / fb_fem_read_embedding /
// fb_fem_embed_update (fembrain_hip.h).  Header-only.  In the reference this is the receiver of Deformable::setDeformCallback with
// the weights of VolumetricMesh::generateInterpolationWeights (vegafem volumetricMesh.cpp:1059-1134); here the displacements never
// reach the host: what arrives per frame is positions, normals and box of the embedded points (24 bytes each).
//
// The binding follows Deformable::cut, syncForceModelDelta, syncForceModel and the removal of a detached part by itself (fembrain_hip.h,
// "Mesh changes"); the points and triangles of the drawn mesh never change.  Made by Deformable::embed, which owns it, or directly over an
// integrator that outlives it.
//
// The way back runs on the device too (fb_fem_embed_add_forces / fb_fem_embed_pick_ray / fb_fem_embed_pick_point / fb_fem_embed_stress):
// addForces pushes on drawn points, pickRay / pickPoint click on the drawn mesh, touch does both, applyStress colours it.  The reference
// has none of these: its probe talks to nodes and its drawn surface only receives.
#pragma once
#include <limits>
#include <stdexcept>
#include <utility>
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
  // how the points no element contains found their closest centre in the last search (fb_fem_embed_search_info_get): a surface drawn
  // around the body has most of its points there
  fb_fem_embed_search_info searchInfo() const {
    fb_fem_embed_search_info si;
    HipIntegrator::check(fb_fem_embed_search_info_get(m_lpIntegrator->handle(), m_id, &si));
    return si;
  }

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

  // ---- the way back: the drawn mesh touched, clicked and coloured (fb_fem_embed_add_forces / pick_ray / pick_point / embed_stress) ----
  // forces[s] on point pointIds[s] (strictly ascending), added to the external forces of the four nodes of the point's element by its
  // weights -- bit for bit the host loop over readBinding
  void addForces(const std::vector<int>& pointIds, const std::vector<vec3d>& forces) {
    if (pointIds.size() != forces.size()) throw std::invalid_argument("EmbeddedMesh::addForces: one force per point id");
    stage(forces);
    m_lpIntegrator->EmbedAddForces(m_id, (int)pointIds.size(), pointIds.data(), m_forceStage.data());
  }
  // ... one force on every point
  void addForces(const std::vector<vec3d>& forces) {
    if (forces.size() != (size_t)m_info.n_points) throw std::invalid_argument("EmbeddedMesh::addForces: one force per point");
    stage(forces);
    m_lpIntegrator->EmbedAddForces(m_id, (int)forces.size(), nullptr, m_forceStage.data());
  }
  // what a click on the drawn mesh finds
  struct RayHit {
    int triangle;  // -1: a miss
    double t, u, v;  // origin + t dir = (1-u-v) a + u b + v c
    vec3d point;
    RayHit() : triangle(-1), t(0.0), u(0.0), v(0.0) {}
  };
  // the nearest hit of the ray on the triangles at the current state; tMax < 0: unbounded
  RayHit pickRay(const vec3d& origin, const vec3d& dir, double tMax = -1.0) {
    const double o[3] = {origin.x, origin.y, origin.z}, d[3] = {dir.x, dir.y, dir.z};
    double bary[2] = {0.0, 0.0}, p[3] = {0.0, 0.0, 0.0};
    RayHit hit;
    hit.triangle = m_lpIntegrator->EmbedPickRay(m_id, o, d, tMax < 0.0 ? std::numeric_limits<double>::infinity() : tMax, &hit.t, bary, p);
    hit.u = bary[0]; hit.v = bary[1];
    hit.point = vec3d(p[0], p[1], p[2]);
    return hit;
  }
  // the point closest to wpos at the current state (of equal distances the lowest index), its fp64 position in `vertex`
  int pickPoint(const vec3d& wpos, vec3d& vertex) {
    const double w[3] = {wpos.x, wpos.y, wpos.z};
    double p[3] = {0.0, 0.0, 0.0};
    const int best = m_lpIntegrator->EmbedPickPoint(m_id, w, p);
    if (best >= 0) vertex = vec3d(p[0], p[1], p[2]);
    return best;
  }
  // a click that pulls: the ray's nearest hit, and `force` shared among the hit triangle's three points by (1-u-v, u, v)
  RayHit touch(const vec3d& origin, const vec3d& dir, const vec3d& force) {
    const RayHit hit = pickRay(origin, dir);
    if (hit.triangle < 0) return hit;
    const double share[3] = {1.0 - hit.u - hit.v, hit.u, hit.v};
    int order[3] = {0, 1, 2};
    const int* f = &m_triangles[3 * (size_t)hit.triangle];
    for (int a = 0; a < 3; a++)  // ascending point ids
      for (int b = a + 1; b < 3; b++)
        if (f[order[b]] < f[order[a]]) std::swap(order[a], order[b]);
    std::vector<int> ids(3);
    std::vector<vec3d> forces(3);
    for (int k = 0; k < 3; k++) {
      ids[k] = f[order[k]];
      forces[k] = vec3d(share[order[k]] * force.x, share[order[k]] * force.y, share[order[k]] * force.z);
    }
    addForces(ids, forces);
    return hit;
  }
  // the colour of the drawn mesh: per point the von Mises stress of its element, from the last Deformable::computeStress
  void applyStress() {
    m_stress.assign((size_t)m_info.n_points, 0.0f);
    m_lpIntegrator->EmbedStress(m_id, m_stress.data());
  }
  float stressAt(U32 idx) const { return m_stress[idx]; }
  const std::vector<float>& stress() const { return m_stress; }

 private:
  void stage(const std::vector<vec3d>& forces) {
    m_forceStage.resize(3 * forces.size());
    for (size_t i = 0; i < forces.size(); i++) { m_forceStage[3 * i] = forces[i].x; m_forceStage[3 * i + 1] = forces[i].y; m_forceStage[3 * i + 2] = forces[i].z; }
  }
  HipIntegrator* m_lpIntegrator;  // not owned
  int m_id;
  fb_fem_embed_info m_info;
  std::vector<int> m_triangles;
  std::vector<float> m_xyz, m_normals, m_stress;
  std::vector<double> m_forceStage;
};

// the members of Deformable that need the class above (Deformable.h declares them)
inline EmbeddedMesh* Deformable::embed(const std::vector<double>& xyz, const std::vector<int>& triangles, double zeroThreshold) {
  if (!m_lpIntegrator) syncForceModel();
  m_vEmbedded.push_back(new EmbeddedMesh(m_lpIntegrator, xyz, triangles, zeroThreshold));
  return m_vEmbedded.back();
}
inline int Deformable::touchEmbedded(EmbeddedMesh* mesh, const vec3d& origin, const vec3d& dir, const vec3d& force) {
  return mesh->touch(origin, dir, force).triangle;
}
inline void Deformable::releaseEmbedded() {
  for (size_t i = 0; i < m_vEmbedded.size(); i++) delete m_vEmbedded[i];
  m_vEmbedded.clear();
}

}  // namespace FEM
}  // namespace PS
