// PS::FEM::AvatarProbe <-> class AvatarProbe (reference src/deformable/AvatarProbe.h, AvatarProbe.cpp): what the reference's probe does
// below the scene graph.  The box mesh, its transform, the mouse and the header lines stay with the host application, which hands the
// tool's box in world coordinates to onTranslate; the touched-vertex hash, the contact face and the penalty forces live on the device
// in the tissue's handle (fb_fem_contact_move), and Deformable::timestep spreads the list (fb_fem_contact_apply).  Header-only.
#pragma once
#include "Deformable.h"

namespace PS {
namespace FEM {

class AvatarProbe {
 public:
  enum Face { LEFT = 0, RIGHT = 1, BOTTOM = 2, TOP = 3, NEAR = 4, FAR = 5 };

  AvatarProbe() { init(); }
  explicit AvatarProbe(Deformable* tissue) { init(); setTissue(tissue); }

  // A probe is new to its tissue: no touched vertices, no contact face (the reference sets its face to -1 in the constructor only)
  void setTissue(Deformable* tissue) {
    m_lpTissue = tissue;
    if (m_lpTissue && m_lpTissue->integrator()) m_lpTissue->integrator()->ContactReset(false);
    m_last = fb_fem_contact_info();
    m_last.face = -1; m_last.closest_node = -1;
  }
  Deformable* tissue() const { return m_lpTissue; }

  // AvatarProbe::mousePress, button down without pick mode (AvatarProbe.cpp:108-109)
  void start() {
    if (m_lpTissue && !m_lpTissue->isHapticInProgress()) m_lpTissue->probeStart();
  }
  // ... button up (AvatarProbe.cpp:114-120): the hash is cleared, the face stays
  void end() {
    if (m_lpTissue && m_lpTissue->isHapticInProgress()) m_lpTissue->probeEnd();
  }
  // AvatarProbe::onTranslate (AvatarProbe.cpp:124-265) below its pick-mode branch, with the tool's box in world coordinates.  Returns the
  // move's status (FB_CONTACT_MISS / EMPTY / SET); nothing happens while no probing is in progress.
  int onTranslate(const vec3d& lower, const vec3d& upper) {
    if (m_lpTissue == nullptr || !m_lpTissue->isHapticInProgress()) return FB_CONTACT_MISS;
    m_last = m_lpTissue->probeMove(lower, upper, m_hapticForceCoeff);
    return m_last.status;
  }

  int contactFace() const { return m_last.face; }
  double contactDist() const { return m_last.contact_dist; }
  vec3d closestPoint() const { return vec3d(m_last.closest_point[0], m_last.closest_point[1], m_last.closest_point[2]); }
  int closestVertex() const { return m_last.closest_node; }
  int countTouched() const { return m_last.n_touched; }
  const fb_fem_contact_info& lastContact() const { return m_last; }
  double forceCoeff() const { return m_hapticForceCoeff; }
  void setForceCoeff(double coeff) { m_hapticForceCoeff = coeff; }
  static const char* faceName(int face) {
    static const char* names[6] = {"LEFT", "RIGHT", "BOTTOM", "TOP", "NEAR", "FAR"};
    return face >= 0 && face < 6 ? names[face] : "NONE";
  }

 private:
  void init() {
    m_lpTissue = nullptr;
    m_hapticForceCoeff = 200000.0;  // DEFAULT_HAPTIC_FORCE_COEFF, AvatarProbe.cpp:11
    m_last = fb_fem_contact_info();
    m_last.face = -1; m_last.closest_node = -1;
  }
  Deformable* m_lpTissue;
  double m_hapticForceCoeff;
  fb_fem_contact_info m_last;
};

}  // namespace FEM
}  // namespace PS
