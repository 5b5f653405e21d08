// Penalty contact between two handles on one device (body_contact.hip): fb_fem_body_contact / fb_fem_read_body_contact /
// fb_fem_time_body_contact.  What Deformable::setCollisionObject / collisionDetect hand to CollisionDetection (Bullet) in the reference:
// here the surface vertices of one body against the elements and the boundary faces of the other, both at their current states.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.h"

namespace fb {

// One contact as the closest-face kernel and the force pass leave it, and as it comes back to the host in one copy per direction
struct BodyContactRec {
  double c[3];        // the closest point on the other body's boundary
  double b[3];        // its weights on the face's corners: b0 = 1 - b1 - b2
  double d;           // |c - p|
  double f[3];        // the force on the point's node (zero: degenerate)
  long long tested;   // faces this point's search tested
  int node, elem, face;  // the point's node, the containing element and the closest face: caller ids / the orders of fb_fem_read_mesh and fb_fem_read_surface
  int far;            // the search through the grid gave the point up at its budget
};

// What the friction calls keep per contact beside its BodyContactRec (contact_friction.hip.h): only their force kernels write it
struct ContactFrictionRec {
  double N;      // the normal force after damping, never negative
  double s;      // |t|
  double t[3];   // the tangential velocity of the point relative to the face
  double mf[3];  // -f, the friction on the point's node
};

// What both contact units keep for the closest-face search and the force stage (face_search.hip.h, contact_force.hip.h)
struct FaceSearchWork {
  hipEvent_t ev_t[2] = {nullptr, nullptr};  // fb_fem_time_*_contact's stages
  DevBuf<int> f_cnt, f_start, f_face;  // the face grid: faces per cell, prefix sums, faces by cell
  DevBuf<double> f_tri;              // [9][faces] their current coordinates in that order, a plane per coordinate
  DevBuf<double> f_R;                // per-workgroup partials of the largest centroid-to-vertex distance; the padded maximum in the last
  DevBuf<BodyContactRec> rec;        // [contacts]
  DevBuf<uint32_t> r_key, r_key_s, r_val, r_val_s;  // the records (node | records-per-contact contact + record), before and after the sort
  DevBuf<ContactFrictionRec> fric;   // [contacts] the friction calls only
  ~FaceSearchWork() {
    for (auto& e : ev_t) if (e) (void)hipEventDestroy(e);
  }
};

// The working state of the calls, kept in handle `a`.  Nothing is allocated before the first call; everything grows only.
struct BodyContactWork {
  hipEvent_t ev_in = nullptr, ev_out = nullptr;  // the other handle's stream -> this one's, and back
  // current positions and boxes: [0] of this handle, [1] of the other
  DevBuf<double> cur[2];
  DevBuf<double> box_part;   // per-workgroup boxes of the running fold
  DevBuf<double> boxes;      // [24] nodes of a | surface of a | nodes of b | surface of b
  // per direction, reused by the second
  DevBuf<unsigned char> flag;        // a flag per surface vertex, element or candidate of the running selection
  DevBuf<int> cand, hit, sel, counts;  // candidates (surface-vertex ranks) | contacts (candidate ranks) | binned elements | the selections' lengths
  DevBuf<int> t_cnt, t_off, cell_lo, cell_hi, cell_elem;  // the element grid: cells per binned element, prefix sums, runs per cell, elements by cell
  DevBuf<int> c_elem;                // [candidates] the containing element or -1
  FaceSearchWork fs;                 // the face grid, the contacts and the other side's records (node | 3 contact + corner)
  DevBuf<double> scratch[2];         // fb_fem_time_body_contact: what the scatter adds into instead of the force vectors
  // the last call, per direction
  std::vector<BodyContactRec> host[2];
  fb_fem_body_contact_info info = {};
  std::vector<ContactFrictionRec> fric_host[2];  // the last friction call, per direction
  ~BodyContactWork() {
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
  }
};

}  // namespace fb
