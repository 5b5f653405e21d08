// Penalty contact of a handle with itself (self_contact.hip): fb_fem_self_contact / fb_fem_read_self_contact / fb_fem_time_self_contact.
// The lips of a cut, or a body folded onto itself: the surface vertices of the handle against its own elements and boundary faces, those
// of the point's own node (FB_SELF_CONTACT_ANY) or part (FB_SELF_CONTACT_OTHER_PARTS) excluded.  The reference has no counterpart.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "body_contact.h"
#include "common.h"

namespace fb {

// The working state of the calls.  Nothing is allocated before the first call; everything grows only and is sized again at every call
// from the surface of that call (a cut, a delta or a re-sync changes the surface; no count is carried from one mesh generation to the
// next except `ident_n`, which says how much of `ident` is filled and does not depend on the mesh).
struct SelfContactWork {
  DevBuf<double> cur;         // [3 nodes] x0 + q, internal order
  DevBuf<double> box_part;    // per-workgroup boxes of the running fold
  DevBuf<double> boxes;       // [6] the nodes' box (infinite where a position is not finite)
  // the grid of surface vertices
  DevBuf<int> p_key;          // [surface vertices] what the exclusion compares: the internal node (ANY) | the part (OTHER_PARTS)
  DevBuf<uint32_t> p_cell, p_cell_s, p_v, p_v_s;  // (cell, surface vertex) before and after the sort
  DevBuf<int> cell_lo, cell_hi;  // runs per cell
  DevBuf<double> p_xyz;       // [3][surface vertices] positions in sorted order, a plane per coordinate
  DevBuf<int> p_key_s;        // [surface vertices] p_key in sorted order
  DevBuf<int> slot;           // [surface vertices] the lowest containing element, INT_MAX for none
  DevBuf<unsigned char> flag; // [max(elements, surface vertices)] element is wide | vertex is in contact
  DevBuf<int> wide;           // [elements] the overflow list
  DevBuf<int> counts;         // [0] wide elements, [1] contacts
  DevBuf<int> ident;          // [surface vertices] 0, 1, 2, ...: the searches' candidate list (every surface vertex is one)
  size_t ident_n = 0;
  DevBuf<int> hit;            // [contacts] surface vertices in contact, ascending
  // the closest faces
  DevBuf<int> face_part;      // [faces] OTHER_PARTS: the part of the face's element
  FaceSearchWork fs;          // the face grid, the contacts and their records (node | 4 contact + record)
  DevBuf<double> scratch;     // fb_fem_time_self_contact: what the scatter adds into instead of the force vector
  // the last adding call
  std::vector<BodyContactRec> host;
  fb_fem_self_contact_info info = {};
  std::vector<ContactFrictionRec> fric_host;  // the last friction call
};

}  // namespace fb
