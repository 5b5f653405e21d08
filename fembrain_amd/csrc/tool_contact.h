// Penalty contact of a rigid tool with the tissue (tool_contact.hip): fb_fem_tool_contact / fb_fem_read_tool_contact /
// fb_fem_time_tool_contact.  The tool is a set of spheres, capsules and oriented boxes -- the shapes of fembrain_amd/erosion.py -- in the
// world frame; the points are the surface vertices of the handle or all of its nodes.  The reference has only the axis-aligned probe box
// (contact.hip); the rule is this project's (include/fembrain_hip.h, "Contact with a rigid tool").
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "body_contact.h"
#include "common.h"

namespace fb {

// One point held by the tool: as the first kernel leaves it per point (f unset) and as the second leaves it per contact
struct ToolContactRec {
  double p[3];      // x0 + q of the point
  double n[3];      // outward normal of the winning shape there (zero: degenerate)
  double depth;     // before the cap
  double f[3];      // the force added to the point's node (zero: degenerate)
  int node, nd;     // the point's node: caller id | internal id
  int shape;        // the winning shape
  int degenerate;   // the point sits on the centre of the winning sphere or on the capsule's segment: no normal, nothing pushed
};

// The working state of the calls.  Nothing is allocated before the first call; everything grows only and is sized again at every call
// from the points of that call.
struct ToolContactWork {
  hipEvent_t ev_t[2] = {nullptr, nullptr};  // fb_fem_time_tool_contact's stages
  DevBuf<ToolContactRec> dense;      // [points]
  DevBuf<unsigned char> flag;        // [points] some shape holds the point
  DevBuf<int> hit;                   // [contacts] the points in contact, ascending
  DevBuf<int> counts;                // [0] contacts, [1] a position that is not finite, [2] a velocity that is not finite
  DevBuf<ToolContactRec> rec;        // [contacts]
  DevBuf<ContactFrictionRec> fric;   // [contacts] the calls with friction only
  DevBuf<double> scratch;            // fb_fem_time_tool_contact: what the second kernel adds into instead of the force vector
  // the last adding call
  std::vector<ToolContactRec> host;
  std::vector<ContactFrictionRec> fric_host;  // (empty: that call was frictionless)
  ~ToolContactWork() {
    for (auto& e : ev_t)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace fb
