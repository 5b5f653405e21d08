// Constrained DOFs that move (motion.hip): fb_fem_set_constrained_motion / fb_fem_read_reactions / fb_fem_grasp and what goes with them.
// A subset of the handle's constrained DOFs follows targets: the free rows get the columns the stored matrix does not hold as a
// right-hand-side correction formed from the elements, and the force the constraint puts on the body is read back ("Constrained
// motion" in include/fembrain_hip.h).  The reference has only IAvatar::grip()'s flag.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"

struct fb_fem_s;

namespace fb {

// The working state.  Nothing is allocated before the first fb_fem_set_constrained_motion / fb_fem_grasp with a non-empty set;
// everything grows only.  The set lives on the host in the caller's ids (what survives a re-sync that renumbers), the targets on the
// device in the set's order.
struct MotionWork {
  // ---- the set ----
  std::vector<int> dofs;        // caller ids, ascending, each a constrained DOF
  DevBuf<double> target;        // [n] u_c
  DevBuf<double> vstar, dvc;    // [n] the velocity the step ends with, and dv_c = v* - qvel_c (k_motion_dv)
  DevBuf<double> react;         // [n + 3] lambda of the last step, then its sum by axis
  DevBuf<double> react_t;       // fb_fem_time_motion writes here instead
  DevBuf<int> err;              // [1] k_motion_dv met a target or a state that is not finite
  bool react_valid = false;     // a step has run with this set
  // ---- the table, per (set, mesh generation) ----
  bool table_valid = false;
  int table_builds = 0;
  int n_listed = 0, n_touched = 0, longest_run = 0;
  DevBuf<int> dofs_dev;         // [n] the set's caller ids, then
  DevBuf<int> dof;              // [n] internal DOF of every entry
  DevBuf<int> dof_slot;         // [3 nodes] entry of the set at an internal DOF, -1: none
  DevBuf<unsigned char> flag;   // [max(elements, records)] element is listed | record opens a node's run
  DevBuf<int> listed;           // [n_listed] elements with a node that has a DOF in the set, ascending
  DevBuf<int> esel;             // [12 n_listed] dof_slot at the DOFs of the listed elements' corners (record 4p + k: 3 entries)
  DevBuf<uint32_t> key, key_s, val, val_s;  // records (internal node | 4p + k) before and after the stable sort by node
  DevBuf<int> heads;            // [n_touched] first sorted record of every touched node
  DevBuf<int> counts;           // [0] listed elements, [1] touched nodes, [2] longest run
  DevBuf<double> y;             // [4 n_listed][3] what the element kernel leaves for the gather
  // ---- the grasp ----
  std::vector<int> grasp_nodes;      // caller node ids, ascending
  std::vector<int> grasp_added;      // the DOFs fb_fem_grasp added to the constrained list (fb_fem_release takes them out again)
  std::vector<int> grasp_set_added;  // ... and to the set
  DevBuf<int> grasp_nodes_dev;       // [nodes]
  DevBuf<int> grasp_slot;            // [3 nodes] entry of the set at every DOF of the grasp, -1: dropped since
  DevBuf<double> grasp_pos;          // [3 nodes] world positions at the grasp
  bool grasp_slots_valid = false;    // grasp_slot belongs to the current set
  hipEvent_t ev_t[2] = {nullptr, nullptr};  // fb_fem_time_motion's stages
  ~MotionWork() {
    for (auto& e : ev_t) if (e) (void)hipEventDestroy(e);
  }
};

// fem.hip's step and fb_fem_system ask these three, and only where motion_active(): a handle with an empty set launches nothing new
int motion_correct_rhs(fb_fem_s* h);   // after assemble_system: v*, dv_c, rhs_f -= Keff_fc dv_c
int motion_reactions(fb_fem_s* h);     // after the solve, before the state update: lambda and its sum
int motion_apply(fb_fem_s* h);         // after the state update: q_c = u_c, qvel_c = v*_c; FB_EINVAL where k_motion_dv refused
// fem_build.hip
void motion_mesh_changed(MotionWork& W);   // begin_mesh_generation: the table goes stale (the set is filtered when it is built again)
void motion_clear(MotionWork& W);          // a state reset: the set and the grasp go
int motion_rest_absorbs_q(fb_fem_s* h);    // FB_CUT_BAKE, before x0 += q and q = 0: u_c -= q_c, a held node's world-space target stays (asked only where motion_active())
int motion_constraints_changed(fb_fem_s* h);  // the constrained list was replaced: entries whose DOF is no longer in it are dropped

}  // namespace fb
