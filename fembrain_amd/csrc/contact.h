// The probe's box contact on the device (contact.hip): fb_fem_contact_move / _info_get / _reset / fb_fem_read_contact / fb_fem_contact_apply.
// What AvatarProbe::onTranslate (src/deformable/AvatarProbe.cpp:124-265) decides on the host of the reference below its pick-mode branch,
// and Deformable::applyHapticForces (src/deformable/Deformable.cpp:634-706) on the list it stores, for any number of sources.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace fb {

// records (target, source rank, ring) one apply may emit before it falls back to the level arrays of haptic.hip; FEMBRAIN_CONTACT_MAX_RECORDS=n
// (read at every apply) sets another budget for the tests
constexpr long long kContactMaxRecords = 1LL << 24;
// the walk's visited table of one source, in LDS: slots (open addressing), nodes a ball may hold, probes an insertion may take
constexpr int kContactTableSlots = 2048;
constexpr int kContactBallMax = 1024;
constexpr int kContactProbes = 32;

// Everything the contact session of one handle owns, in the CALLER's numbering.  Nothing is allocated before the first move; the touched set
// and the list survive every change of the mesh but a full re-sync (contact_mesh_changed).
struct ContactWork {
  // ---- the session ----
  int n_state = 0;                  // nodes the two arrays below cover (a cut appends nodes: grown, the new ones untouched)
  DevBuf<unsigned char> touched;    // [n_state] 1: in the set
  DevBuf<double> first;             // [3 n_state] position at first touch
  DevBuf<int> ids;                  // [n_state] the list: touched ids ascending, info.list_size in use
  DevBuf<double> forces;            // [3 n_state] ... and their forces
  fb_fem_contact_info info = {0, 0, 0, -1, -1, 0, 0, 0, 0.0, {0.0, 0.0, 0.0}};  // the host's mirror, what fb_fem_contact_info_get returns
  // ---- a move's scratch ----
  DevBuf<float> box_part, box6;     // the tissue's float box: per-workgroup partials | lo[3], hi[3]
  DevBuf<int> cnt, off;             // per workgroup: touched, new | touched before it; off[workgroups] the total, off[workgroups + 1] the new ones
  DevBuf<double> part_d;            // per-workgroup minima of d ...
  DevBuf<long long> part_k;         // ... and their keys 8 node + face
  DevBuf<int> push_cnt;             // per workgroup: forces greater than zero
  DevBuf<fb_fem_contact_info> res;  // what comes back, one copy
  // ---- an apply's ----
  bool pat_valid = false;           // host-built plan: pat_ptr / pat_col hold the current mesh's pattern (uploaded once per mesh generation)
  DevBuf<int> pat_ptr, pat_col;
  DevBuf<unsigned long long> keys, keys_sorted;   // records: target << rank bits | source rank (grow-only)
  DevBuf<unsigned char> rings, rings_sorted;      // ... and their rings
  DevBuf<char> temp;                // the sort's
  DevBuf<unsigned long long> walk;  // [0] records emitted (the cursor), [1] a ball overflowed its table, [2] target segments
  DevBuf<double> mag;               // [256] fall-off of ring j for the size of mag_size
  int mag_size = 0;
  ContactWork() = default;
  ContactWork(const ContactWork&) = delete;
  ContactWork& operator=(const ContactWork&) = delete;
};

// A new mesh generation (begin_mesh_generation): the uploaded pattern goes stale; in_place (fb_fem_resync_delta, fb_fem_cut: ids stay valid) keeps
// the session, a full re-sync clears it and counts that
void contact_mesh_changed(ContactWork& C, bool in_place);

}  // namespace fb
