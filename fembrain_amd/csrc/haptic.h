// The haptic probe on the device (haptic.hip): fb_fem_add_haptic_forces / fb_fem_pick_vertex / fb_fem_pick_box / fb_fem_volume.
// What Deformable::applyHapticForces (src/deformable/Deformable.cpp:634-706), pickVertex / pickVertices (:422-448) and computeVolume
// (:260-279) compute on the host of the reference.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"

namespace fb {

// sources whose rings are walked together: one byte per (source, node) of the level array
constexpr int kHapticBatch = 32;

// what fb_fem_pick_vertex brings back in one copy
struct PickResult {
  double dist2, xyz[3];
  int index, pad;
};

// Everything the probe of one handle owns.  Nothing is allocated before the first call of the entry point that uses it; the
// allocations are kept (grow-only) and filled again by every call, so nothing here can go stale with the mesh.
struct HapticWork {
  // spread
  DevBuf<unsigned char> level;    // [min(n, kHapticBatch)][n_nodes] ring of every node per source of the batch, internal order; 0xFF: not reached
  DevBuf<unsigned char> args;     // one upload per call: forces3[3 n] | mag[size] | ids[n]
  unsigned char* args_pinned = nullptr;  // its pinned staging (kHapticArgBytes), so that the copy is asynchronous; args_ev: recorded after the copy,
  hipEvent_t args_ev = nullptr;          // waited for before the next call rewrites the staging (long complete by then)
  // pick
  DevBuf<double> pick_d;          // per-workgroup minima ...
  DevBuf<int> pick_i;             // ... and their caller ids
  DevBuf<PickResult> pick_out;
  // box
  DevBuf<int> box_cnt, box_off;   // [workgroups] hits of each | hits before it; box_off[workgroups] the total
  DevBuf<int> box_ids;            // [capacity]
  DevBuf<double> box_xyz;         // [3 capacity]
  // volume
  DevBuf<double> vol;             // [n_tets] per element
  DevBuf<double> vol_part;        // [workgroups] + the total
  HapticWork() = default;
  HapticWork(const HapticWork&) = delete;
  HapticWork& operator=(const HapticWork&) = delete;
  ~HapticWork() {
    if (args_ev) (void)hipEventDestroy(args_ev);
    if (args_pinned) (void)hipHostFree(args_pinned);
  }
};
constexpr size_t kHapticArgBytes = sizeof(double) * (3 * (size_t)FB_HAPTIC_MAX_SOURCES + 256) + sizeof(int) * (size_t)FB_HAPTIC_MAX_SOURCES;

// Adds the n forces and their rings into fext (internal order).  ids: the caller's, validated by the caller of this function;
// new_of_old: the renumbering's map (null: the caller's order is the internal one).  No host wait: the arguments leave through pinned staging.
int haptic_spread(hipStream_t s, HapticWork& H, int n_nodes, int n_tets, const int4* tets, const int* new_of_old, int n, const int* ids, const double* forces3, int size,
                  double* fext);
// ... the rings alone, of n sources already on the device (d_ids[n], d_f3[3 n], d_mag[size]; the sources' own nodes are the caller's to add):
// the level-array passes in batches of kHapticBatch, for any n.  What haptic_spread ends with, and fb_fem_contact_apply's fallback.
int haptic_spread_rings(hipStream_t s, HapticWork& H, int n_nodes, int n_tets, const int4* tets, const int* new_of_old, int n, const int* d_ids, const double* d_f3,
                        const double* d_mag, int size, double* fext);
int haptic_pick_vertex(hipStream_t s, HapticWork& H, int n_nodes, const double* x0, const double* q, const int* new_of_old, const double wpos[3], PickResult* out);
int haptic_pick_box(hipStream_t s, HapticWork& H, int n_nodes, const double* x0, const double* q, const int* new_of_old, const double lo[3], const double hi[3], int capacity,
                    int* ids, double* xyz, int* n_found);
int haptic_volume(hipStream_t s, HapticWork& H, int n_nodes, int n_tets, const int4* tets, const double* x0, const double* q, double* total, double* per_element);

}  // namespace fb
