// Element stress and strain on the device (stress.hip): fb_fem_stress / fb_fem_read_stress / fb_fem_surface_stress / fb_fem_time_stress.
// The bracket of the corotational element force, f_e,i = V R [lambda tr(H) I + mu (H + H^T)] b_i (fem_device.hip.h, k_tet_warp;
// E B (R^T x - x0) of corotationalLinearFEM.cpp:107-137, 270-286), which the assembly forms every step and does not keep.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

namespace fb {

// Everything the stress pass of one handle owns.  Nothing is allocated before the first fb_fem_stress; the allocations are kept
// (grow-only, the handle's slack rule).  `valid` follows the mesh generation as SurfaceWork::valid does.
struct StressWork {
  bool valid = false;        // vm / psi / J (and the tensors, with FB_STRESS_TENSORS) belong to the handle's current mesh
  int n_elements = 0, flags = 0;
  DevBuf<double> vm, psi, J;         // [n_tets] von Mises stress, energy density, det F
  DevBuf<double> sig, eps;           // [6 n_tets] xx yy zz xy yz zx, FB_STRESS_TENSORS only
  DevBuf<double> part_d;             // [3 workgroups] largest von Mises | smallest J | sum of V psi of each workgroup
  DevBuf<int> part_i;                // [3 workgroups] element of the first | of the second | inverted elements
  DevBuf<fb_fem_stress_info> out;        // what fb_fem_stress brings back in one copy
  DevBuf<float> surf_vm;             // [n_vertices] fb_fem_surface_stress
};

struct StressArgs {
  int n_tets, n_nodes;
  const int4* tets;
  const double *x0, *q, *rest;
  double lambda, mu;
  const uint8_t* mat_ids;   // null: the uniform instantiation
  const double* mtab;
  int linear, world;
};

// vm / psi / J of every element (and the tensors, with `tensors`) from the current q, and the summary in one copy (out may be null: none)
int stress_elements(hipStream_t s, StressWork& S, const StressArgs& a, bool tensors, fb_fem_stress_info* out);

// the mean von Mises stress of the elements behind every surface vertex's faces into S.surf_vm (inc_off / inc / face_tets: SurfaceWork's)
int stress_surface(hipStream_t s, StressWork& S, int n_vertices, int n_faces, const int* inc_off, const uint32_t* inc, const int* face_tets);

}  // namespace fb
