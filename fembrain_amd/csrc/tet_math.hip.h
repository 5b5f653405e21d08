// Per-element 3x3 helpers of the tet kernels, shared by the units that form an element's deformation gradient and rotation
// (fem_device.hip.h: rest records and the assembly's k_tet_warp; stress.hip: k_tet_stress).  One definition, so the rotation of
// every unit is the assembly's.
#pragma once
#include <hip/hip_runtime.h>

namespace fb {

// entries of a handle's material table (fem_device.hip.h, "Per-element materials")
constexpr int kMaxMaterials = 256;

__device__ inline void inv3x3(const double* A, double* I) {
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double id = 1.0 / (A[0] * c00 + A[1] * c01 + A[2] * c02);
  I[0] = c00 * id; I[1] = (A[2] * A[7] - A[1] * A[8]) * id; I[2] = (A[1] * A[5] - A[2] * A[4]) * id;
  I[3] = c01 * id; I[4] = (A[0] * A[8] - A[2] * A[6]) * id; I[5] = (A[2] * A[3] - A[0] * A[5]) * id;
  I[6] = c02 * id; I[7] = (A[1] * A[6] - A[0] * A[7]) * id; I[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}

// scaled-Newton polar decomposition of F (row-major), R out; returns last determinant
// (vegafem polarDecomposition.cpp:37-108; the iteration is data dependent, capped for safety)
__device__ inline double one_norm3(const double* A) {
  return fmax(fmax(fabs(A[0]) + fabs(A[3]) + fabs(A[6]), fabs(A[1]) + fabs(A[4]) + fabs(A[7])), fabs(A[2]) + fabs(A[5]) + fabs(A[8]));
}
__device__ inline double inf_norm3(const double* A) {
  return fmax(fmax(fabs(A[0]) + fabs(A[1]) + fabs(A[2]), fabs(A[3]) + fabs(A[4]) + fabs(A[5])), fabs(A[6]) + fabs(A[7]) + fabs(A[8]));
}

__device__ inline double polar_rotation(const double* F, double* R, double tol) {
  double Mk[9], A[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Mk[3 * i + j] = F[3 * j + i];
  double M1 = one_norm3(Mk), Mi = inf_norm3(Mk), det = 0.0, E1;
  int guard = 0;
  do {
    A[0] = Mk[4] * Mk[8] - Mk[5] * Mk[7]; A[1] = Mk[5] * Mk[6] - Mk[3] * Mk[8]; A[2] = Mk[3] * Mk[7] - Mk[4] * Mk[6];
    A[3] = Mk[7] * Mk[2] - Mk[8] * Mk[1]; A[4] = Mk[8] * Mk[0] - Mk[6] * Mk[2]; A[5] = Mk[6] * Mk[1] - Mk[7] * Mk[0];
    A[6] = Mk[1] * Mk[5] - Mk[2] * Mk[4]; A[7] = Mk[2] * Mk[3] - Mk[0] * Mk[5]; A[8] = Mk[0] * Mk[4] - Mk[1] * Mk[3];
    det = Mk[0] * A[0] + Mk[1] * A[1] + Mk[2] * A[2];
    if (det == 0.0) break;
    const double A1 = one_norm3(A), Ai = inf_norm3(A);
    const double gamma = sqrt(sqrt((A1 * Ai) / (M1 * Mi)) / fabs(det));
    const double g1 = gamma * 0.5, g2 = 0.5 / (gamma * det);
    double Ek[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
      Ek[i] = Mk[i];
      Mk[i] = g1 * Mk[i] + g2 * A[i];
      Ek[i] -= Mk[i];
    }
    E1 = one_norm3(Ek);
    M1 = one_norm3(Mk);
    Mi = inf_norm3(Mk);
  } while (E1 > M1 * tol && ++guard < 64);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) R[3 * i + j] = Mk[3 * j + i];
  return det;
}

// y_i = sum_j K0[ij] v_j with the undeformed element stiffness in closed form, K0[ij] = V [lambda b_i b_j^T + mu b_j b_i^T + mu (b_i.b_j) I]
// (fem_device.hip.h: k_tet_warp's exact tangent; motion.hip: with the rotated gradients c_k for b_k it is the element's K_e)
__device__ inline void k0_apply(const double b[4][3], double V, double lambda, double mu, const double* v, double* y) {
  double sl = 0.0, sm[3] = {0, 0, 0}, sg[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const double bv = b[j][0] * v[3 * j] + b[j][1] * v[3 * j + 1] + b[j][2] * v[3 * j + 2];
    sl += bv;                                   // sum_j b_j . v_j
#pragma unroll
    for (int a = 0; a < 3; a++) {
      sm[a] += b[j][a] * bv;                    // unused below (kept symmetric form): sum_j b_j (b_j . v_j)
#pragma unroll
      for (int c = 0; c < 3; c++) sg[a][c] += b[j][a] * v[3 * j + c];  // sum_j b_j v_j^T
    }
  }
  (void)sm;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int a = 0; a < 3; a++) {
      // lambda b_i (sum_j b_j.v_j) + mu sum_j b_j (b_i.v_j) + mu sum_j (b_i.b_j) v_j
      double t1 = 0.0, t2 = 0.0;
#pragma unroll
      for (int c = 0; c < 3; c++) { t1 += sg[a][c] * b[i][c]; t2 += b[i][c] * sg[c][a]; }
      y[3 * i + a] = V * (lambda * b[i][a] * sl + mu * t1 + mu * t2);
    }
}

// the material id k_tet_warp<.., MAT> leaves in the V lane of quarter 1 of an element's step record (fem_device.hip.h, "Per-element materials")
template <typename MT>
__device__ __forceinline__ int rec_mat_id(MT w) { return (int)w & (kMaxMaterials - 1); }

}  // namespace fb
