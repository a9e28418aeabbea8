// The relative pose of two vertices and its first-order covariance on the device: what k_relative_cov
// (joint_marginals_kernels.hip) computes per pair and k_tree_weights (condense_tree_kernels.hip) per candidate edge.
#pragma once
#include <hip/hip_runtime.h>

namespace cgmr {

// theta into [-pi, pi)
__device__ __forceinline__ double j_norm_theta(double t) {
  const double pi = 3.14159265358979323846;
  if (t >= -pi && t < pi) return t;
  return t - 2 * pi * floor((t + pi) / (2 * pi));
}

// z = x_a^-1 x_b and Sigma_z by first-order propagation of the joint covariance of (x_a, x_b): Saa, Sab (rows index a), Sbb,
// 3x3 row-major.  J_a, J_b: the Jacobians of z for the additive (x, y, theta) update -- A and B of k_linearize
// (gn_kernels.hip) with a zero measurement.  Sigma_z comes back symmetrised.
__device__ __forceinline__ void relative_pose_cov(const double* __restrict__ xa, const double* __restrict__ xb,
                                                  const double* __restrict__ Saa, const double* __restrict__ Sab,
                                                  const double* __restrict__ Sbb, double* z, double* Sz) {
  const double c = cos(xa[2]), s = sin(xa[2]);
  const double dx = xb[0] - xa[0], dy = xb[1] - xa[1];
  z[0] = c * dx + s * dy; z[1] = -s * dx + c * dy; z[2] = j_norm_theta(xb[2] - xa[2]);
  const double Ja[9] = {-c, -s, -s * dx + c * dy, s, -c, -c * dx - s * dy, 0, 0, -1};
  const double Jb[9] = {c, s, 0, -s, c, 0, 0, 0, 1};
  // M_a = J_a Saa + J_b Sab^T, M_b = J_a Sab + J_b Sbb;  Sigma_z = M_a J_a^T + M_b J_b^T
  double Ma[9], Mb[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double u = 0, v = 0;
      for (int k = 0; k < 3; k++) {
        u += Ja[3 * i + k] * Saa[3 * k + j] + Jb[3 * i + k] * Sab[3 * j + k];
        v += Ja[3 * i + k] * Sab[3 * k + j] + Jb[3 * i + k] * Sbb[3 * k + j];
      }
      Ma[3 * i + j] = u; Mb[3 * i + j] = v;
    }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double u = 0;
      for (int k = 0; k < 3; k++) u += Ma[3 * i + k] * Ja[3 * j + k] + Mb[3 * i + k] * Jb[3 * j + k];
      Sz[3 * i + j] = u;
    }
  // (the two cross terms are each other's transposes: the sum is symmetric to rounding; returned symmetrised)
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < i; j++) { const double u = 0.5 * (Sz[3 * i + j] + Sz[3 * j + i]); Sz[3 * i + j] = u; Sz[3 * j + i] = u; }
}

}  // namespace cgmr
