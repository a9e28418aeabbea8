// EdgeLabeler::labelEdge for an edge whose `from` end is fixed (SURVEY.md Appendix A [g2o-recalled]): what k_label_edges
// (marginals_kernels.hip) does per star edge gauge -> v and k_tree_labels (condense_tree_kernels.hip) per tree edge that
// starts at the gauge.
#pragma once
#include <hip/hip_runtime.h>

#include "relative_cov_device.h"

namespace cgmr {

// The edge xg -> xv with xg fixed and S (3x3 row-major) the covariance of xv: est[0..2] := xg^-1 xv
// (setMeasurementFromState); iu[0..5] := the upper triangle of the information by the unscented transform of the edge error
// (7 sigma points, alpha 1e-3, beta 2, lambda = alpha^2 3) and a 3x3 inverse.  Returns 0, or 1 when (3 + lambda) S has no
// Cholesky factor: g2o leaves the edge unlabeled, iu is the identity.
__device__ __forceinline__ int label_star_edge(const double* __restrict__ xg, const double* __restrict__ xv,
                                               const double* __restrict__ S, double* __restrict__ est, double* __restrict__ iu) {
  const double alpha = 1e-3, beta = 2.0;
  const int dim = 3;
  const double lambda = alpha * alpha * dim;
  const double wi = 1.0 / (2.0 * (dim + lambda));
  const double wm0 = lambda / (dim + lambda);
  const double wc0 = wm0 + (1.0 - alpha * alpha + beta);
  // measurement := xg^-1 * xv (setMeasurementFromState)
  double cg = cos(xg[2]), sg = sin(xg[2]);
  double dx = xv[0] - xg[0], dy = xv[1] - xg[1];
  double z0 = cg * dx + sg * dy, z1 = -sg * dx + cg * dy, z2 = j_norm_theta(xv[2] - xg[2]);
  est[0] = z0; est[1] = z1; est[2] = z2;
  // LLT of (dim + lambda) * Sigma
  double A[9], L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int q = 0; q < 9; q++) A[q] = S[q] * (dim + lambda);
  bool ok = true;
  for (int j = 0; j < 3 && ok; j++) {
    double d = A[3 * j + j];
    for (int q = 0; q < j; q++) d -= L[3 * j + q] * L[3 * j + q];
    if (!(d > 0)) { ok = false; break; }
    L[3 * j + j] = sqrt(d);
    for (int i = j + 1; i < 3; i++) {
      double s = A[3 * i + j];
      for (int q = 0; q < j; q++) s -= L[3 * i + q] * L[3 * j + q];
      L[3 * i + j] = s / L[3 * j + j];
    }
  }
  if (!ok) {   // g2o leaves the edge unlabeled: identity information
    iu[0] = 1; iu[1] = 0; iu[2] = 0; iu[3] = 1; iu[4] = 0; iu[5] = 1;
    return 1;
  }
  double err[7][3], wm[7], wc[7];
  const double czz = cos(z2), szz = sin(z2);
  for (int q = 0; q < 7; q++) {
    double px = 0, py = 0, pt = 0;
    if (q > 0) {
      int i = (q - 1) >> 1;
      double sgn = ((q - 1) & 1) ? -1.0 : 1.0;
      px = sgn * L[0 + i]; py = sgn * L[3 + i]; pt = sgn * L[6 + i];
    }
    wm[q] = q ? wi : wm0;
    wc[q] = q ? wi : wc0;
    double sx = xv[0] + px, sy = xv[1] + py, st = j_norm_theta(xv[2] + pt);
    double ddx = sx - xg[0], ddy = sy - xg[1];
    double rx = cg * ddx + sg * ddy, ry = -sg * ddx + cg * ddy, rth = j_norm_theta(st - xg[2]);
    double tx = rx - z0, ty = ry - z1;
    err[q][0] = czz * tx + szz * ty;
    err[q][1] = -szz * tx + czz * ty;
    err[q][2] = j_norm_theta(rth - z2);
  }
  double mean[3] = {0, 0, 0}, C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int q = 0; q < 7; q++)
    for (int a = 0; a < 3; a++) mean[a] += wm[q] * err[q][a];
  for (int q = 0; q < 7; q++) {
    double d[3] = {err[q][0] - mean[0], err[q][1] - mean[1], err[q][2] - mean[2]};
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) C[3 * a + b] += wc[q] * d[a] * d[b];
  }
  double a = C[0], b = C[1], c = C[2], d = C[3], e = C[4], f = C[5], g = C[6], h = C[7], i = C[8];
  double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
  double id = 1.0 / det;
  iu[0] = (e * i - f * h) * id; iu[1] = (c * h - b * i) * id; iu[2] = (b * f - c * e) * id;
  iu[3] = (a * i - c * g) * id; iu[4] = (c * d - a * f) * id; iu[5] = (a * e - b * d) * id;
  return 0;
}

}  // namespace cgmr
