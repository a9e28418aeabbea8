// The weight of a candidate edge and the total order of the spanning-tree searches on the device: what k_tree_weights and
// k_min_spanning_tree (condense_tree_kernels.hip) and k_remove_nodes (remove_nodes_kernels.hip) share.
#pragma once
#include <hip/hip_runtime.h>

namespace cgmr {

// log det S of a symmetric 3x3 from its Cholesky pivots; +inf where a pivot is not positive and finite
__device__ __forceinline__ double logdet3(const double* S) {
  double L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double w = 0.0;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    double d = S[3 * j + j];
    for (int q = 0; q < j; q++) d -= L[3 * j + q] * L[3 * j + q];
    if (!(d > 0) || !(d < INFINITY)) return INFINITY;
    w += log(d);
    L[3 * j + j] = sqrt(d);
    for (int i = j + 1; i < 3; i++) {
      double u = S[3 * i + j];
      for (int q = 0; q < j; q++) u -= L[3 * i + q] * L[3 * j + q];
      L[3 * i + j] = u / L[3 * j + j];
    }
  }
  return w == w ? w : INFINITY;
}

// edge (p1, v1) of weight w1 before edge (p2, v2) of weight w2 in the total order (w, max, min); v < 0: no edge (last)
__device__ __forceinline__ bool edge_before(double w1, int p1, int v1, double w2, int p2, int v2) {
  if (v1 < 0) return false;
  if (v2 < 0) return true;
  if (w1 < w2) return true;
  if (w1 > w2) return false;
  const int h1 = max(p1, v1), h2 = max(p2, v2);
  if (h1 != h2) return h1 < h2;
  return min(p1, v1) < min(p2, v2);
}

}  // namespace cgmr
