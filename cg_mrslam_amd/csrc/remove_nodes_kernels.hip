// HIP kernel of vertex removal (remove_nodes_device.h; include/cgmr.h: cgmr_remove_nodes): one 64-lane workgroup per removed
// vertex, everything of it in LDS.
//
//   the unknowns: v (block 0) and the neighbours n_2 .. n_m (node k: block k); n_1 (node 0) is the gauge and has no block.
//   H [3 m x 3 m], lower triangle, row stride 49 doubles: a lane per row walks it with an odd stride, every 32-lane half on 32
//   different bank pairs.  Right-looking Cholesky, one lane per row under the pivot.  v's three columns go first: what is
//   left below them, L22, is the factor of the Schur complement -- the information of n_2 .. n_m with v marginalised out.
//   M = L22^-1 by forward substitution, one lane per column (L22 is read as a broadcast, M along a row); Sigma = M^T M over H.
//   The pair weights: one lane per pair, two rounds at most.  Prim: lane t owns node t, the arg-min of a round by shuffles.
//   The labels: one lane per tree edge.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cgmr.h"
#include "relative_cov_device.h"
#include "remove_nodes_device.h"
#include "tree_order_device.h"

namespace cgmr {

namespace {

constexpr int kMaxDeg = CGMR_REMOVE_MAX_DEGREE;
constexpr int kN = 3 * kMaxDeg;                 // unknowns at the largest degree: v and 15 neighbours
constexpr int kLd = kN + 1;                     // row stride of H, odd
constexpr int kN2 = kN - 3;                     // the trailing block at the largest degree
static_assert(kMaxDeg <= 64 && kN <= 64, "one lane per node, one lane per row");

// x^-1 of a pose (x, y, theta)
__device__ __forceinline__ void pose_inverse(const double* z, double* x) {
  const double c = cos(z[2]), s = sin(z[2]);
  x[0] = -(c * z[0] + s * z[1]); x[1] = -(-s * z[0] + c * z[1]); x[2] = j_norm_theta(-z[2]);
}

// the 3x3 block Sigma(node a, node b), rows indexing a; node 0 (the gauge n_1): zeros
__device__ __forceinline__ void sigma_block(const double* S, int a, int b, double* B) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) B[3 * r + c] = (a == 0 || b == 0) ? 0.0 : S[(3 * (a - 1) + r) * kLd + 3 * (b - 1) + c];
}

}  // namespace

__global__ __launch_bounds__(64) void k_remove_nodes(RemoveNodes P) {
  __shared__ double Hs[kN * kLd];               // H, then its factor, then Sigma of n_2 .. n_m
  __shared__ double Ms[kN2 * kN2];              // L22^-1
  __shared__ double xs[3 * kMaxDeg];            // the neighbours in v's frame
  __shared__ double vv[9 * kMaxDeg];            // each neighbour's share of H_vv
  __shared__ double Ws[kMaxDeg * kMaxDeg];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int m = P.deg[r];
  if (m < 0 || m > kMaxDeg) { if (lane == 0) P.flags[r] = 2; return; }
  if (m < 2) { if (lane == 0) P.flags[r] = 0; return; }
  const int v = P.remove[r], q0 = P.inc_off[r], q1 = P.inc_off[r + 1];
  const int N = 3 * m, N2 = N - 3;

  // ---- the local configuration, and H zeroed
  if (lane < m) {
    int q = q0;
    while (q < q1 && P.inc_node[q] != lane) q++;                  // the lowest-index edge to this neighbour (there is one)
    const int e = P.inc_edge[q];
    const double z[3] = {P.meas[3 * (size_t)e], P.meas[3 * (size_t)e + 1], P.meas[3 * (size_t)e + 2]};
    double x[3] = {z[0], z[1], j_norm_theta(z[2])};
    if (P.ef[e] != v) pose_inverse(z, x);
    xs[3 * lane] = x[0]; xs[3 * lane + 1] = x[1]; xs[3 * lane + 2] = x[2];
  }
  for (int q = lane; q < N * kLd; q += 64) Hs[q] = 0.0;
  __syncthreads();

  // ---- H: lane k sums the edges of node k in index order; it alone writes the blocks (k, k) and (k, v)
  if (lane < m) {
    double Hvv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Hnv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Hnn[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const double xn[3] = {xs[3 * lane], xs[3 * lane + 1], xs[3 * lane + 2]};
    for (int q = q0; q < q1; q++) {
      if (P.inc_node[q] != lane) continue;
      const int e = P.inc_edge[q];
      const bool fwd = P.ef[e] == v;                               // stored v -> n
      // x_i, x_j of the edge: one of them v at the identity
      const double ti = fwd ? 0.0 : xn[2];
      const double dx = fwd ? xn[0] : -xn[0], dy = fwd ? xn[1] : -xn[1];
      const double c = cos(ti), s = sin(ti);
      const double A[9] = {-c, -s, -s * dx + c * dy, s, -c, -c * dx - s * dy, 0, 0, -1};
      const double B[9] = {c, s, 0, -s, c, 0, 0, 0, 1};
      const double zt = P.meas[3 * (size_t)e + 2];
      const double cz = cos(zt), sz = sin(zt);
      double Ji[9], Jj[9];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        Ji[k] = cz * A[k] + sz * A[3 + k]; Ji[3 + k] = -sz * A[k] + cz * A[3 + k]; Ji[6 + k] = A[6 + k];
        Jj[k] = cz * B[k] + sz * B[3 + k]; Jj[3 + k] = -sz * B[k] + cz * B[3 + k]; Jj[6 + k] = B[6 + k];
      }
      const double* iu = P.info + 6 * (size_t)e;
      const double O[9] = {iu[0], iu[1], iu[2], iu[1], iu[3], iu[4], iu[2], iu[4], iu[5]};
      const double* Jv = fwd ? Ji : Jj;
      const double* Jn = fwd ? Jj : Ji;
      double OJv[9], OJn[9];
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
          double u = 0, w = 0;
#pragma unroll
          for (int k = 0; k < 3; k++) { u += O[3 * a + k] * Jv[3 * k + b]; w += O[3 * a + k] * Jn[3 * k + b]; }
          OJv[3 * a + b] = u; OJn[3 * a + b] = w;
        }
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
          double u = 0, w = 0, t = 0;
#pragma unroll
          for (int k = 0; k < 3; k++) {
            u += Jv[3 * k + a] * OJv[3 * k + b];
            w += Jn[3 * k + a] * OJv[3 * k + b];
            t += Jn[3 * k + a] * OJn[3 * k + b];
          }
          Hvv[3 * a + b] += u; Hnv[3 * a + b] += w; Hnn[3 * a + b] += t;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) vv[9 * lane + k] = Hvv[k];
    if (lane > 0)
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
          Hs[(3 * lane + a) * kLd + b] = Hnv[3 * a + b];
          Hs[(3 * lane + a) * kLd + 3 * lane + b] = Hnn[3 * a + b];
        }
  }
  __syncthreads();
  if (lane < 9) {                                                  // H_vv: the neighbours' shares in node order
    double u = 0;
    for (int k = 0; k < m; k++) u += vv[9 * k + lane];
    Hs[(lane / 3) * kLd + lane % 3] = u;
  }
  __syncthreads();

  // ---- Cholesky, in place in the lower triangle; lane t has row j + 1 + t of column j
  for (int j = 0; j < N; j++) {
    const double d = Hs[j * kLd + j];
    if (!(d > 0) || !(d < INFINITY)) { if (lane == 0) P.flags[r] = 1; return; }   // (every lane reads the same pivot)
    const double ljj = sqrt(d);
    const int i = j + 1 + lane;
    double lij = 0;
    if (i < N) { lij = Hs[i * kLd + j] / ljj; Hs[i * kLd + j] = lij; }
    __syncthreads();
    if (lane == 0) Hs[j * kLd + j] = ljj;
    if (i < N)
      for (int k = j + 1; k <= i; k++) Hs[i * kLd + k] -= lij * Hs[k * kLd + j];
    __syncthreads();
  }

  // ---- M = L22^-1: lane c has column c.  Rows above c come out as zeros by themselves.
  if (lane < N2) {
    for (int i = 0; i < N2; i++) {
      const double* Li = Hs + (3 + i) * kLd + 3;
      double u = i == lane ? 1.0 : 0.0;
      for (int k = 0; k < i; k++) u -= Li[k] * Ms[k * kN2 + lane];
      Ms[i * kN2 + lane] = i < lane ? 0.0 : u / Li[i];
    }
  }
  __syncthreads();
  // ---- Sigma = M^T M over H, both triangles (the same products in the same order: symmetric bit for bit)
  for (int q = lane; q < N2 * N2; q += 64) {
    const int a = q / N2, b = q - a * N2;
    double u = 0;
    for (int k = max(a, b); k < N2; k++) u += Ms[k * kN2 + a] * Ms[k * kN2 + b];
    Hs[a * kLd + b] = u;
  }
  __syncthreads();

  // ---- the weight of every pair of nodes a < b
  for (int q = lane; q < kMaxDeg * kMaxDeg; q += 64) Ws[q] = INFINITY;
  __syncthreads();
  for (int q = lane; q < m * (m - 1) / 2; q += 64) {
    int b = (int)((1.0 + sqrt(1.0 + 8.0 * (double)q)) * 0.5);     // q = b (b - 1) / 2 + a, a < b
    while (b * (b + 1) / 2 <= q) b++;
    while (b * (b - 1) / 2 > q) b--;
    const int a = q - b * (b - 1) / 2;
    double Saa[9], Sab[9], Sbb[9], z[3], Sz[9];
    sigma_block(Hs, a, a, Saa);
    sigma_block(Hs, a, b, Sab);
    sigma_block(Hs, b, b, Sbb);
    relative_pose_cov(xs + 3 * a, xs + 3 * b, Saa, Sab, Sbb, z, Sz);
    const double w = logdet3(Sz);
    Ws[a * kMaxDeg + b] = w;
    Ws[b * kMaxDeg + a] = w;
  }
  __syncthreads();

  // ---- Prim from node 0: lane t keeps node t's best edge into the tree
  const bool node = lane < m;
  bool in_tree = lane == 0;
  int par = lane == 0 ? -1 : 0;
  double key = (node && lane > 0) ? Ws[lane] : 0.0;
  for (int round = 1; round < m; round++) {
    double bw = INFINITY;
    int bv = -1, bp = 0;
    if (node && !in_tree) { bw = key; bv = lane; bp = par; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double ow = __shfl_xor(bw, off);
      const int ov = __shfl_xor(bv, off), op = __shfl_xor(bp, off);
      if (edge_before(ow, op, ov, bw, bp, bv)) { bw = ow; bp = op; bv = ov; }
    }
    const int u = bv;                                              // (uniform; some node is always outside)
    if (u < 0) break;
    if (lane == u) in_tree = true;
    if (node && !in_tree) {
      const double w = Ws[u * kMaxDeg + lane];
      if (edge_before(w, u, lane, key, par, lane)) { key = w; par = u; }
    }
  }
  const bool edge = node && lane > 0;
  if (__any(edge && !(key < INFINITY))) { if (lane == 0) P.flags[r] = 3; return; }

  // ---- the labels, first order: lane t has the edge par -> t
  if (edge) {
    double Spp[9], Spc[9], Scc[9], z[3], Sz[9];
    sigma_block(Hs, par, par, Spp);
    sigma_block(Hs, par, lane, Spc);
    sigma_block(Hs, lane, lane, Scc);
    relative_pose_cov(xs + 3 * par, xs + 3 * lane, Spp, Spc, Scc, z, Sz);
    const double c = cos(z[2]), s = sin(z[2]);
    const double Je[9] = {c, s, 0, -s, c, 0, 0, 0, 1};
    double T[9], C[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) {
        double u = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) u += Je[3 * a + k] * Sz[3 * k + b];
        T[3 * a + b] = u;
      }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) {
        double u = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) u += T[3 * a + k] * Je[3 * b + k];
        C[3 * a + b] = u;
      }
    // the inverse of the symmetrised C from its Cholesky factor, C = L L^T, Z = L^-1, C^-1 = Z^T Z: no cancelling cofactors
    // (DESIGN.md 2.17).  C is a rotation of Sz, whose Cholesky factor the chosen weight has already taken.
    const double a = C[0], b = 0.5 * (C[1] + C[3]), cc = 0.5 * (C[2] + C[6]), e = C[4], f = 0.5 * (C[5] + C[7]), i = C[8];
    const double l00 = sqrt(a), l10 = b / l00, l20 = cc / l00;
    const double l11 = sqrt(e - l10 * l10), l21 = (f - l20 * l10) / l11;
    const double l22 = sqrt(i - l20 * l20 - l21 * l21);
    const double z00 = 1.0 / l00, z11 = 1.0 / l11, z22 = 1.0 / l22;
    const double z10 = -l10 * z00 * z11, z21 = -l21 * z11 * z22, z20 = -(l20 * z00 + l21 * z10) * z22;
    const size_t o = (size_t)P.out_off[r] + (size_t)(lane - 1);
    double* iu = P.info_out + 6 * o;
    iu[0] = z00 * z00 + z10 * z10 + z20 * z20; iu[1] = z10 * z11 + z20 * z21; iu[2] = z20 * z22;
    iu[3] = z11 * z11 + z21 * z21; iu[4] = z21 * z22; iu[5] = z22 * z22;
    P.est[3 * o] = z[0]; P.est[3 * o + 1] = z[1]; P.est[3 * o + 2] = z[2];
    P.parent[o] = par;
    P.weight[o] = key;
  }
  if (lane == 0) P.flags[r] = 0;
}

void launch_remove_nodes(hipStream_t st, const RemoveNodes& P) {
  if (P.nR <= 0) return;
  hipLaunchKernelGGL(k_remove_nodes, dim3((unsigned)P.nR), dim3(64), 0, st, P);
}

}  // namespace cgmr
