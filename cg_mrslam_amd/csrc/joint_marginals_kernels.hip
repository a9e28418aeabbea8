// HIP kernels for the joint and pairwise marginal covariances and the relative-pose uncertainty built on them.
//
// Reference behaviour being extended:
//   SparseOptimizer::computeMarginals(spinv, blockIndices) accepts arbitrary (i, j) block pairs [g2o-recalled]; the reference
//   only ever asks for (h, h) (src/slam/graph_manipulator.cpp:134-142), and so did marginals_kernels.hip.
// Y = L^-1 E comes from the multi-right-hand-side forward solve of marginals_kernels.hip (launch_marginals_solve), 4 columns
// per query vertex.  Sigma_ab = Y_a^T Y_b: where marginals_kernels.hip contracts the diagonal 16x16 tiles of Y^T Y only, the
// kernels here contract a list of tiles (I, J), J <= I, or every lower tile in 64x64 macro-tiles:
//   k_gram_tiles_partial   one workgroup per (listed tile, row range), rows split over its 4 wavefronts
//   k_gram_macro_partial   one workgroup per (64x64 macro-tile, row range), wavefront w owns the tile row 4 MI + w
//   k_gram_tiles_reduce    the row ranges summed in range order (no floating-point atomics anywhere: two runs are bit-identical)
// A tile is stored as 256 doubles, element (row, col) of G_IJ = Y_I^T Y_J at row * 16 + col, at its position in the list
// (dense: position I (I + 1) / 2 + J).  Operands of v_mfma_f64_16x16x4_f64:
//   A: lane l holds Y[k0 + (l >> 4)][16 I + (l & 15)]      B: lane l holds Y[k0 + (l >> 4)][16 J + (l & 15)]
//   C/D: 4 doubles per lane, element (row = (l >> 4) + 4 * reg, col = l & 15)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "factor_model.h"
#include "gn_device.h"
#include "pcm_device.h"
#include "relative_cov_device.h"

namespace cgmr {

typedef double double4_t __attribute__((ext_vector_type(4)));

// (gram_at, dense_pos: pcm_device.h, shared with pcm_kernels.hip; j_norm_theta, relative_pose_cov: relative_cov_device.h, shared
// with condense_tree_kernels.hip)

// Partial tiles of the list: workgroup (tile t, row range s); each of the 4 wavefronts accumulates the tile over its quarter of
// the range, then the four are summed in a fixed order.  rows: rows per range, a multiple of 16.
__global__ __launch_bounds__(256) void k_gram_tiles_partial(int n, int m, int rows, int ntile, const int32_t* __restrict__ tiles,
                                                            const double* __restrict__ Y, double* __restrict__ part) {
  __shared__ double red[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x;
  const int I = tiles[2 * t], J = tiles[2 * t + 1];
  const int per = rows / 4;
  const int w0 = min(n, (int)blockIdx.y * rows + wave * per), w1 = min(n, w0 + per);
  const int kk = lane >> 4, ii = lane & 15;
  const double* ya = Y + 16 * I + ii;
  const double* yb = Y + 16 * J + ii;
  double4_t acc = {0, 0, 0, 0};
  for (int k0 = w0; k0 < w1; k0 += 4) {
    const int k = k0 + kk;
    const bool in = k < w1;
    const double a = in ? ya[(size_t)k * m] : 0.0;
    const double b = in ? yb[(size_t)k * m] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int rg = 0; rg < 4; rg++) red[wave][(kk + 4 * rg) * 16 + ii] = acc[rg];
  __syncthreads();
  const double s = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  part[((size_t)blockIdx.y * ntile + t) * 256 + tid] = s;
}

// Partial tiles of the whole lower triangle: workgroup (macro-tile (MI, MJ), MJ <= MI, row range s).  Wavefront w walks the
// whole range for the tile row I = 4 MI + w against the macro-tile's 4 tile columns: one A operand feeds 4 MFMAs, and the B
// operands are the same for the 4 wavefronts (they meet in the cache), so Y is read about 4x less than with a workgroup per
// 16x16 tile.  Tiles above the diagonal or beyond T are neither computed nor stored.
__global__ __launch_bounds__(256) void k_gram_macro_partial(int n, int m, int rows, int T, const double* __restrict__ Y,
                                                            double* __restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // macro-tile of blockIdx.x: MI (MI + 1) / 2 + MJ
  int MI = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while ((MI + 1) * (MI + 2) / 2 <= (int)blockIdx.x) MI++;
  while (MI * (MI + 1) / 2 > (int)blockIdx.x) MI--;
  const int MJ = (int)blockIdx.x - MI * (MI + 1) / 2;
  const int I = 4 * MI + wave;
  if (I >= T) return;                                             // (no barrier in this kernel)
  const int k_begin = min(n, (int)blockIdx.y * rows), k_end = min(n, k_begin + rows);
  const int kk = lane >> 4, ii = lane & 15;
  const int ntile = T * (T + 1) / 2;
  const double* ya = Y + 16 * I + ii;
  double4_t acc[4];
#pragma unroll
  for (int c = 0; c < 4; c++) acc[c] = double4_t{0, 0, 0, 0};
  for (int k0 = k_begin; k0 < k_end; k0 += 4) {
    const int k = k0 + kk;
    const bool in = k < k_end;
    const double a = in ? ya[(size_t)k * m] : 0.0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int J = 4 * MJ + c;
      if (J > I) continue;                                        // (wavefront-uniform)
      const double b = in ? Y[(size_t)k * m + 16 * J + ii] : 0.0;
      acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int J = 4 * MJ + c;
    if (J > I) continue;
    double* o = part + ((size_t)blockIdx.y * ntile + (size_t)I * (I + 1) / 2 + J) * 256;
#pragma unroll
    for (int rg = 0; rg < 4; rg++) o[(kk + 4 * rg) * 16 + ii] = acc[c][rg];
  }
}

// G[tile][row][col] = sum over the row ranges, in range order
__global__ void k_gram_tiles_reduce(long long total, int nsplit, const double* __restrict__ part, double* __restrict__ G) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  double s = 0;
  for (int c = 0; c < nsplit; c++) s += part[(size_t)c * total + q];
  G[q] = s;
}

// Dense joint covariance, [3 nK x 3 nK] row-major in query order: slot[k] = the query's 4-column group of Y, or -1 (fixed /
// inactive: zeros).  Every element comes out of the lower tiles (gram_at), so the output is exactly symmetric.
__global__ void k_joint_extract(int nK, const int32_t* __restrict__ slot, const double* __restrict__ G, double* __restrict__ cov) {
  const long long N = 3LL * nK;
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= N * N) return;
  const int r = (int)(q / N), c = (int)(q - (long long)r * N);
  const int sa = slot[r / 3], sb = slot[c / 3];
  double v = 0.0;
  if (sa >= 0 && sb >= 0) {
    const int ca = 4 * sa + r % 3, cb = 4 * sb + c % 3;
    v = gram_at(G, dense_pos(ca, cb), ca, cb);
  }
  cov[q] = v;
}

// Blocks of pairs: pr[5 p ..] = slot of a, slot of b (or -1), list positions of the tiles holding (a, a), (a, b), (b, b).
// Rows of ab index a.  One thread per (pair, element).
__global__ void k_pairs_extract(int nP, const int32_t* __restrict__ pr, const double* __restrict__ G, double* __restrict__ aa,
                                double* __restrict__ ab, double* __restrict__ bb) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 9LL * nP) return;
  const int p = (int)(q / 9), e = (int)(q - 9LL * p);
  const int32_t* P = pr + 5 * (size_t)p;
  const int sa = P[0], sb = P[1];
  const int ca = 4 * sa + e / 3, cb = 4 * sb + e % 3;
  aa[q] = sa >= 0 ? gram_at(G, P[2], ca, 4 * sa + e % 3) : 0.0;
  bb[q] = sb >= 0 ? gram_at(G, P[4], 4 * sb + e / 3, cb) : 0.0;
  ab[q] = (sa >= 0 && sb >= 0) ? gram_at(G, P[3], ca, cb) : 0.0;
}

// z = x_a^-1 x_b and its covariance by first-order propagation of the joint covariance of (x_a, x_b) (relative_pose_cov); one
// thread per pair.  With a hypothesis (zh, Omega): e = zh^-1 z (EdgeSE2::computeError), J_e = R(zh.theta)^T (+) 1, and
// d2 = e^T (J_e Sigma_z J_e^T + Omega^-1)^-1 e (no Omega term with hyp_info null); NaN when that matrix is not positive definite.
__global__ void k_relative_cov(int nP, const int32_t* __restrict__ pa, const int32_t* __restrict__ pb,
                               const double* __restrict__ poses, const double* __restrict__ aa, const double* __restrict__ ab,
                               const double* __restrict__ bb, const double* __restrict__ hyp_meas,
                               const double* __restrict__ hyp_info, double* __restrict__ rel, double* __restrict__ rel_cov,
                               double* __restrict__ d2) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nP) return;
  const double* xa = poses + 3 * (size_t)pa[p];
  const double* xb = poses + 3 * (size_t)pb[p];
  double z[3], Sz[9];
  relative_pose_cov(xa, xb, aa + 9 * (size_t)p, ab + 9 * (size_t)p, bb + 9 * (size_t)p, z, Sz);
  if (rel) for (int i = 0; i < 3; i++) rel[3 * (size_t)p + i] = z[i];
  if (rel_cov) for (int i = 0; i < 9; i++) rel_cov[9 * (size_t)p + i] = Sz[i];
  if (!d2) return;
  const double* zh = hyp_meas + 3 * (size_t)p;
  const double cz = cos(zh[2]), sz = sin(zh[2]);
  const double tx = z[0] - zh[0], ty = z[1] - zh[1];
  const double e[3] = {cz * tx + sz * ty, -sz * tx + cz * ty, j_norm_theta(z[2] - zh[2])};
  const double Je[9] = {cz, sz, 0, -sz, cz, 0, 0, 0, 1};
  double T1[9], S[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double u = 0;
      for (int k = 0; k < 3; k++) u += Je[3 * i + k] * Sz[3 * k + j];
      T1[3 * i + j] = u;
    }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j <= i; j++) {
      double u = 0;
      for (int k = 0; k < 3; k++) u += T1[3 * i + k] * Je[3 * j + k];
      S[3 * i + j] = u; S[3 * j + i] = u;
    }
  if (hyp_info) {
    const double* iu = hyp_info + 6 * (size_t)p;
    const double a = iu[0], b = iu[1], cc = iu[2], d = iu[3], f = iu[4], g = iu[5];     // [[a b cc] [b d f] [cc f g]]
    const double det = a * (d * g - f * f) - b * (b * g - f * cc) + cc * (b * f - d * cc);
    const double id = 1.0 / det;
    const double W[6] = {(d * g - f * f) * id, (cc * f - b * g) * id, (b * f - cc * d) * id,
                         (a * g - cc * cc) * id, (b * cc - a * f) * id, (a * d - b * b) * id};
    S[0] += W[0]; S[1] += W[1]; S[2] += W[2]; S[3] += W[1]; S[4] += W[3]; S[5] += W[4]; S[6] += W[2]; S[7] += W[4]; S[8] += W[5];
  }
  // S = L L^T; d2 = |L^-1 e|^2
  double L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool ok = true;
  for (int j = 0; j < 3 && ok; j++) {
    double d = S[3 * j + j];
    for (int q = 0; q < j; q++) d -= L[3 * j + q] * L[3 * j + q];
    if (!(d > 0) || !(d < INFINITY)) { ok = false; break; }
    L[3 * j + j] = sqrt(d);
    for (int i = j + 1; i < 3; i++) {
      double u = S[3 * i + j];
      for (int q = 0; q < j; q++) u -= L[3 * i + q] * L[3 * j + q];
      L[3 * i + j] = u / L[3 * j + j];
    }
  }
  double r = NAN;
  if (ok) {
    const double y0 = e[0] / L[0];
    const double y1 = (e[1] - L[3] * y0) / L[4];
    const double y2 = (e[2] - L[6] * y0 - L[7] * y1) / L[8];
    r = y0 * y0 + y1 * y1 + y2 * y2;
  }
  d2[p] = r;
}

// The predicted observation of vertex b from pose a, its covariance and the gate of a candidate measurement; one thread per
// pair, kind[p] the factor the pair would be (include/cgmr.h: cgmr_observation_covariance):
//   0  pose - pose   nothing here: k_relative_cov, launched in front over the same list, has written the pair (EDGE_SE2)
//   1  pose - point  z = R_a^T (l - t_a) (2),  J = [A rows 0-1 | R_a^T] (2x5)            (EDGE_SE2_XY)
//   2  pose - point  z = atan2(ry, rx) (1),    J = (-ry / q) J1 row 0 + (rx / q) J1 row 1  (EDGE_BEARING_SE2_XY), q = rx^2 + ry^2
// S = J Sigma J^T with Sigma the 5x5 joint covariance of (x_a, l): the pose's block, the first two columns of Sigma_ab, the
// point's leading 2x2 (the point's dummy third unknown is never read).  With a hypothesis: e = z - zh (the bearing's
// normalised), d2 = e^T (S + Omega^-1)^-1 e in the factor's own dimension, Omega from info_upper[0, 1, 3] / info_upper[0];
// NaN when that matrix is not positive definite.  Outputs padded to 3 and 3x3 with exact zeros.  A bearing of a point on
// the pose (q == 0): z = 0, S and d2 NaN.
__global__ void k_observation_cov(int nP, const int32_t* __restrict__ pa, const int32_t* __restrict__ pb,
                                  const uint8_t* __restrict__ kind, const double* __restrict__ poses,
                                  const double* __restrict__ aa, const double* __restrict__ ab, const double* __restrict__ bb,
                                  const double* __restrict__ hyp_meas, const double* __restrict__ hyp_info,
                                  double* __restrict__ zo, double* __restrict__ cov, double* __restrict__ d2) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nP) return;
  const int fk = kind[p];
  if (fk == CGMR_EDGE_SE2) return;
  const double* xa = poses + 3 * (size_t)pa[p];
  const double* xl = poses + 3 * (size_t)pb[p];
  const double c = cos(xa[2]), s = sin(xa[2]);
  const double dx = xl[0] - xa[0], dy = xl[1] - xa[1];
  const double rx = c * dx + s * dy, ry = -s * dx + c * dy;
  const double* Saa = aa + 9 * (size_t)p;
  const double* Sab = ab + 9 * (size_t)p;
  const double* Sbb = bb + 9 * (size_t)p;
  double Sg[25];                                                  // the joint covariance of (x_a, l)
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) Sg[5 * i + j] = Saa[3 * i + j];
    for (int j = 0; j < 2; j++) { Sg[5 * i + 3 + j] = Sab[3 * i + j]; Sg[5 * (3 + j) + i] = Sab[3 * i + j]; }
  }
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2; j++) Sg[5 * (3 + i) + 3 + j] = Sbb[3 * i + j];
  double J[10] = {-c, -s, ry, c, s, s, -c, -rx, -s, c};
  const int dim = fk == CGMR_EDGE_SE2_XY ? 2 : 1;
  double z[3] = {rx, ry, 0.0};
  bool on_pose = false;
  if (fk == CGMR_EDGE_BEARING_SE2_XY) {
    const double q = rx * rx + ry * ry;
    on_pose = !(q > 0.0);
    z[0] = on_pose ? 0.0 : atan2(ry, rx);
    z[1] = 0.0;
    const double u = -ry / q, v = rx / q;
    for (int k = 0; k < 5; k++) J[k] = u * J[k] + v * J[5 + k];
    J[2] = -1.0;
  }
  // M = J Sigma (2 x 5), S = M J^T (2 x 2); a bearing uses S(0, 0) alone (its second row of J is left over from kind 1)
  double M[10], S[4];
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 5; j++) {
      double u = 0;
      for (int k = 0; k < 5; k++) u += J[5 * i + k] * Sg[5 * k + j];
      M[5 * i + j] = u;
    }
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2; j++) {
      double u = 0;
      for (int k = 0; k < 5; k++) u += M[5 * i + k] * J[5 * j + k];
      S[2 * i + j] = u;
    }
  if (dim == 2) { const double u = 0.5 * (S[1] + S[2]); S[1] = u; S[2] = u; }
  if (on_pose) S[0] = NAN;
  if (zo) for (int i = 0; i < 3; i++) zo[3 * (size_t)p + i] = z[i];
  if (cov) {
    double* o = cov + 9 * (size_t)p;
    for (int i = 0; i < 9; i++) o[i] = 0.0;
    o[0] = S[0];
    if (dim == 2) { o[1] = S[1]; o[3] = S[2]; o[4] = S[3]; }
  }
  if (!d2) return;
  const double* zh = hyp_meas + 3 * (size_t)p;
  double r = NAN;
  if (dim == 2) {
    const double e0 = z[0] - zh[0], e1 = z[1] - zh[1];
    double m00 = S[0], m01 = S[1], m11 = S[3];
    if (hyp_info) {
      const double* iu = hyp_info + 6 * (size_t)p;
      const double a = iu[0], b = iu[1], d = iu[3];
      const double id = 1.0 / (a * d - b * b);
      m00 += d * id; m01 -= b * id; m11 += a * id;
    }
    // M = L L^T; d2 = |L^-1 e|^2
    if (m00 > 0 && m00 < INFINITY) {
      const double l00 = sqrt(m00), l10 = m01 / l00, dd = m11 - l10 * l10;
      if (dd > 0 && dd < INFINITY) {
        const double y0 = e0 / l00, y1 = (e1 - l10 * y0) / sqrt(dd);
        r = y0 * y0 + y1 * y1;
      }
    }
  } else if (!on_pose) {
    const double e0 = j_norm_theta(z[0] - zh[0]);
    double m = S[0];
    if (hyp_info) m += 1.0 / hyp_info[6 * (size_t)p];
    if (m > 0 && m < INFINITY) r = e0 * e0 / m;
  }
  d2[p] = r;
}

// ----------------------------------------------------------------------------------- launchers
void joint_gram_split(int n, long long nwg, int* rows_out, int* nsplit_out) {
  // about kTargetWgs workgroups in all; a range is at least kMinRows rows (a multiple of 16: 4 wavefronts x 4 rows a step)
  constexpr long long kTargetWgs = 2048;
  constexpr int kMinRows = 128;
  long long want = nwg > 0 ? (kTargetWgs + nwg - 1) / nwg : 1;
  const long long most = (n + kMinRows - 1) / kMinRows;
  if (want > most) want = most;
  if (want < 1) want = 1;
  int rows = (int)((n + want - 1) / want);
  rows = ((rows + 15) / 16) * 16;
  if (rows < 16) rows = 16;
  *rows_out = rows;
  *nsplit_out = n > 0 ? (n + rows - 1) / rows : 1;
}

void launch_joint_gram(hipStream_t st, int n, int m, const double* Y, const JointGram& J) {
  if (J.ntile <= 0) return;
  double* part = J.nsplit > 1 ? J.part : J.G;                 // one range: the partial tiles are the tiles
  if (J.tiles) {
    hipLaunchKernelGGL(k_gram_tiles_partial, dim3((unsigned)J.ntile, J.nsplit), dim3(256), 0, st, n, m, J.rows, (int)J.ntile, J.tiles, Y, part);
  } else {
    const int T = m / 16, TM = (T + 3) / 4;
    hipLaunchKernelGGL(k_gram_macro_partial, dim3(TM * (TM + 1) / 2, J.nsplit), dim3(256), 0, st, n, m, J.rows, T, Y, part);
  }
  if (J.nsplit > 1) {
    const long long total = J.ntile * 256;
    hipLaunchKernelGGL(k_gram_tiles_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, J.nsplit, part, J.G);
  }
}

void launch_joint_extract(hipStream_t st, int nK, const int32_t* slot, const double* G, double* cov) {
  const long long total = 9LL * nK * nK;
  hipLaunchKernelGGL(k_joint_extract, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, nK, slot, G, cov);
}

void launch_pairs_extract(hipStream_t st, int nP, const int32_t* pr, const double* G, double* aa, double* ab, double* bb) {
  hipLaunchKernelGGL(k_pairs_extract, dim3((unsigned)((9LL * nP + 255) / 256)), dim3(256), 0, st, nP, pr, G, aa, ab, bb);
}

void launch_relative_cov(hipStream_t st, int nP, const int32_t* pa, const int32_t* pb, const double* poses, const double* aa,
                         const double* ab, const double* bb, const double* hyp_meas, const double* hyp_info, double* rel,
                         double* rel_cov, double* d2) {
  hipLaunchKernelGGL(k_relative_cov, dim3((nP + 63) / 64), dim3(64), 0, st, nP, pa, pb, poses, aa, ab, bb, hyp_meas, hyp_info, rel,
                     rel_cov, d2);
}

void launch_observation_cov(hipStream_t st, int nP, const int32_t* pa, const int32_t* pb, const uint8_t* kind, const double* poses,
                            const double* aa, const double* ab, const double* bb, const double* hyp_meas, const double* hyp_info,
                            double* z, double* cov, double* d2) {
  hipLaunchKernelGGL(k_observation_cov, dim3((nP + 63) / 64), dim3(64), 0, st, nP, pa, pb, kind, poses, aa, ab, bb, hyp_meas, hyp_info,
                     z, cov, d2);
}

}  // namespace cgmr
