// HIP kernels for the condensed graph as a spanning tree of relative poses (condense_tree_device.h; include/cgmr.h:
// cgmr_condense_tree, cgmr_min_spanning_tree).
//
// Reference behaviour being extended:
//   CondensedGraphCreator::compute (src/mrslam/condensed_graph/condensed_graph_creator.cpp:33-66) builds a star gauge -> v and
//   labels every edge from Sigma_vv alone; the cross-covariances between the requested vertices are dropped.  Here the dense
//   lower tiles of Y^T Y (joint_marginals_kernels.hip) hold Sigma_ab of any two requested vertices:
//     k_tree_weights        one thread per unordered pair of nodes: log det of the covariance of x_a^-1 x_b (relative_pose_cov)
//     k_min_spanning_tree   one workgroup: Prim from the root, n - 1 rounds of (arg-min over the nodes outside, relaxation along
//                           the new node's row), under the total order (w, max(a, b), min(a, b)) -- the tree is unique
//     k_tree_labels         one thread per tree edge: EdgeLabeler's unscented transform, over the child alone where the parent is
//                           the gauge (label_star_edge), over both ends otherwise (13 sigma points of the 6x6 joint covariance)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cgmr.h"
#include "condense_tree_device.h"
#include "label_device.h"
#include "pcm_device.h"
#include "relative_cov_device.h"
#include "tree_order_device.h"

namespace cgmr {

namespace {

// the 3x3 block Sigma(node with slot sa, node with slot sb), rows indexing the first, out of the dense lower tiles; a slot of -1
// (the gauge, a fixed or inactive vertex): zeros.  A query's 4 columns never straddle a tile: one tile holds the block.
__device__ __forceinline__ void gram_block(const double* __restrict__ G, int sa, int sb, double* B) {
  if (sa < 0 || sb < 0) {
#pragma unroll
    for (int q = 0; q < 9; q++) B[q] = 0.0;
    return;
  }
  const int ca = 4 * sa, cb = 4 * sb;
  const long long pos = dense_pos(ca, cb);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) B[3 * r + c] = gram_at(G, pos, ca + r, cb + c);
}

__device__ __forceinline__ double clean_weight(double w) { return w == w ? w : INFINITY; }

constexpr int kMstThreads = 256;

}  // namespace

__global__ __launch_bounds__(64) void k_tree_weights(TreeNodes N, const double* __restrict__ poses, const double* __restrict__ G,
                                                     double* __restrict__ W) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = N.n;
  if (q < n) W[(size_t)q * n + q] = INFINITY;
  if (q >= (long long)n * (n - 1) / 2) return;
  // q = a (a - 1) / 2 + b, b < a
  int a = (int)((1.0 + sqrt(1.0 + 8.0 * (double)q)) * 0.5);
  while ((long long)a * (a + 1) / 2 <= q) a++;
  while ((long long)a * (a - 1) / 2 > q) a--;
  const int b = (int)(q - (long long)a * (a - 1) / 2);
  const int sb = N.slot[b], sa = N.slot[a];
  double Sbb[9], Sba[9], Saa[9], z[3], Sz[9];
  gram_block(G, sb, sb, Sbb);
  gram_block(G, sb, sa, Sba);
  gram_block(G, sa, sa, Saa);
  relative_pose_cov(poses + 3 * (size_t)N.vert[b], poses + 3 * (size_t)N.vert[a], Sbb, Sba, Saa, z, Sz);   // x_b^-1 x_a, b < a
  // a requested vertex without a covariance (no edge touches it) is not known exactly, it is not known at all: no finite weight
  const double w = (sa < 0 || (b != 0 && sb < 0)) ? INFINITY : logdet3(Sz);
  W[(size_t)a * n + b] = w;
  W[(size_t)b * n + a] = w;
}

// Prim from the root.  Thread t owns the nodes t, t + 256, ...: it alone reads and writes their key (the best edge into the
// tree so far), parent and membership, so the only exchange between threads is the arg-min of a round -- within a wavefront by
// shuffles, across the four through LDS, in two buffers taken in turn (one barrier a round).
__global__ __launch_bounds__(kMstThreads) void k_min_spanning_tree(int n, const double* __restrict__ W, int root,
                                                                    int32_t* __restrict__ parent, double* __restrict__ wsel) {
  __shared__ double key[CGMR_TREE_MAX_NODES];
  __shared__ int32_t par[CGMR_TREE_MAX_NODES];
  __shared__ uint8_t in_tree[CGMR_TREE_MAX_NODES];
  __shared__ double red_w[2][kMstThreads / 64];
  __shared__ int32_t red_v[2][kMstThreads / 64], red_p[2][kMstThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int v = tid; v < n; v += kMstThreads) {
    in_tree[v] = v == root;
    par[v] = v == root ? -1 : root;
    key[v] = v == root ? 0.0 : clean_weight(W[(size_t)root * n + v]);
  }
  for (int round = 1; round < n; round++) {
    double bw = INFINITY;
    int bv = -1, bp = 0;
    for (int v = tid; v < n; v += kMstThreads)
      if (!in_tree[v] && edge_before(key[v], par[v], v, bw, bp, bv)) { bw = key[v]; bp = par[v]; bv = v; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double ow = __shfl_xor(bw, off);
      const int ov = __shfl_xor(bv, off), op = __shfl_xor(bp, off);
      if (edge_before(ow, op, ov, bw, bp, bv)) { bw = ow; bp = op; bv = ov; }
    }
    const int buf = round & 1;
    if (lane == 0) { red_w[buf][wave] = bw; red_v[buf][wave] = bv; red_p[buf][wave] = bp; }
    __syncthreads();
    bw = red_w[buf][0]; bv = red_v[buf][0]; bp = red_p[buf][0];
#pragma unroll
    for (int k = 1; k < kMstThreads / 64; k++)
      if (edge_before(red_w[buf][k], red_p[buf][k], red_v[buf][k], bw, bp, bv)) { bw = red_w[buf][k]; bp = red_p[buf][k]; bv = red_v[buf][k]; }
    const int u = bv;                                             // (uniform; some node is always outside)
    if (u < 0) break;
    if ((u & (kMstThreads - 1)) == tid) in_tree[u] = 1;
    const double* row = W + (size_t)u * n;
    for (int v = tid; v < n; v += kMstThreads) {
      if (in_tree[v] || v == u) continue;
      const double w = clean_weight(row[v]);
      if (edge_before(w, u, v, key[v], par[v], v)) { key[v] = w; par[v] = u; }
    }
  }
  for (int v = tid; v < n; v += kMstThreads) { parent[v] = par[v]; wsel[v] = key[v]; }
}

namespace {

// EdgeLabeler::labelEdge for an edge xp -> xc with both ends free: est := xp^-1 xc; the 13 sigma points of N(0, S6), S6 =
// [Spp Spc; Spc^T Scc], sampleUnscented's rule at dimension 6 (alpha 1e-3, beta 2, lambda = alpha^2 6): L = chol((6 + lambda) S6),
// points 0, +-L[:, i]; each applied to both vertices by the additive (x, y, theta) update with normalised theta, the edge error
// taken in the measurement's frame; their weighted mean and covariance, and a 3x3 inverse.  Returns 0, or 1 without a factor.
__device__ __forceinline__ int label_tree_edge(const double* __restrict__ xp, const double* __restrict__ xc, const double* Spp,
                                               const double* Spc, const double* Scc, double* __restrict__ est,
                                               double* __restrict__ iu) {
  const double alpha = 1e-3, beta = 2.0;
  const int dim = 6;
  const double lambda = alpha * alpha * dim;
  const double wi = 1.0 / (2.0 * (dim + lambda));
  const double wm0 = lambda / (dim + lambda);
  const double wc0 = wm0 + (1.0 - alpha * alpha + beta);
  const double cp = cos(xp[2]), sp = sin(xp[2]);
  const double dx = xc[0] - xp[0], dy = xc[1] - xp[1];
  const double z0 = cp * dx + sp * dy, z1 = -sp * dx + cp * dy, z2 = j_norm_theta(xc[2] - xp[2]);
  est[0] = z0; est[1] = z1; est[2] = z2;
  // LLT of (dim + lambda) * S6, in place in the lower triangle
  double L[36];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      L[6 * r + c] = Spp[3 * r + c] * (dim + lambda);
      L[6 * (3 + r) + c] = Spc[3 * c + r] * (dim + lambda);
      L[6 * (3 + r) + 3 + c] = Scc[3 * r + c] * (dim + lambda);
      L[6 * r + 3 + c] = 0.0;
    }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double d = L[6 * j + j];
#pragma unroll
    for (int q = 0; q < j; q++) d -= L[6 * j + q] * L[6 * j + q];
    if (!(d > 0) || !(d < INFINITY)) ok = false;
    const double ljj = sqrt(d);
    L[6 * j + j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = L[6 * i + j];
#pragma unroll
      for (int q = 0; q < j; q++) s -= L[6 * i + q] * L[6 * j + q];
      L[6 * i + j] = s / ljj;
      L[6 * j + i] = 0.0;                                         // (the upper triangle: the sigma points read whole columns)
    }
  }
  if (!ok) {   // g2o leaves the edge unlabeled: identity information
    iu[0] = 1; iu[1] = 0; iu[2] = 0; iu[3] = 1; iu[4] = 0; iu[5] = 1;
    return 1;
  }
  double err[13][3];
  const double czz = cos(z2), szz = sin(z2);
#pragma unroll
  for (int q = 0; q < 13; q++) {
    double d[6] = {0, 0, 0, 0, 0, 0};
    if (q > 0) {
      const int i = (q - 1) >> 1;
      const double sgn = ((q - 1) & 1) ? -1.0 : 1.0;
#pragma unroll
      for (int r = 0; r < 6; r++) d[r] = sgn * L[6 * r + i];
    }
    const double px = xp[0] + d[0], py = xp[1] + d[1], pt = j_norm_theta(xp[2] + d[2]);
    const double cx = xc[0] + d[3], cy = xc[1] + d[4], ct = j_norm_theta(xc[2] + d[5]);
    const double c = cos(pt), s = sin(pt);
    const double ddx = cx - px, ddy = cy - py;
    const double rx = c * ddx + s * ddy, ry = -s * ddx + c * ddy, rth = j_norm_theta(ct - pt);
    const double tx = rx - z0, ty = ry - z1;
    err[q][0] = czz * tx + szz * ty;
    err[q][1] = -szz * tx + czz * ty;
    err[q][2] = j_norm_theta(rth - z2);
  }
  double mean[3] = {0, 0, 0}, C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 13; q++)
    for (int a = 0; a < 3; a++) mean[a] += (q ? wi : wm0) * err[q][a];
#pragma unroll
  for (int q = 0; q < 13; q++) {
    const double d[3] = {err[q][0] - mean[0], err[q][1] - mean[1], err[q][2] - mean[2]};
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) C[3 * a + b] += (q ? wi : wc0) * d[a] * d[b];
  }
  const double a = C[0], b = C[1], c = C[2], d = C[3], e = C[4], f = C[5], g = C[6], h = C[7], i = C[8];
  const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
  const double id = 1.0 / det;
  iu[0] = (e * i - f * h) * id; iu[1] = (c * h - b * i) * id; iu[2] = (b * f - c * e) * id;
  iu[3] = (a * i - c * g) * id; iu[4] = (c * d - a * f) * id; iu[5] = (a * e - b * d) * id;
  return 0;
}

}  // namespace

__global__ __launch_bounds__(64) void k_tree_labels(TreeNodes N, const int32_t* __restrict__ parent, const double* __restrict__ wsel,
                                                    const double* __restrict__ poses, const double* __restrict__ G,
                                                    double* __restrict__ est, double* __restrict__ info, int32_t* __restrict__ flags) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N.n - 1) return;
  const int k = e + 1, p = parent[k];
  const double* xp = poses + 3 * (size_t)N.vert[p];
  const double* xc = poses + 3 * (size_t)N.vert[k];
  double* ze = est + 3 * (size_t)e;
  double* iu = info + 6 * (size_t)e;
  const int sp = N.slot[p], sc = N.slot[k];
  if (!(wsel[k] < INFINITY)) {                                    // hung on the tree by no finite weight: unlabelled
    const double c = cos(xp[2]), s = sin(xp[2]);
    const double dx = xc[0] - xp[0], dy = xc[1] - xp[1];
    ze[0] = c * dx + s * dy; ze[1] = -s * dx + c * dy; ze[2] = j_norm_theta(xc[2] - xp[2]);
    iu[0] = 1; iu[1] = 0; iu[2] = 0; iu[3] = 1; iu[4] = 0; iu[5] = 1;
    flags[e] = 2;
    return;
  }
  double Scc[9];
  gram_block(G, sc, sc, Scc);
  if (sp < 0) {                                                   // the parent is the gauge (or as fixed as it): a star edge
    flags[e] = label_star_edge(xp, xc, Scc, ze, iu);
    return;
  }
  double Spp[9], Spc[9];
  gram_block(G, sp, sp, Spp);
  gram_block(G, sp, sc, Spc);
  flags[e] = label_tree_edge(xp, xc, Spp, Spc, Scc, ze, iu);
}

// ----------------------------------------------------------------------------------- launchers
void launch_tree_weights(hipStream_t st, const TreeNodes& N, const double* poses, const double* G, double* W) {
  const long long pairs = (long long)N.n * (N.n - 1) / 2, total = pairs > N.n ? pairs : N.n;
  hipLaunchKernelGGL(k_tree_weights, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, N, poses, G, W);
}

void launch_min_spanning_tree(hipStream_t st, int n, const double* W, int root, int32_t* parent, double* wsel) {
  hipLaunchKernelGGL(k_min_spanning_tree, dim3(1), dim3(kMstThreads), 0, st, n, W, root, parent, wsel);
}

void launch_tree_labels(hipStream_t st, const TreeNodes& N, const int32_t* parent, const double* wsel, const double* poses,
                        const double* G, double* est, double* info, int32_t* flags) {
  if (N.n <= 1) return;
  hipLaunchKernelGGL(k_tree_labels, dim3((N.n - 1 + 63) / 64), dim3(64), 0, st, N, parent, wsel, poses, G, est, info, flags);
}

}  // namespace cgmr
