// HIP kernels for the pairwise consistency maximisation (PCM) of loop-closure candidates: which candidates agree with each
// other, given what the graph knows about the poses between them (include/cgmr.h: cgmr_closure_consistency).
//
// Reference behaviour being replaced: LoopClosureChecker::check (src/slam/closure_checker.cpp) makes each candidate exact in turn
// and counts the others' chi2 under a constant information against a fixed threshold; the trajectory's uncertainty between two
// closures does not enter.  Here every pair of candidates is tested with the Mahalanobis distance of the loop the pair closes,
// under the joint covariance of the four poses it touches, and the largest set of pairwise consistent candidates is kept.
//
//   k_closure_consistency   one thread per pair l < k, behind the dense Gram tiles of the unique endpoints
//                           (joint_marginals_kernels.hip: k_gram_macro_partial; the tiles stay on the device)
//   k_closure_consistency_inter   the same for candidates that end at a peer robot's vertex, known only by the pose (and,
//                           where the caller has one, the covariance) the peer sent (cgmr_closure_consistency_inter)
//   k_consistency_bits      rows of d2 -> rows of 64-bit words, one __ballot per word
//   k_clique_greedy         one workgroup per seed: P in LDS, candidates strided over the threads, __popcll counts
//   k_clique_best           the seeds' results reduced by (size, lowest seed), the winner's members written ascending
// The clique search is the greedy heuristic of PCM implementations, not an exact maximum-clique solver.
// No workgroup waits for another, nothing spins, every loop has a bound known at launch; no floating-point atomics: two calls
// give identical bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcm_device.h"

namespace cgmr {

typedef unsigned long long u64;

namespace {

// theta into (-pi, pi]
__device__ __forceinline__ double p_norm_theta(double t) {
  const double pi = 3.14159265358979323846;
  if (t > -pi && t <= pi) return t;
  return t - 2 * pi * ceil((t - pi) / (2 * pi));
}

// C = A B (3x3, row-major)
__device__ __forceinline__ void mul3(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// S += X + X^T (off == true) or S += X (off == false), X = J_i B J_j^T
__device__ __forceinline__ void add_jbjt(const double* Ji, const double* B, const double* Jj, bool off, double* S) {
  double T[9];
  mul3(Ji, B, T);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double x = T[3 * i] * Jj[3 * j] + T[3 * i + 1] * Jj[3 * j + 1] + T[3 * i + 2] * Jj[3 * j + 2];
      S[3 * i + j] += x;
      if (off) S[3 * j + i] += x;
    }
}

// T = A (+) B (theta left as the sum) and dT/dA for additive updates of A; dT/dB is the rotation by A's theta
__device__ __forceinline__ void compose(const double* A, const double* B, double* T, double* dA) {
  const double c = cos(A[2]), s = sin(A[2]);
  T[0] = A[0] + c * B[0] - s * B[1];
  T[1] = A[1] + s * B[0] + c * B[1];
  T[2] = A[2] + B[2];
  dA[0] = 1; dA[1] = 0; dA[2] = -s * B[0] - c * B[1];
  dA[3] = 0; dA[4] = 1; dA[5] = c * B[0] - s * B[1];
  dA[6] = 0; dA[7] = 0; dA[8] = 1;
}

__device__ __forceinline__ void rot3(double th, double* R) {
  const double c = cos(th), s = sin(th);
  R[0] = c; R[1] = -s; R[2] = 0; R[3] = s; R[4] = c; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
}

// z = x_a^-1 x_b and its Jacobians for additive updates of x_a and x_b (A and B of EdgeSE2 with a zero measurement)
__device__ __forceinline__ void relative(const double* xa, const double* xb, double* z, double* Ja, double* Jb) {
  const double c = cos(xa[2]), s = sin(xa[2]);
  const double dx = xb[0] - xa[0], dy = xb[1] - xa[1];
  z[0] = c * dx + s * dy; z[1] = -s * dx + c * dy; z[2] = xb[2] - xa[2];
  Ja[0] = -c; Ja[1] = -s; Ja[2] = z[1]; Ja[3] = s; Ja[4] = -c; Ja[5] = -z[0]; Ja[6] = 0; Ja[7] = 0; Ja[8] = -1;
  Jb[0] = c; Jb[1] = s; Jb[2] = 0; Jb[3] = -s; Jb[4] = c; Jb[5] = 0; Jb[6] = 0; Jb[7] = 0; Jb[8] = 1;
}

// Omega^-1 of the 6 upper entries [[a b c] [b d f] [c f g]], by the adjugate (as k_relative_cov), full 3x3
__device__ __forceinline__ void info_inverse(const double* iu, double* W) {
  const double a = iu[0], b = iu[1], cc = iu[2], d = iu[3], f = iu[4], g = iu[5];
  const double det = a * (d * g - f * f) - b * (b * g - f * cc) + cc * (b * f - d * cc);
  const double id = 1.0 / det;
  W[0] = (d * g - f * f) * id; W[1] = (cc * f - b * g) * id; W[2] = (b * f - cc * d) * id;
  W[4] = (a * g - cc * cc) * id; W[5] = (b * cc - a * f) * id; W[8] = (a * d - b * b) * id;
  W[3] = W[1]; W[6] = W[2]; W[7] = W[5];
}

}  // namespace

// Pair (k, l), l < k: the loop residual eps = z_k (+) (x_bk^-1 x_bl) (+) z_l^-1 (+) (x_al^-1 x_ak), its covariance
// S = J_x Sigma J_x^T + J_zk Omega_k^-1 J_zk^T + J_zl Omega_l^-1 J_zl^T by first-order propagation -- Sigma the 12x12 joint
// covariance of (x_ak, x_bk, x_al, x_bl) out of the Gram tiles, cross-covariances included --, and d2 = eps^T S^-1 eps;
// NaN where S is not finite or not positive definite.
// With T1 = z_k, T2 = x_bk^-1 x_bl, T3 = z_l^-1, T4 = x_al^-1 x_ak and the partial products P2 = T1 T2, P3 = P2 T3:
//   d eps / d T4 = R(P3),  d eps / d T3 = L3 R(P2),  d eps / d T2 = L3 L2 R(T1),  d eps / d T1 = L3 L2 L1
// (L1, L2, L3: the derivatives of T1 (+) T2, P2 (+) T3, P3 (+) T4 in their left factor), chained with the Jacobians of the two
// relative poses and of the inverse.  Sigma is never formed: its 10 blocks on and above the diagonal are read one at a time.
__device__ __forceinline__ double pair_d2(const PcmClosures& C, const double* __restrict__ poses, const double* __restrict__ G,
                                          int k, int l) {
  const double* zk = C.meas + 3 * (size_t)k;
  const double* zl = C.meas + 3 * (size_t)l;
  const double* xak = poses + 3 * (size_t)C.a[k];
  const double* xbk = poses + 3 * (size_t)C.b[k];
  const double* xal = poses + 3 * (size_t)C.a[l];
  const double* xbl = poses + 3 * (size_t)C.b[l];
  double T2[3], T3[3], T4[3], P2[3], P3[3], eps[3];
  double J2a[9], J2b[9], J4a[9], J4b[9], L1[9], L2[9], L3[9], R[9], U[9], V[9];
  double J[4][9], Jzk[9], Jzl[9];                                 // J: for x_ak, x_bk, x_al, x_bl
  relative(xbk, xbl, T2, J2a, J2b);
  relative(xal, xak, T4, J4a, J4b);
  // T3 = z_l^-1 and its Jacobian
  const double cl = cos(zl[2]), sl = sin(zl[2]);
  T3[0] = -cl * zl[0] - sl * zl[1]; T3[1] = sl * zl[0] - cl * zl[1]; T3[2] = -zl[2];
  const double Ji[9] = {-cl, -sl, T3[1], sl, -cl, -T3[0], 0, 0, -1};
  compose(zk, T2, P2, L1);
  compose(P2, T3, P3, L2);
  compose(P3, T4, eps, L3);
  eps[2] = p_norm_theta(eps[2]);
  rot3(P3[2], R);                                                 // d eps / d T4
  mul3(R, J4a, J[2]);
  mul3(R, J4b, J[0]);
  rot3(P2[2], R);
  mul3(L3, R, U);                                                 // d eps / d T3
  mul3(U, Ji, Jzl);
  mul3(L3, L2, U);
  rot3(zk[2], R);
  mul3(U, R, V);                                                  // d eps / d T2
  mul3(V, J2a, J[1]);
  mul3(V, J2b, J[3]);
  mul3(U, L1, Jzk);                                               // d eps / d T1
  const int32_t sl4[4] = {C.slot[2 * k], C.slot[2 * k + 1], C.slot[2 * l], C.slot[2 * l + 1]};
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = i; j < 4; j++) {
      if (sl4[i] < 0 || sl4[j] < 0) continue;                     // fixed / inactive: zero rows of Sigma
      const int ca = 4 * sl4[i], cb = 4 * sl4[j];
      const long long pos = dense_pos(ca, cb);
      double B[9];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) B[3 * r + c] = gram_at(G, pos, ca + r, cb + c);
      add_jbjt(J[i], B, J[j], j != i, S);
    }
  double W[9];
  info_inverse(C.info + 6 * (size_t)k, W);
  add_jbjt(Jzk, W, Jzk, false, S);
  info_inverse(C.info + 6 * (size_t)l, W);
  add_jbjt(Jzl, W, Jzl, false, S);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < i; j++) { const double u = 0.5 * (S[3 * i + j] + S[3 * j + i]); S[3 * i + j] = u; S[3 * j + i] = u; }
  // S = L L^T; d2 = |L^-1 eps|^2
  double L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    double d = S[3 * j + j];
    for (int p = 0; p < j; p++) d -= L[3 * j + p] * L[3 * j + p];
    if (!(d > 0) || !(d < INFINITY)) ok = false;
    L[3 * j + j] = sqrt(d);
    for (int i = j + 1; i < 3; i++) {
      double u = S[3 * i + j];
      for (int p = 0; p < j; p++) u -= L[3 * i + p] * L[3 * j + p];
      L[3 * i + j] = u / L[3 * j + j];
    }
  }
  double r = NAN;
  if (ok) {
    const double y0 = eps[0] / L[0];
    const double y1 = (eps[1] - L[3] * y0) / L[4];
    const double y2 = (eps[2] - L[6] * y0 - L[7] * y1) / L[8];
    r = y0 * y0 + y1 * y1 + y2 * y2;
    if (!(r < INFINITY)) r = NAN;                                 // (an entry of S that is not finite)
  }
  return r;
}

// One thread per pair l < k (as k_relative_cov's one per pair; 246 VGPRs, no scratch): its d2 written to (k, l) and (l, k).
// Threads q < n also write the zero diagonal.
__global__ __launch_bounds__(64) void k_closure_consistency(PcmClosures C, const double* __restrict__ poses,
                                                            const double* __restrict__ G, double* __restrict__ d2) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = C.n;
  if (q < n) d2[(size_t)q * n + q] = 0.0;
  if (q >= (long long)n * (n - 1) / 2) return;
  // q = k (k - 1) / 2 + l
  int k = (int)((1.0 + sqrt(1.0 + 8.0 * (double)q)) * 0.5);
  while ((long long)k * (k + 1) / 2 <= q) k++;
  while ((long long)k * (k - 1) / 2 > q) k--;
  const int l = (int)(q - (long long)k * (k - 1) / 2);
  const double r = pair_d2(C, poses, G, k, l);
  d2[(size_t)k * n + l] = r;
  d2[(size_t)l * n + k] = r;
}

// The two-graph form (cgmr_closure_consistency_inter): candidate k goes from the own vertex a[k] to a peer vertex that is in no
// graph, known by the pose peer[3 k ..] the peer sent.  Pair (k, l), l < k: pair_d2's residual with x_b replaced by p,
//   eps = z_k (+) (p_k^-1 p_l) (+) z_l^-1 (+) (x_al^-1 x_ak),
// the same chain of Jacobians, and S = J_a Sigma_a J_a^T + J_p Sigma_p J_p^T + J_zk Omega_k^-1 J_zk^T + J_zl Omega_l^-1 J_zl^T:
// Sigma_a the 6x6 joint covariance of (x_ak, x_al) out of the Gram tiles (3 blocks), Sigma_p the 6x6 sub-matrix at candidates
// (k, l) of the caller's peer_cov, read from its lower triangle (3 blocks; none when peer_cov is null: the peer's poses taken as
// exact).  The two graphs share no factor, so there is no cross term.  Symmetrisation, factorisation of S and the rejection
// test are pair_d2's, statement for statement.
__device__ __forceinline__ double pair_d2_inter(const PcmInterClosures& C, const double* __restrict__ poses,
                                                const double* __restrict__ G, int k, int l) {
  const double* zk = C.meas + 3 * (size_t)k;
  const double* zl = C.meas + 3 * (size_t)l;
  const double* xak = poses + 3 * (size_t)C.a[k];
  const double* xbk = C.peer + 3 * (size_t)k;
  const double* xal = poses + 3 * (size_t)C.a[l];
  const double* xbl = C.peer + 3 * (size_t)l;
  double T2[3], T3[3], T4[3], P2[3], P3[3], eps[3];
  double J2a[9], J2b[9], J4a[9], J4b[9], L1[9], L2[9], L3[9], R[9], U[9], V[9];
  double Ja[2][9], Jp[2][9], Jzk[9], Jzl[9];                      // Ja: for x_ak, x_al; Jp: for p_k, p_l
  relative(xbk, xbl, T2, J2a, J2b);
  relative(xal, xak, T4, J4a, J4b);
  // T3 = z_l^-1 and its Jacobian
  const double cl = cos(zl[2]), sl = sin(zl[2]);
  T3[0] = -cl * zl[0] - sl * zl[1]; T3[1] = sl * zl[0] - cl * zl[1]; T3[2] = -zl[2];
  const double Ji[9] = {-cl, -sl, T3[1], sl, -cl, -T3[0], 0, 0, -1};
  compose(zk, T2, P2, L1);
  compose(P2, T3, P3, L2);
  compose(P3, T4, eps, L3);
  eps[2] = p_norm_theta(eps[2]);
  rot3(P3[2], R);                                                 // d eps / d T4
  mul3(R, J4a, Ja[1]);
  mul3(R, J4b, Ja[0]);
  rot3(P2[2], R);
  mul3(L3, R, U);                                                 // d eps / d T3
  mul3(U, Ji, Jzl);
  mul3(L3, L2, U);
  rot3(zk[2], R);
  mul3(U, R, V);                                                  // d eps / d T2
  mul3(V, J2a, Jp[0]);
  mul3(V, J2b, Jp[1]);
  mul3(U, L1, Jzk);                                               // d eps / d T1
  const int32_t sl2[2] = {C.slot[k], C.slot[l]};
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = i; j < 2; j++) {
      if (sl2[i] < 0 || sl2[j] < 0) continue;                     // fixed / inactive: zero rows of Sigma_a
      const int ca = 4 * sl2[i], cb = 4 * sl2[j];
      const long long pos = dense_pos(ca, cb);
      double B[9];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) B[3 * r + c] = gram_at(G, pos, ca + r, cb + c);
      add_jbjt(Ja[i], B, Ja[j], j != i, S);
    }
  if (C.peer_cov) {
    const size_t N3 = 3 * (size_t)C.n;
    const int kl[2] = {k, l};
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = i; j < 2; j++) {
        double B[9];                                              // block (kl[i], kl[j]), rows kl[i], out of the lower triangle
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const size_t row = 3 * (size_t)kl[i] + r, col = 3 * (size_t)kl[j] + c;
            B[3 * r + c] = row >= col ? C.peer_cov[row * N3 + col] : C.peer_cov[col * N3 + row];
          }
        add_jbjt(Jp[i], B, Jp[j], j != i, S);
      }
  }
  double W[9];
  info_inverse(C.info + 6 * (size_t)k, W);
  add_jbjt(Jzk, W, Jzk, false, S);
  info_inverse(C.info + 6 * (size_t)l, W);
  add_jbjt(Jzl, W, Jzl, false, S);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < i; j++) { const double u = 0.5 * (S[3 * i + j] + S[3 * j + i]); S[3 * i + j] = u; S[3 * j + i] = u; }
  // S = L L^T; d2 = |L^-1 eps|^2
  double L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    double d = S[3 * j + j];
    for (int p = 0; p < j; p++) d -= L[3 * j + p] * L[3 * j + p];
    if (!(d > 0) || !(d < INFINITY)) ok = false;
    L[3 * j + j] = sqrt(d);
    for (int i = j + 1; i < 3; i++) {
      double u = S[3 * i + j];
      for (int p = 0; p < j; p++) u -= L[3 * i + p] * L[3 * j + p];
      L[3 * i + j] = u / L[3 * j + j];
    }
  }
  double r = NAN;
  if (ok) {
    const double y0 = eps[0] / L[0];
    const double y1 = (eps[1] - L[3] * y0) / L[4];
    const double y2 = (eps[2] - L[6] * y0 - L[7] * y1) / L[8];
    r = y0 * y0 + y1 * y1 + y2 * y2;
    if (!(r < INFINITY)) r = NAN;                                 // (an entry of S that is not finite)
  }
  return r;
}

// One thread per pair l < k, k_closure_consistency's mapping: its d2 written to (k, l) and (l, k); threads q < n also write
// the zero diagonal.
__global__ __launch_bounds__(64) void k_closure_consistency_inter(PcmInterClosures C, const double* __restrict__ poses,
                                                                  const double* __restrict__ G, double* __restrict__ d2) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = C.n;
  if (q < n) d2[(size_t)q * n + q] = 0.0;
  if (q >= (long long)n * (n - 1) / 2) return;
  // q = k (k - 1) / 2 + l
  int k = (int)((1.0 + sqrt(1.0 + 8.0 * (double)q)) * 0.5);
  while ((long long)k * (k + 1) / 2 <= q) k++;
  while ((long long)k * (k - 1) / 2 > q) k--;
  const int l = (int)(q - (long long)k * (k - 1) / 2);
  const double r = pair_d2_inter(C, poses, G, k, l);
  d2[(size_t)k * n + l] = r;
  d2[(size_t)l * n + k] = r;
}

// Word (k, w): lane t tests column 64 w + t of row k; NaN is not adjacent, the diagonal and the padding bits are zero.
__global__ __launch_bounds__(64) void k_consistency_bits(int n, int W, const double* __restrict__ d2, double gamma,
                                                         u64* __restrict__ adj) {
  const int w = blockIdx.x, k = blockIdx.y, l = 64 * w + (int)threadIdx.x;
  const bool on = l < n && l != k && d2[(size_t)k * n + l] < gamma;
  const u64 word = __ballot(on);
  if (threadIdx.x == 0) adj[(size_t)k * W + w] = word;
}

// The greedy clique from seed s = blockIdx.x: C = {s}, P = A[s]; while P is not empty, the u in P with the largest
// |A[u] & P| (ties: the lowest index) joins C and P &= A[u].  A round's arg-max is the maximum of the 64-bit key
// (count << 32) | (2^32 - 1 - u): 0 only when no thread holds a candidate, i.e. P is empty.  A has a zero diagonal, so u leaves
// P in its own round and there are at most n rounds.
__global__ __launch_bounds__(256) void k_clique_greedy(int n, int W, const u64* __restrict__ adj, u64* __restrict__ seed_bits,
                                                       int32_t* __restrict__ seed_size) {
  __shared__ u64 P[16], Cm[16], red[4];                           // W <= 16 (CGMR_PCM_MAX_CLOSURES = 1024)
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < W) {
    P[tid] = adj[(size_t)s * W + tid];
    Cm[tid] = tid == (s >> 6) ? 1ull << (s & 63) : 0ull;
  }
  __syncthreads();
  int size = 1;
  for (int round = 0; round < n; round++) {
    u64 best = 0;
    for (int u = tid; u < n; u += 256) {
      if (!((P[u >> 6] >> (u & 63)) & 1ull)) continue;
      const u64* row = adj + (size_t)u * W;
      int cnt = 0;
      for (int w = 0; w < W; w++) cnt += __popcll(row[w] & P[w]);
      const u64 key = ((u64)cnt << 32) | (u64)(0xFFFFFFFFu - (unsigned)u);
      best = key > best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const u64 o = __shfl_xor(best, off);
      best = o > best ? o : best;
    }
    if (lane == 0) red[wave] = best;
    __syncthreads();
    const u64 b01 = red[0] > red[1] ? red[0] : red[1], b23 = red[2] > red[3] ? red[2] : red[3];
    best = b01 > b23 ? b01 : b23;
    if (best == 0) break;                                         // (the same value in every thread)
    const int u = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
    __syncthreads();                                              // P and red have been read by everybody
    if (tid < W) {
      P[tid] &= adj[(size_t)u * W + tid];
      if (tid == (u >> 6)) Cm[tid] |= 1ull << (u & 63);
    }
    size++;
    __syncthreads();
  }
  if (tid < W) seed_bits[(size_t)s * W + tid] = Cm[tid];
  if (tid == 0) seed_size[s] = size;
}

// The largest clique over the seeds, ties to the lowest seed: out[0] = size, out[1] = seed, out[2 ..] the members ascending,
// -1 behind them.  One workgroup.
__global__ __launch_bounds__(256) void k_clique_best(int n, int W, const u64* __restrict__ seed_bits,
                                                     const int32_t* __restrict__ seed_size, int32_t* __restrict__ out) {
  __shared__ u64 red[256];
  const int tid = threadIdx.x;
  u64 best = 0;
  for (int s = tid; s < n; s += 256) {
    const u64 key = ((u64)seed_size[s] << 32) | (u64)(0xFFFFFFFFu - (unsigned)s);
    best = key > best ? key : best;
  }
  red[tid] = best;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h && red[tid + h] > red[tid]) red[tid] = red[tid + h];
    __syncthreads();
  }
  if (tid != 0) return;
  const int seed = (int)(0xFFFFFFFFu - (unsigned)(red[0] & 0xFFFFFFFFull));
  out[0] = (int32_t)(red[0] >> 32);
  out[1] = seed;
  int m = 0;
  for (int w = 0; w < W; w++) {
    u64 word = seed_bits[(size_t)seed * W + w];
    while (word) {
      out[2 + m++] = 64 * w + (__ffsll((long long)word) - 1);
      word &= word - 1;
    }
  }
  for (; m < n; m++) out[2 + m] = -1;
}

// ----------------------------------------------------------------------------------- launchers
void launch_closure_consistency(hipStream_t st, const PcmClosures& C, const double* poses, const double* G, double* d2) {
  const long long np = (long long)C.n * (C.n - 1) / 2, nt = np > C.n ? np : C.n;
  hipLaunchKernelGGL(k_closure_consistency, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, st, C, poses, G, d2);
}

void launch_closure_consistency_inter(hipStream_t st, const PcmInterClosures& C, const double* poses, const double* G, double* d2) {
  const long long np = (long long)C.n * (C.n - 1) / 2, nt = np > C.n ? np : C.n;
  hipLaunchKernelGGL(k_closure_consistency_inter, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, st, C, poses, G, d2);
}

void launch_consistency_bits(hipStream_t st, int n, const double* d2, double gamma, unsigned long long* adj) {
  const int W = (n + 63) / 64;
  hipLaunchKernelGGL(k_consistency_bits, dim3(W, n), dim3(64), 0, st, n, W, d2, gamma, adj);
}

void launch_clique_greedy(hipStream_t st, int n, const unsigned long long* adj, unsigned long long* seed_bits, int32_t* seed_size,
                          int32_t* out) {
  const int W = (n + 63) / 64;
  hipLaunchKernelGGL(k_clique_greedy, dim3(n), dim3(256), 0, st, n, W, adj, seed_bits, seed_size);
  hipLaunchKernelGGL(k_clique_best, dim3(1), dim3(256), 0, st, n, W, seed_bits, seed_size, out);
}

}  // namespace cgmr
