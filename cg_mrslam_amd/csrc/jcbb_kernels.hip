// HIP kernels of the joint-compatibility data association of landmark observations (include/cgmr.h: cgmr_jcbb_dense,
// cgmr_joint_compatibility): Neira and Tardos' joint compatibility branch and bound (JCBB).  A hypothesis pairs observation i
// with landmark h[i] or with none; it is admissible when every pairing is individually compatible and every prefix of it is
// jointly compatible, d2 = e^T C^-1 e < gamma[dof] with C the joint innovation covariance of the pairings (jcbb_device.h).
//
//   k_jc_sigma    (graph form) the row-major Sigma of the state out of the dense lower Gram tiles
//   k_jc_pairs    one workgroup per observation, one thread per landmark: [e and J of the pair as k_observation_cov predicts
//                 them,] ic as k_observation_cov computes it, and the observation's individually compatible landmarks in
//                 ascending (ic, index) -- a rank among the row's compatible entries, no sort, no atomics
//   k_jc_greedy   one wavefront, the lower bound: observations in order, each takes its first candidate that is unused and keeps
//                 the hypothesis jointly compatible, else none
//   k_jc_search   one wavefront per root (i0, j), an individually compatible pair: the observations before i0 unpaired, i0 with
//                 j, depth-first over i0 + 1 .. nM - 1, candidates in list order, "none" last.  Four roots per workgroup.
//                 Launched CGMR_JC_ROUNDS = 2 times: round 0 with the greedy hypothesis as the bound, round 1 only for the
//                 roots that ran out of nodes, with the best of round 0 as the bound.
//   k_jc_best     the winner over roots and rounds: most pairings, then the smallest d2, then the lowest root, then the earlier
//                 round; the greedy hypothesis when nothing beat it; proven and the node total
//
// A wavefront's hypothesis: the lower Cholesky factor of C in LDS, column-major with a stride of 64 (lane c reads column k of
// row c at k * 64 + c: consecutive addresses) -- 64 x 64 doubles = 32 KiB, four roots per workgroup 128 KiB of the 160; lane c
// keeps what belongs to row c in registers: its Jacobian row, its two blocks of the state, its observation, y_c of
// y = L^-1 e.  Appending a pairing appends its 1 or 2 rows: lane c computes the new row's entry of C against row c (a 5 x 5
// bilinear form on Sigma), a forward substitution over the columns turns the row into L's, the Schur pivot and the new entry
// of y come out of the same loop, and d2 grows by y_new^2.  Backtracking truncates the row count.  The stack (observation,
// next candidate, rows, d2 per pairing), in LDS as well, is at most nM deep; the used landmarks are 4 words in registers.
//
// A node is one joint-compatibility test (one append), the root's own included; a root stops in front of test node_limit + 1
// and keeps the best it has recorded.  A hypothesis is recorded as soon as its last pairing passes (the observations behind
// it unpaired), when it has more pairings than the bound or as many and a smaller d2 -- strictly, so of equal hypotheses the
// first in the search order stays.  A subtree is left when count + (observations left that have a candidate) cannot reach the
// bound's count, or only reaches it and d2, which never decreases, is not below the bound's.
//
// Determinism: a workgroup reads the problem, the greedy hypothesis and (round 1) what round 0 wrote; it writes only its own
// roots' entries of the current round.  Nothing it reads changes during a launch.  No workgroup waits for another, nothing
// spins, every loop is bounded by nM, nL, the row count or the node limit, no atomics: two calls give identical bytes.
//
// Measured on an MI355X (tools/gpu_jcbb_time.py): an append is a chain of D dependent steps, so a call in which
// only the roots of observation 0 search (a row of landmarks 0.5 m apart, 32 x 256) makes 7.5e5 .. 1.2e6 tests/s; with a decoy
// that leaves the greedy hypothesis one pairing all 8192 roots search in round 0, 6e7 tests/s, and the call takes 75 ms at
// node_limit 512, 229 ms at 2048, 417 ms at 4096: CGMR_JC_DEFAULT_NODE_LIMIT = 2048.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "jcbb_device.h"
#include "pcm_device.h"

namespace cgmr {

typedef unsigned long long u64;

__global__ void k_jc_sigma(int n, const int32_t* __restrict__ col, const double* __restrict__ G, double* __restrict__ sigma) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (long long)n * n) return;
  const int r = (int)(q / n), c = (int)(q - (long long)r * n);
  const int ca = col[r], cb = col[c];
  sigma[q] = (ca >= 0 && cb >= 0) ? gram_at(G, dense_pos(ca, cb), ca, cb) : 0.0;
}

namespace {

__device__ __forceinline__ double jc_norm_theta(double t) {
  const double pi = 3.14159265358979323846;
  if (t >= -pi && t < pi) return t;
  return t - 2 * pi * floor((t + pi) / (2 * pi));
}

// Sigma (a, b) out of the lower triangle
__device__ __forceinline__ double sig(const double* __restrict__ S, int n, int a, int b) {
  const int hi = a > b ? a : b, lo = a > b ? b : a;
  return S[(size_t)hi * n + lo];
}

// a distance passes when it is finite and below its threshold (NaN fails)
__device__ __forceinline__ bool jc_passes(double d2, double gamma) { return d2 < gamma && d2 > -INFINITY; }

}  // namespace

// Observation i = blockIdx.x, landmark j = threadIdx.x (+ 256 k: nL <= 256, one pass).
__global__ __launch_bounds__(256) void k_jc_pairs(JcProblem P, JcPredict G) {
  __shared__ double ic_row[256];
  __shared__ int ok_row[256];
  const int i = blockIdx.x, j = threadIdx.x, nL = P.nL;
  const int d = P.dim[i];
  double r = NAN;
  if (j < nL) {
    const size_t p = (size_t)i * nL + j;
    double J[10], e0, e1;
    if (G.poses) {
      const double* xa = G.poses + 3 * (size_t)G.obs_pose[i];
      const double* xl = G.poses + 3 * (size_t)G.lm[j];
      const double* zh = G.meas + 3 * (size_t)i;
      const double c = cos(xa[2]), s = sin(xa[2]);
      const double dx = xl[0] - xa[0], dy = xl[1] - xa[1];
      const double rx = c * dx + s * dy, ry = -s * dx + c * dy;
      const double J1[10] = {-c, -s, ry, c, s, s, -c, -rx, -s, c};
      for (int k = 0; k < 10; k++) J[k] = J1[k];
      e0 = rx - zh[0]; e1 = ry - zh[1];
      if (d == 1) {
        const double q = rx * rx + ry * ry;                        // (a point on the pose: q == 0, J and e NaN, incompatible)
        const double u = -ry / q, v = rx / q;
        for (int k = 0; k < 5; k++) { J[k] = u * J1[k] + v * J1[5 + k]; J[5 + k] = 0.0; }
        J[2] = q > 0.0 ? -1.0 : NAN;
        e0 = q > 0.0 ? jc_norm_theta(atan2(ry, rx) - zh[0]) : NAN;
        e1 = 0.0;
      }
      for (int k = 0; k < 10; k++) P.J[10 * p + k] = J[k];
      P.e[2 * p] = e0; P.e[2 * p + 1] = e1;
    } else {
      for (int k = 0; k < 10; k++) J[k] = P.J[10 * p + k];
      e0 = P.e[2 * p]; e1 = P.e[2 * p + 1];
    }
    // S = J Sigma J^T + R over the pair's five state entries, as k_observation_cov forms it
    const int pb = 3 * P.slot[i], lb = 3 * P.nA + 2 * j;
    const int idx[5] = {pb, pb + 1, pb + 2, lb, lb + 1};
    double M[10], S[4];
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 5; b++) {
        double u = 0;
        for (int k = 0; k < 5; k++) u += J[5 * a + k] * sig(P.sigma, P.n, idx[k], idx[b]);
        M[5 * a + b] = u;
      }
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 2; b++) {
        double u = 0;
        for (int k = 0; k < 5; k++) u += M[5 * a + k] * J[5 * b + k];
        S[2 * a + b] = u;
      }
    const double* Ri = P.R + 3 * (size_t)i;
    if (d == 2) {
      const double m00 = S[0] + Ri[0], m01 = 0.5 * (S[1] + S[2]) + Ri[1], m11 = S[3] + Ri[2];
      if (m00 > 0 && m00 < INFINITY) {
        const double l00 = sqrt(m00), l10 = m01 / l00, dd = m11 - l10 * l10;
        if (dd > 0 && dd < INFINITY) {
          const double y0 = e0 / l00, y1 = (e1 - l10 * y0) / sqrt(dd);
          r = y0 * y0 + y1 * y1;
        }
      }
    } else {
      const double m = S[0] + Ri[0];
      if (m > 0 && m < INFINITY) r = e0 * e0 / m;
    }
    P.ic[p] = r;
  }
  const bool ok = j < nL && jc_passes(r, P.gamma[d]);
  ic_row[j] = r;
  ok_row[j] = ok ? 1 : 0;
  __syncthreads();
  int rank = 0, total = 0;
  for (int k = 0; k < nL; k++) {
    if (!ok_row[k]) continue;
    total++;
    if (ok && (ic_row[k] < r || (ic_row[k] == r && k < j))) rank++;
  }
  if (ok) P.cand[(size_t)i * nL + rank] = j;
  if (j == 0) P.ncand[i] = total;
}

namespace {

// What a lane keeps of "its" row c = lane of the hypothesis' factor.
struct JcRow {
  double J[5] = {0, 0, 0, 0, 0};
  double y = 0;
  int pb = 0, lb = 0, obs = -1, t = 0;
};

// Pairing (i, j) appended to the hypothesis of D rows and distance d2, whose factor is Lt (LDS, element (r, k) at k * 64 + r):
// true when it stays jointly compatible, and then D and d2 are the new ones; otherwise they are untouched (rows from D on are
// scratch either way).  Wave-uniform arguments; D + dim[i] <= 64.
__device__ bool jc_append(const JcProblem& P, double* Lt, int lane, int i, int j, int& D, double& d2, JcRow& row) {
  const int di = P.dim[i];
  const size_t p = (size_t)i * P.nL + j;
  const int pb = 3 * P.slot[i], lb = 3 * P.nA + 2 * j;
  const int ir[5] = {pb, pb + 1, pb + 2, lb, lb + 1};
  int Dn = D;
  double d2n = d2;
  for (int t = 0; t < di; t++) {
    const int r = Dn;
    double Jr[5];
    for (int k = 0; k < 5; k++) Jr[k] = P.J[10 * p + 5 * t + k];
    const double er = P.e[2 * p + t];
    if (lane == r) {
      for (int k = 0; k < 5; k++) row.J[k] = Jr[k];
      row.pb = pb; row.lb = lb; row.obs = i; row.t = t;
    }
    // entry (r, lane) of C
    double v = 0;
    if (lane <= r) {
      const int ic[5] = {row.pb, row.pb + 1, row.pb + 2, row.lb, row.lb + 1};
      for (int b = 0; b < 5; b++) {
        double u = 0;
        for (int a = 0; a < 5; a++) u += Jr[a] * sig(P.sigma, P.n, ir[a], ic[b]);
        v += u * row.J[b];
      }
      if (row.obs == i) v += P.R[3 * (size_t)i + t + row.t];
    }
    // forward substitution: column k of the new row is final once columns 0 .. k - 1 have been taken out of it
    double acc = er, lrow = 0;
    for (int k = 0; k < r; k++) {
      const double lk = __shfl(v, k) / Lt[k * 64 + k];
      const double yk = __shfl(row.y, k);
      if (lane > k && lane < r) v -= lk * Lt[k * 64 + lane];
      if (lane == r) { v -= lk * lk; acc -= lk * yk; }
      if (lane == k) lrow = lk;
    }
    const double pivot = __shfl(v, r), ae = __shfl(acc, r);
    if (!(pivot > 0) || !(pivot < INFINITY)) return false;
    const double lrr = sqrt(pivot), yr = ae / lrr;
    if (lane < r) Lt[lane * 64 + r] = lrow;
    if (lane == r) { Lt[r * 64 + r] = lrr; row.y = yr; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // (the next row reads this one through other lanes)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    d2n += yr * yr;
    Dn++;
  }
  if (!jc_passes(d2n, P.gamma[Dn])) return false;
  D = Dn;
  d2 = d2n;
  return true;
}

__device__ __forceinline__ bool jc_used(const u64 used[4], int j) { return (used[j >> 6] >> (j & 63)) & 1ull; }
__device__ __forceinline__ void jc_flip(u64 used[4], int j) {
  for (int w = 0; w < 4; w++) used[w] ^= w == (j >> 6) ? 1ull << (j & 63) : 0ull;
}

}  // namespace

// One wavefront.  X.g_assign [nM], X.g_head = (count, dof), X.g_d2.
__global__ __launch_bounds__(64) void k_jc_greedy(JcProblem P, JcWork X) {
  __shared__ double Lt[64 * 64];
  const int lane = threadIdx.x;
  JcRow row;
  u64 used[4] = {0, 0, 0, 0};
  int D = 0, count = 0, mine = -1;
  double d2 = 0;
  for (int i = 0; i < P.nM; i++) {
    const int nc = P.ncand[i];
    for (int q = 0; q < nc; q++) {
      const int j = P.cand[(size_t)i * P.nL + q];
      if (jc_used(used, j)) continue;
      if (!jc_append(P, Lt, lane, i, j, D, d2, row)) continue;
      jc_flip(used, j);
      count++;
      if (lane == i) mine = j;
      break;
    }
  }
  if (lane < P.nM) X.g_assign[lane] = mine;
  if (lane == 0) { X.g_head[0] = count; X.g_head[1] = D; X.g_d2[0] = d2; }
}

// Root (i0, j) = 4 blockIdx.x + wave, as i0 * nL + j.
__global__ __launch_bounds__(256) void k_jc_search(JcProblem P, int round, long long node_limit, long long turn_limit, JcWork X) {
  __shared__ double Lt_all[4][64 * 64];
  __shared__ double st_d2[4][32];
  __shared__ int st_obs[4][32], st_pos[4][32], st_D[4][32], st_j[4][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nM = P.nM, nL = P.nL;
  const int nroot = nM * nL, root = 4 * blockIdx.x + wave;
  if (root >= nroot) return;                                      // (wave-uniform, as everything below; no barrier follows)
  const size_t ro = (size_t)round * nroot + root;
  const int i0 = root / nL, j0 = root - i0 * nL;
  auto nothing = [&]() {
    if (lane == 0) { X.count[ro] = 0; X.dof[ro] = 0; X.d2[ro] = 0.0; X.stopped[ro] = 0; X.nodes[ro] = 0; }
  };
  if (!jc_passes(P.ic[root], P.gamma[P.dim[i0]])) { nothing(); return; }
  // the bound: the greedy hypothesis, and in round 1 the best any root found in round 0
  int bc = X.g_head[0];
  double bd = X.g_d2[0];
  if (round > 0) {
    if (!X.stopped[root]) { nothing(); return; }                  // settled in round 0
    for (int base = 0; base < nroot; base += 64) {
      const int q = base + lane;
      int c = q < nroot ? X.count[q] : 0;
      double d = q < nroot ? X.d2[q] : 0.0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const int c2 = __shfl_xor(c, off);
        const double d2o = __shfl_xor(d, off);
        if (c2 > c || (c2 == c && d2o < d)) { c = c2; d = d2o; }
      }
      if (c > bc || (c == bc && c > 0 && d < bd)) { bc = c; bd = d; }
    }
  }
  // observations from i on that have a candidate at all: bit i of live
  const u64 live = __ballot(lane < nM && P.ncand[lane < nM ? lane : 0] > 0);
  double* Lt = Lt_all[wave];
  JcRow row;
  u64 used[4] = {0, 0, 0, 0};
  int D = 0, mine = -1, found = 0, found_dof = 0, stopped = 0;
  double d2 = 0, found_d2 = 0;
  long long nodes = 1;
  auto record = [&](int count) {
    if (!(count > bc || (count == bc && d2 < bd))) return;
    bc = found = count; bd = found_d2 = d2; found_dof = D;
    if (lane < nM) X.assign[ro * nM + lane] = mine;
  };
  if (!jc_append(P, Lt, lane, i0, j0, D, d2, row)) { nothing(); if (lane == 0) X.nodes[ro] = 1; return; }
  jc_flip(used, j0);
  if (lane == i0) mine = j0;
  int count = 1, i = i0 + 1, pos = 0;
  bool ended = false;                                             // (false behind the loop: the turn bound ran out)
  st_obs[wave][0] = i0; st_j[wave][0] = j0;                        // (level 0 is never popped)
  record(count);
  for (long long turn = 0; turn < turn_limit; turn++) {
    const int left = i < nM ? __popcll(live >> i) : 0;
    const bool dead = i >= nM || count + left < bc || (count + left == bc && !(d2 < bd));
    if (dead) {                                                    // back to the last pairing's observation, its next candidate
      if (count == 1) { ended = true; break; }
      count--;
      const int jo = st_j[wave][count], io = st_obs[wave][count];
      jc_flip(used, jo);
      if (lane == io) mine = -1;
      i = io; pos = st_pos[wave][count]; D = st_D[wave][count]; d2 = st_d2[wave][count];
      continue;
    }
    if (pos >= P.ncand[i]) { i++; pos = 0; continue; }            // observation i stays unpaired
    const int j = P.cand[(size_t)i * nL + pos];
    pos++;
    if (jc_used(used, j)) continue;
    if (nodes >= node_limit) { ended = true; stopped = 1; break; }
    nodes++;
    const int D0 = D;
    const double d20 = d2;
    if (!jc_append(P, Lt, lane, i, j, D, d2, row)) continue;
    st_obs[wave][count] = i; st_j[wave][count] = j; st_pos[wave][count] = pos; st_D[wave][count] = D0; st_d2[wave][count] = d20;
    jc_flip(used, j);
    if (lane == i) mine = j;
    count++;
    record(count);
    i++; pos = 0;
  }
  if (!ended) stopped = 1;
  if (lane == 0) { X.count[ro] = found; X.dof[ro] = found_dof; X.d2[ro] = found_d2; X.stopped[ro] = stopped; X.nodes[ro] = nodes; }
}

// One workgroup.  The key of an entry: count, then -d2, then the lower root, then the earlier round.
__global__ __launch_bounds__(256) void k_jc_best(int nM, int nL, JcWork X) {
  __shared__ int b_cnt[256], b_at[256], b_open[256];
  __shared__ double b_d2[256];
  __shared__ long long b_nodes[256];
  const int tid = threadIdx.x, nroot = nM * nL;
  int cnt = 0, at = -1, open = 0;
  double d2 = 0;
  long long ns = 0;
  for (int r = tid; r < nroot; r += 256) {
    for (int round = 0; round < CGMR_JC_ROUNDS; round++) {
      const int q = round * nroot + r, c = X.count[q];
      const double d = X.d2[q];
      if (c > cnt || (c == cnt && c > 0 && d < d2)) { cnt = c; d2 = d; at = q; }
      ns += X.nodes[q];
    }
    open |= X.stopped[r] ? X.stopped[nroot + r] : 0;
  }
  b_cnt[tid] = cnt; b_at[tid] = at; b_d2[tid] = d2; b_open[tid] = open; b_nodes[tid] = ns;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      const int c = b_cnt[tid + h], a = b_at[tid + h];
      const double d = b_d2[tid + h];
      // (threads hold interleaved roots: the lower root, then the earlier round, by their own numbers)
      const int mr = b_at[tid] % nroot, orr = a % nroot;
      const bool better = a >= 0 && (b_at[tid] < 0 || c > b_cnt[tid] || (c == b_cnt[tid] && (d < b_d2[tid] ||
                          (d == b_d2[tid] && (orr < mr || (orr == mr && a < b_at[tid]))))));
      if (better) { b_cnt[tid] = c; b_at[tid] = a; b_d2[tid] = d; }
      b_open[tid] |= b_open[tid + h];
      b_nodes[tid] += b_nodes[tid + h];
    }
    __syncthreads();
  }
  const int gc = X.g_head[0];
  const double gd = X.g_d2[0];
  const bool beat = b_at[0] >= 0 && b_cnt[0] > 0 && (b_cnt[0] > gc || (b_cnt[0] == gc && b_d2[0] < gd));
  if (tid < nM) X.out_assign[tid] = beat ? X.assign[(size_t)b_at[0] * nM + tid] : X.g_assign[tid];
  if (tid == 0) {
    X.out_head[0] = beat ? b_cnt[0] : gc;
    X.out_head[1] = beat ? X.dof[b_at[0]] : X.g_head[1];
    X.out_head[2] = b_open[0] ? 0 : 1;
    X.out_d2[0] = beat ? b_d2[0] : gd;
    X.out_nodes[0] = b_nodes[0];
  }
}

// ----------------------------------------------------------------------------------- launchers
void launch_jc_sigma(hipStream_t st, int n, const int32_t* col, const double* G, double* sigma) {
  const long long total = (long long)n * n;
  hipLaunchKernelGGL(k_jc_sigma, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, n, col, G, sigma);
}

void launch_jc(hipStream_t st, const JcProblem& P, const JcPredict& G, long long node_limit, const JcWork& X) {
  if (node_limit > (1ll << 40)) node_limit = 1ll << 40;           // (beyond any search; keeps the turn bound in 64 bits)
  // between two tests a root skips at most nL used candidates per observation, leaves at most nM observations unpaired and
  // pops at most nM pairings
  const long long turn_limit = (node_limit + 1) * ((long long)P.nM * (P.nL + 2) + 2);
  const int nroot = P.nM * P.nL;
  hipLaunchKernelGGL(k_jc_pairs, dim3(P.nM), dim3(256), 0, st, P, G);
  hipLaunchKernelGGL(k_jc_greedy, dim3(1), dim3(64), 0, st, P, X);
  for (int round = 0; round < CGMR_JC_ROUNDS; round++)
    hipLaunchKernelGGL(k_jc_search, dim3((nroot + 3) / 4), dim3(256), 0, st, P, round, node_limit, turn_limit, X);
  hipLaunchKernelGGL(k_jc_best, dim3(1), dim3(256), 0, st, P.nM, P.nL, X);
}

}  // namespace cgmr
