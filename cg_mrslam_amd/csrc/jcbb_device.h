// Device side of the joint-compatibility data association of landmark observations (jcbb_kernels.hip; include/cgmr.h:
// cgmr_jcbb_dense, cgmr_joint_compatibility): Neira and Tardos' joint compatibility branch and bound on the joint covariance
// of the observing poses and the candidate landmarks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cgmr {

#define CGMR_JC_ROUNDS 2

// The state vector: the nA observing poses (3 entries each), then the nL candidate landmarks (2 each), n = 3 nA + 2 nL.
// Observation i is made from pose slot[i] in dimension dim[i] (2: EDGE_SE2_XY, 1: EDGE_BEARING_SE2_XY); pair (i, j) has the
// innovation e [2], the Jacobian J [2 x 5] with respect to (x_slot[i], l_j) (a bearing: row 0 alone, the rest zero) and the
// individual distance ic.  R [3 i ..] = (R00, R01, R11) of observation i.  cand [i * nL ..]: the ncand[i] individually
// compatible landmarks of observation i, ascending in (ic, j).
struct JcProblem {
  int nM = 0, nL = 0, nA = 0, n = 0;
  const int32_t *slot = nullptr, *dim = nullptr;
  const double *sigma = nullptr, *R = nullptr, *gamma = nullptr;   // sigma [n * n] row-major, the lower triangle is read
  double *e = nullptr, *J = nullptr, *ic = nullptr;
  int32_t *cand = nullptr, *ncand = nullptr;
};
// The graph form: e and J are predicted from the estimates (poses [3 v ..]) as k_observation_cov predicts them -- observation
// i from vertex obs_pose[i] with the measurement meas [3 i ..], landmark j = vertex lm[j].  Null poses: the dense form, e and J
// are the caller's.
struct JcPredict {
  const double* poses = nullptr;
  const int32_t *obs_pose = nullptr, *lm = nullptr;
  const double* meas = nullptr;
};
// What the search works in.  g_*: the greedy hypothesis (assign [nM], head = count, dof; d2).  [CGMR_JC_ROUNDS][nM * nL], one
// entry per round and root (i0, j) = i0 * nL + j: count (0: nothing better than the bound was found), dof, d2, stopped, nodes,
// and the hypothesis [nM].  out_*: the result -- assign [nM], head = count, dof, proven; d2; the node total.
struct JcWork {
  int32_t *g_assign = nullptr, *g_head = nullptr;
  double* g_d2 = nullptr;
  int32_t *count = nullptr, *dof = nullptr, *stopped = nullptr, *assign = nullptr;
  double* d2 = nullptr;
  long long* nodes = nullptr;
  int32_t *out_assign = nullptr, *out_head = nullptr;
  double* out_d2 = nullptr;
  long long* out_nodes = nullptr;
};

// sigma [n * n] out of the dense lower Gram tiles G (joint_marginals_kernels.hip): col[r] = the column of Y of state entry r
// (4 * the vertex's group + its component), or -1 (fixed / inactive: a zero row and column).  Exactly symmetric.
void launch_jc_sigma(hipStream_t st, int n, const int32_t* col, const double* G, double* sigma);
// k_jc_pairs, k_jc_greedy, CGMR_JC_ROUNDS times k_jc_search, k_jc_best: 3 + CGMR_JC_ROUNDS launches.  nM, nL >= 1,
// node_limit >= 1.
void launch_jc(hipStream_t st, const JcProblem& P, const JcPredict& G, long long node_limit, const JcWork& X);

}  // namespace cgmr
