// HIP kernels (gfx950 / CDNA4) of graduated non-convexity around the Gauss-Newton pass it reuses unchanged.
//
// Reference behaviour: Yang, Antonante, Tzoumas, Carlone, "Graduated Non-Convexity for Robust Spatial Perception" (RA-L 2020)
// and GTSAM's GncOptimizer [recalled: from memory, not read from either source; the contract is tests/ref_gnc.py]:
//   mu0 from the residuals at the start                 -> k_gnc_start_part, k_gnc_start_fold
//   the weights of an outer iteration                   -> k_linearize's GncArgs instances (gn_kernels.hip; gnc_device.h: gnc_weight)
//   cost / partial records, "is this the last one"      -> k_gnc_outer
//   failure, the inner count, the step of mu, done      -> k_gnc_step, k_tr_commit (tr_kernels.hip)
//
// One outer iteration is a fixed launch sequence whatever its outcome (optimize_host.cpp: GncPolicy::outer): linearise with fresh
// weights, assemble, k_gnc_outer, factor, solve, update, k_gnc_step; for every further inner iteration the same with the stored
// weights and without k_gnc_outer; then the commit.  The state (mu, counters, records) lives on the device: the host queues
// outer iterations without reading anything back in between.  Once the call is over, every later launch of a queued iteration
// leaves the poses, the weights, mu and the records alone (k_gnc_step keeps status[0] set, so k_update_poses skips; the
// linearisation stores no weight; k_tr_commit does nothing).  All reductions have a fixed order, and max is order-independent
// anyway: results are bit-reproducible and do not depend on how many iterations a round queues.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gn_device.h"
#include "gnc_device.h"
#include "tr_device.h"

namespace cgmr {

// An edge's candidate for mu0, as a value whose MAXIMUM over the free edges is wanted: GM 2 r / c; TLS -(c / (2 r - c)) where
// 2 r - c > 0 (the minimum of the positive candidates), -inf elsewhere.  Known inliers give the neutral value.
__device__ __forceinline__ double gnc_mu0_candidate(int loss, double r, double c, bool free_edge) {
  if (loss == kGncTls) {
    const double d = 2.0 * r - c;
    return free_edge && d > 0.0 ? -(c / d) : -INFINITY;
  }
  return free_edge ? 2.0 * r / c : 0.0;
}

// One value per workgroup of 256 edges: wave64 shuffles, then the four waves' values through LDS.
__global__ __launch_bounds__(256) void k_gnc_start_part(int nE, const double* __restrict__ r, const double* __restrict__ c,
                                                        const uint8_t* __restrict__ known, const GncState* __restrict__ S,
                                                        double* __restrict__ part) {
  __shared__ double s_m[4];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int loss = S->loss;
  double m = k < nE ? gnc_mu0_candidate(loss, r[k], c[k], known[k] == 0) : gnc_mu0_candidate(loss, 0.0, 1.0, false);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
}

// The second stage: the workgroups' values into mu0 and "nothing to reject".  Only while S->need_init is set.
__global__ __launch_bounds__(kDecideT) void k_gnc_start_fold(int nP, const double* __restrict__ part, GncState* S) {
  __shared__ double sh[kDecideT];
  if (!S->need_init || S->done || S->halted) return;
  const int loss = S->loss;
  double m = gnc_mu0_candidate(loss, 0.0, 1.0, false);
  for (int p = threadIdx.x; p < nP; p += kDecideT) m = fmax(m, part[p]);
  m = block_reduce<true>(m, sh);
  if (threadIdx.x != 0) return;
  const bool nothing = loss == kGncTls ? m == -INFINITY : !(m > 1.0);
  S->nothing = nothing ? 1 : 0;
  S->mu = nothing ? 0.0 : loss == kGncTls ? -m : m;
  S->need_init = 0;
}

// Behind the assembly of an outer iteration's first pass: the chi2 partial sums of its linearisation (sum of w r at x_t) and the
// stored weights into the records of iteration S->iter, and whether this iteration is the last.
__global__ __launch_bounds__(kDecideT) void k_gnc_outer(int nE, int nP, const double* __restrict__ weight,
                                                        const uint8_t* __restrict__ known, const double* __restrict__ part,
                                                        GncState* S, double* __restrict__ rec_mu, double* __restrict__ rec_cost,
                                                        int32_t* __restrict__ rec_partial) {
  __shared__ double sh[kDecideT];
  __shared__ int s_skip;
  if (threadIdx.x == 0) {
    s_skip = S->done || S->halted;
    if (s_skip) S->accept = -1;
  }
  __syncthreads();
  if (s_skip) return;
  double cost = 0.0, np = 0.0;
  for (int p = threadIdx.x; p < nP; p += kDecideT) cost += part[p];
  for (int k = threadIdx.x; k < nE; k += kDecideT) {
    const double w = weight[k];
    if (!known[k] && w > 0.0 && w < 1.0) np += 1.0;              // (a count: exact in double)
  }
  cost = block_reduce<false>(cost, sh);
  np = block_reduce<false>(np, sh);
  if (threadIdx.x != 0) return;
  const int t = S->iter;
  const int partial = (int)np;
  rec_mu[t] = S->nothing ? 0.0 : S->mu;
  rec_cost[t] = cost;
  rec_partial[t] = partial;
  S->last = (S->nothing || (S->loss == kGncTls ? partial == 0 : S->mu == 1.0) || t + 1 >= S->max_outer) ? 1 : 0;
}

// Behind every inner pass.  A bounded wait that ran out (status[2]) halts the state and sends the poses back to the start of
// the outer iteration: the host repeats it with one launch per level, from the same poses and the same mu.  A non-positive
// pivot (status[0]) ends the call: k_update_poses has skipped, the poses are the last good update's.  Otherwise the pass
// counts, and behind the last inner pass the outer iteration ends: mu takes one step (one multiplication or division, in
// double, as the reference does) or the call is done.
__global__ __launch_bounds__(64) void k_gnc_step(GncState* S, int* __restrict__ status, int last_inner) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  // k_assemble's chi2 slot, k_update_poses' counter: per pass.  Also behind the end of the call and in a halted round, whose
  // queued passes still count up: the work space holds the slots of a plain call, not of max_outer * inner_iters passes.
  status[1] = 0;
  if (S->done || S->halted) return;
  if (status[2] != 0) {
    S->halted = 1;
    S->accept = 0;
    return;
  }
  if (status[0] != 0) {
    S->failed = S->inner_total + 1;
    S->iter = S->iter + 1;
    S->done = 1;
    S->accept = -1;
    status[0] = kDoneTag;
    return;
  }
  S->inner_total = S->inner_total + 1;
  if (!last_inner) return;
  S->iter = S->iter + 1;
  S->accept = 1;
  if (S->last) {
    S->done = 1;
    status[0] = kDoneTag;
  } else if (S->loss == kGncTls) {
    S->mu = S->mu * S->factor;
  } else {
    S->mu = fmax(1.0, S->mu / S->factor);
  }
}

void launch_gnc_start(hipStream_t st, const GnDevice& D, const GncDev& G) {
  const int nP = (D.nE + 255) / 256;
  if (nP > 0) hipLaunchKernelGGL(k_gnc_start_part, dim3(nP), dim3(256), 0, st, D.nE, G.r, G.barc_sq, G.known, G.S, G.part);
  hipLaunchKernelGGL(k_gnc_start_fold, dim3(1), dim3(kDecideT), 0, st, nP, G.part, G.S);
}

void launch_gnc_outer(hipStream_t st, const GnDevice& D, const GncDev& G) {
  hipLaunchKernelGGL(k_gnc_outer, dim3(1), dim3(kDecideT), 0, st, D.nE, (D.nE + 255) / 256, G.weight, G.known,
                     D.term + (size_t)33 * D.nE, G.S, G.rec_mu, G.rec_cost, G.rec_partial);
}

void launch_gnc_step(hipStream_t st, const GnDevice& D, const GncDev& G, bool last_inner) {
  hipLaunchKernelGGL(k_gnc_step, dim3(1), dim3(64), 0, st, G.S, D.status, last_inner ? 1 : 0);
}

}  // namespace cgmr
