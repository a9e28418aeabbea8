// HIP kernels (gfx950 / CDNA4) of the Levenberg-Marquardt iteration, next to the Gauss-Newton pass they reuse unchanged.
//
// Reference behaviour: g2o's OptimizationAlgorithmLevenberg::solve [g2o-recalled; the contract is tests/ref_lm.py]:
//   computeLambdaInit                                   -> k_lm_init
//   BlockSolver::setLambda (H + lambda I)               -> k_lm_damp
//   computeScale, the rho test, lambda / nu, push / pop -> k_lm_decide, k_tr_commit (tr_kernels.hip)
//
// One trial is a fixed launch sequence whatever its outcome (optimize_host.cpp: LmPolicy::trial): linearise, assemble, [init,] damp,
// factor, solve, update, chi-only linearise, decide, commit.  Re-linearising at unchanged poses yields the same terms bit for
// bit, so a rejected trial needs nothing but the restored poses.  The state (lambda, nu, counters, records) lives on the
// device: the host queues trials without reading anything back in between.  Once the call has terminated, every later
// launch of a queued trial leaves the poses, the state and the records alone (k_lm_decide keeps status[0] set, so
// k_update_poses skips; k_tr_commit does nothing).  All reductions have a fixed order: results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>

#include "gn_device.h"
#include "gn_symbolic.h"
#include "lm_device.h"
#include "tr_device.h"

namespace cgmr {

// lambda = initialLambda if > 0, else tau * max |H_jj| over the unmasked diagonal (H as k_assemble left it: undamped, before
// the children's contributions, which only the factorisation adds).  Only while S->need_init is set: the first trial of a call.
__global__ __launch_bounds__(kDecideT) void k_lm_init(int nf, const int32_t* __restrict__ blk_dst, const uint8_t* __restrict__ cmask,
                                                      const double* __restrict__ Pan, const double* __restrict__ Ablk, LmState* S) {
  __shared__ double sh[kDecideT];
  if (!S->need_init || S->done || S->halted) return;
  double m = 0.0;
  for (int t = threadIdx.x; t < 3 * nf; t += kDecideT) {
    const int c = t / 3, r = t - 3 * c;
    if (cmask[c]) continue;
    const int dst = blk_dst[c];
    const double h = dst >= 0 ? Pan[(size_t)dst + r * kPanStride + r] : Ablk[(size_t)(-dst - 1) * 9 + 4 * r];
    m = fmax(m, fabs(h));
  }
  m = block_reduce<true>(m, sh);
  if (threadIdx.x == 0) {
    S->lambda = S->initial_lambda > 0 ? S->initial_lambda : S->tau * m;
    S->nu = 2.0;
    S->need_init = 0;
  }
}

// H + lambda I on the unmasked diagonal (tr_device.h: damp_diagonal)
__global__ __launch_bounds__(256) void k_lm_damp(int nf, const int32_t* __restrict__ blk_dst, const uint8_t* __restrict__ cmask,
                                                 double* __restrict__ Pan, double* __restrict__ Ablk, const LmState* __restrict__ S) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * nf) return;
  damp_diagonal(t, blk_dst, cmask, Pan, Ablk, S->lambda);
}

// The trial's verdict.  currentChi: chi2 at x (k_assemble's slot 0); tempChi: the chi-only linearisation's partial sums at
// x' (DBL_MAX when the factorisation failed: status[0]); scale = sum_j dx_j (lambda dx_j + b_j) + 1e-3 over the permuted
// x / b (masked columns: dx = b = 0).  A failed factorisation leaves x garbage: rho = -inf, a reject, whatever scale says.
// A bounded wait that ran out (status[2]) is no verdict at all: the state halts, the poses are restored, and the host repeats
// the trial with one launch per level.
__global__ __launch_bounds__(kDecideT) void k_lm_decide(int nf, int nP, const double* __restrict__ part, const double* __restrict__ xvec,
                                                        const double* __restrict__ bvec, const double* __restrict__ chi_slot,
                                                        int* __restrict__ status, LmState* S, double* __restrict__ rec_chi,
                                                        double* __restrict__ rec_lambda, int32_t* __restrict__ rec_trials) {
  __shared__ double sh[kDecideT];
  __shared__ int s_skip;
  if (threadIdx.x == 0) {
    s_skip = S->done || S->halted || status[2] != 0;
    if (s_skip) {
      if (!S->done && !S->halted) { S->halted = 1; S->accept = 0; }   // (time-out: restore x; status[0] stays set)
      else S->accept = -1;
      status[1] = 0;
    }
  }
  __syncthreads();
  if (s_skip) return;
  const bool failed = status[0] != 0;
  const double lam = S->lambda;
  double tc = 0.0, sc = 0.0;
  for (int k = threadIdx.x; k < nP; k += kDecideT) tc += part[k];
  if (!failed)
    for (int j = threadIdx.x; j < 3 * nf; j += kDecideT) sc += xvec[j] * (lam * xvec[j] + bvec[j]);
  tc = block_reduce<false>(tc, sh);
  sc = block_reduce<false>(sc, sh);
  if (threadIdx.x != 0) return;
  const int q = S->trial, i = S->iter;
  double cur = chi_slot[0];
  if (q == 0) rec_chi[i] = cur;
  const double temp = failed ? DBL_MAX : tc;
  const double rho = failed ? -INFINITY : (cur - temp) / (sc + 1e-3);
  const bool accept = rho > 0 && isfinite(temp);
  double lambda = lam, nu = S->nu;
  if (accept) {
    const double a = 2 * rho - 1;
    double alpha = 1.0 - a * a * a;
    alpha = fmin(alpha, S->upper);
    lambda *= fmax(S->lower, alpha);
    nu = 2.0;
    cur = temp;
  } else {
    lambda *= nu;
    nu *= 2.0;
  }
  S->lambda = lambda;
  S->nu = nu;
  S->accept = accept ? 1 : 0;
  S->total_trials++;
  const bool brk = !accept && !isfinite(lambda);
  if (!brk && rho < 0 && q + 1 < S->max_trials) {
    S->trial = q + 1;
  } else {                                             // the iteration ends
    rec_lambda[i] = lambda;
    rec_trials[i] = q + 1;
    rec_chi[i + 1] = cur;
    const bool term = q + 1 >= S->max_trials || rho == 0 || !isfinite(lambda);
    S->iter = i + 1;
    S->trial = 0;
    S->terminated = term ? 1 : 0;
    if (term || i + 1 >= S->iters) S->done = 1;
  }
  status[0] = S->done ? kDoneTag : 0;                  // (a failure tag is consumed: the next trial factors afresh)
  status[1] = 0;                                       // k_assemble's chi2 slot, k_update_poses' counter: per trial
}

void launch_lm_init(hipStream_t st, const GnDevice& D, LmState* S) {
  hipLaunchKernelGGL(k_lm_init, dim3(1), dim3(kDecideT), 0, st, D.nf, D.blk_dst, D.cmask, D.Pan, D.Ablk, S);
}

void launch_lm_damp(hipStream_t st, const GnDevice& D, const LmState* S) {
  if (D.nf <= 0) return;
  hipLaunchKernelGGL(k_lm_damp, dim3((3 * D.nf + 255) / 256), dim3(256), 0, st, D.nf, D.blk_dst, D.cmask, D.Pan, D.Ablk, S);
}

void launch_lm_decide(hipStream_t st, const GnDevice& D, const LmDev& L) {
  hipLaunchKernelGGL(k_lm_decide, dim3(1), dim3(kDecideT), 0, st, D.nf, (D.nE + 255) / 256, D.term + (size_t)33 * D.nE, D.xvec, D.bvec,
                     D.chi2, D.status, L.S, L.rec_chi, L.rec_lambda, L.rec_trials);
}

}  // namespace cgmr
