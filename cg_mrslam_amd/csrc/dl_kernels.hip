// HIP kernels (gfx950 / CDNA4) of the dogleg iteration, next to the Gauss-Newton pass they reuse unchanged.
//
// Reference behaviour: g2o's OptimizationAlgorithmDogleg::solve [g2o-recalled; the contract is tests/ref_dogleg.py]:
//   BlockSolver::setLambda while H has not been PD        -> k_dl_damp
//   multiplyHessian (b^T H b, h^T H h)                    -> k_dl_quad, from the edges' term records
//   alpha, hsd, the damping loop's bookkeeping            -> k_dl_begin
//   the GN / SD / DL choice                               -> k_dl_step
//   rho, the trust region, push / pop                     -> k_dl_decide, k_tr_commit (tr_kernels.hip)
//
// An iteration is a head and one or more tails (optimize_host.cpp: DlPolicy).  Head: linearise, assemble, [damp,] factor, solve
// (no pose update), k_dl_quad(b), k_dl_begin.  Tail: k_dl_step, k_dl_quad(h), update, chi-only linearise, k_dl_decide,
// k_tr_commit.  A rejected trial changes delta only, so the next tail mixes the same saved hgn and hsd again: no
// factorisation.  The term records k_linearize left at x stay valid through the tails (the chi-only linearisation returns
// before it writes them), and b stays in bvec through the solve.  The state lives on the device, so the host queues heads
// and tails without reading anything back in between:
//   - a tail does nothing unless an iteration is open (S->solved): k_dl_step keeps status[0] set, so k_update_poses skips;
//     k_dl_decide and k_tr_commit leave the state, the records and the poses alone;
//   - a head behind an open iteration is stale: x is bit-identical to what the open iteration started from (its rejected
//     trials restored it), so its terms and b are the same; k_dl_begin leaves hgn, hsd and the state alone;
//   - a head whose damped factorisation failed leaves the iteration unsolved: the next head retries with the grown lambda.
// All reductions have a fixed order: results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>

#include "dl_device.h"
#include "gn_device.h"
#include "gn_symbolic.h"
#include "tr_device.h"

namespace cgmr {

namespace {

constexpr int kIdleTag = (1 << 30) + 1;         // status[0] in a tail with no open iteration: its update does nothing
constexpr int kStepGN = 2, kStepSD = 1, kStepDL = 3;   // include/cgmr.h: CGMR_DL_STEP_*

}  // namespace

__global__ __launch_bounds__(256) void k_dl_damp(int nf, const int32_t* __restrict__ blk_dst, const uint8_t* __restrict__ cmask,
                                                 double* __restrict__ Pan, double* __restrict__ Ablk, const DlState* __restrict__ S) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * nf) return;
  if (S->was_pd || S->solved || S->done || S->halted) return;
  damp_diagonal(t, blk_dst, cmask, Pan, Ablk, S->lambda);
}

// v^T H v = sum over the edges of vi^T Hii vi + 2 vi^T Hij vj + vj^T Hjj vj, from the 33-double term records (k_linearize:
// Hii 0..8, Hij 9..17, Hjj 18..26, scaled by the robust weight; switched-off edges hold zeros).  One thread per edge; the
// workgroup's sum goes to qpart[blockIdx.x] (waves by shuffles, then the four waves in a fixed order).
__global__ __launch_bounds__(256) void k_dl_quad(int nE, const int32_t* __restrict__ ef, const int32_t* __restrict__ et,
                                                 const int32_t* __restrict__ vperm, const uint8_t* __restrict__ cmask,
                                                 const double* __restrict__ term, const double* __restrict__ v,
                                                 double* __restrict__ qpart) {
  __shared__ double s_q[4];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  double q = 0.0;
  if (k < nE) {
    const int ci = vperm[ef[k]], cj = vperm[et[k]];
    double vi[3] = {0, 0, 0}, vj[3] = {0, 0, 0};
    if (ci >= 0 && !cmask[ci]) for (int r = 0; r < 3; r++) vi[r] = v[3 * (size_t)ci + r];
    if (cj >= 0 && !cmask[cj]) for (int r = 0; r < 3; r++) vj[r] = v[3 * (size_t)cj + r];
    const double* T = term + (size_t)k * 33;
    double a = 0, m = 0, c = 0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      a += vi[r] * (T[3 * r] * vi[0] + T[3 * r + 1] * vi[1] + T[3 * r + 2] * vi[2]);
      m += vi[r] * (T[9 + 3 * r] * vj[0] + T[9 + 3 * r + 1] * vj[1] + T[9 + 3 * r + 2] * vj[2]);
      c += vj[r] * (T[18 + 3 * r] * vj[0] + T[18 + 3 * r + 1] * vj[1] + T[18 + 3 * r + 2] * vj[2]);
    }
    q = a + 2 * m + c;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) q += __shfl_xor(q, s, 64);
  if ((threadIdx.x & 63) == 0) s_q[threadIdx.x >> 6] = q;
  __syncthreads();
  if (threadIdx.x == 0) qpart[blockIdx.x] = (s_q[0] + s_q[1]) + (s_q[2] + s_q[3]);
}

// After a head's solve (xvec = hgn, or garbage when the factorisation failed: status[0]; bvec = b; qpart: b^T H b).
// A time-out (status[2]) halts the call: the host repeats from the state as it stands with one launch per level.
__global__ __launch_bounds__(kDecideT) void k_dl_begin(int nf, int nP, const double* __restrict__ qpart, const double* __restrict__ bvec,
                                                       const double* __restrict__ xvec, const uint8_t* __restrict__ cmask,
                                                       const double* __restrict__ chi_slot, const int* __restrict__ status, DlState* S,
                                                       double* __restrict__ hgn, double* __restrict__ hsd, double* __restrict__ rec_chi) {
  __shared__ double sh[kDecideT];
  __shared__ int s_go;
  if (threadIdx.x == 0) {
    int go = !S->done && !S->halted;
    if (go && status[2] != 0) { S->halted = 1; go = 0; }
    if (go && S->solved) go = 0;                         // a stale head: the open iteration keeps its hgn / hsd
    if (go) {
      S->factorisations++;
      rec_chi[S->iter] = chi_slot[0];
      const bool ok = status[0] == 0;
      const bool was_pd = S->was_pd && ok;
      double lam = S->lambda;
      if (!was_pd) {
        if (ok) {
          lam = fmax(1e-12, lam / (0.5 * S->lambda_factor));
        } else {
          lam *= S->lambda_factor;
          if (lam > 1e3) { lam = 1e3; S->failed = 1; S->done = 1; }
        }
      }
      S->was_pd = was_pd ? 1 : 0;
      S->lambda = lam;
      if (!ok) go = 0;                                   // (the next head retries with the grown lambda)
    }
    s_go = go;
  }
  __syncthreads();
  if (!s_go) return;
  double bb = 0, hh = 0, bhb = 0;
  for (int j = threadIdx.x; j < 3 * nf; j += kDecideT) {
    const double bj = bvec[j], xj = xvec[j];
    bb += bj * bj;
    hh += xj * xj;
    hgn[j] = xj;
  }
  for (int k = threadIdx.x; k < nP; k += kDecideT) bhb += qpart[k];
  bb = block_reduce<false>(bb, sh);
  hh = block_reduce<false>(hh, sh);
  bhb = block_reduce<false>(bhb, sh);
  const double alpha = bb / bhb;                        // (b = 0: 0 / 0, as in g2o)
  double ss = 0;
  for (int j = threadIdx.x; j < 3 * nf; j += kDecideT) {
    const double s = cmask[j / 3] ? 0.0 : alpha * bvec[j];
    hsd[j] = s;
    ss += s * s;
  }
  ss = block_reduce<false>(ss, sh);
  if (threadIdx.x == 0) {
    S->hgn_norm = sqrt(hh);
    S->hsd_norm = sqrt(ss);
    S->cur_chi = chi_slot[0];
    S->trial = 0;
    S->solved = 1;
  }
}

__global__ __launch_bounds__(kDecideT) void k_dl_step(int nf, const double* __restrict__ bvec, const double* __restrict__ hgn,
                                                      const double* __restrict__ hsd, double* __restrict__ xvec,
                                                      int* __restrict__ status, DlState* S) {
  __shared__ double sh[kDecideT];
  __shared__ int s_go;
  if (threadIdx.x == 0) {
    s_go = !S->done && !S->halted && S->solved;
    if (!s_go) status[0] = kIdleTag;
  }
  __syncthreads();
  if (!s_go) return;
  const double delta = S->delta, gn = S->hgn_norm, sd = S->hsd_norm;
  const int kind = gn < delta ? kStepGN : sd > delta ? kStepSD : kStepDL;
  double beta = 0;
  if (kind == kStepDL) {
    double c = 0, bma = 0, s2 = 0;
    for (int j = threadIdx.x; j < 3 * nf; j += kDecideT) {
      const double a = hgn[j] - hsd[j];
      c += hsd[j] * a;
      bma += a * a;
      s2 += hsd[j] * hsd[j];
    }
    c = block_reduce<false>(c, sh);
    bma = block_reduce<false>(bma, sh);
    s2 = block_reduce<false>(s2, sh);
    if (c <= 0) beta = (-c + sqrt(c * c + bma * (delta * delta - s2))) / bma;
    else beta = (delta * delta - s2) / (c + sqrt(c * c + bma * (delta * delta - s2)));
  }
  const double sc = delta / sd;
  double bh = 0, hh = 0;
  for (int j = threadIdx.x; j < 3 * nf; j += kDecideT) {
    const double h = kind == kStepGN ? hgn[j] : kind == kStepSD ? sc * hsd[j] : hsd[j] + beta * (hgn[j] - hsd[j]);
    xvec[j] = h;
    bh += bvec[j] * h;
    hh += h * h;
  }
  bh = block_reduce<false>(bh, sh);
  hh = block_reduce<false>(hh, sh);
  if (threadIdx.x == 0) {
    S->bh = bh;
    S->h_norm = sqrt(hh);
    S->step = kind;
    status[0] = 0;                                       // (the update applies the step)
  }
}

// The trial's verdict: qpart holds h^T H h, part the chi-only linearisation's chi2 partial sums at x (+) h.
__global__ __launch_bounds__(kDecideT) void k_dl_decide(int nP, const double* __restrict__ part, const double* __restrict__ qpart,
                                                        int* __restrict__ status, DlState* S, double* __restrict__ rec_chi,
                                                        double* __restrict__ rec_delta, int32_t* __restrict__ rec_trials,
                                                        int32_t* __restrict__ rec_step) {
  __shared__ double sh[kDecideT];
  __shared__ int s_go;
  if (threadIdx.x == 0) {
    s_go = !S->done && !S->halted && S->solved;
    if (!s_go) {
      S->accept = -1;
      status[0] = (S->done || S->halted) ? kDoneTag : 0;
      status[1] = 0;
    }
  }
  __syncthreads();
  if (!s_go) return;
  double tc = 0, hq = 0;
  for (int k = threadIdx.x; k < nP; k += kDecideT) { tc += part[k]; hq += qpart[k]; }
  tc = block_reduce<false>(tc, sh);
  hq = block_reduce<false>(hq, sh);
  if (threadIdx.x != 0) return;
  const double cur = S->cur_chi;
  double lin = -1 * hq + 2 * S->bh;
  if (fabs(lin) < 1e-12) lin = 1e-12;
  const double rho = (cur - tc) / lin;
  const bool good = rho > 0;
  double delta = S->delta;
  if (rho > 0.75) delta = fmax(delta, 3. * S->h_norm);
  else if (rho < 0.25) delta *= 0.5;
  S->delta = delta;
  S->accept = good ? 1 : 0;
  S->total_trials++;
  const int q = S->trial + 1, i = S->iter;
  if (good || q >= S->max_trials) {                     // the iteration ends
    const double chi = good ? tc : cur;
    rec_delta[i] = delta;
    rec_trials[i] = q;
    rec_step[i] = S->step;
    rec_chi[i + 1] = chi;
    const bool term = q == S->max_trials || !good;
    S->cur_chi = chi;
    S->iter = i + 1;
    S->trial = 0;
    S->solved = 0;
    S->terminated = term ? 1 : 0;
    if (term || i + 1 >= S->iters) S->done = 1;
  } else {
    S->trial = q;
  }
  status[0] = S->done ? kDoneTag : 0;
  status[1] = 0;                                         // k_assemble's chi2 slot, k_update_poses' counter: per trial
}

void launch_dl_damp(hipStream_t st, const GnDevice& D, const DlState* S) {
  if (D.nf <= 0) return;
  hipLaunchKernelGGL(k_dl_damp, dim3((3 * D.nf + 255) / 256), dim3(256), 0, st, D.nf, D.blk_dst, D.cmask, D.Pan, D.Ablk, S);
}

void launch_dl_quad(hipStream_t st, const GnDevice& D, const double* v, double* qpart) {
  if (D.nE <= 0) return;
  hipLaunchKernelGGL(k_dl_quad, dim3((D.nE + 255) / 256), dim3(256), 0, st, D.nE, D.ef, D.et, D.vperm, D.cmask, D.term, v, qpart);
}

void launch_dl_begin(hipStream_t st, const GnDevice& D, const DlDev& L) {
  hipLaunchKernelGGL(k_dl_begin, dim3(1), dim3(kDecideT), 0, st, D.nf, (D.nE + 255) / 256, L.qpart, D.bvec, D.xvec, D.cmask, D.chi2,
                     D.status, L.S, L.hgn, L.hsd, L.rec_chi);
}

void launch_dl_step(hipStream_t st, const GnDevice& D, const DlDev& L) {
  hipLaunchKernelGGL(k_dl_step, dim3(1), dim3(kDecideT), 0, st, D.nf, D.bvec, L.hgn, L.hsd, D.xvec, D.status, L.S);
}

void launch_dl_decide(hipStream_t st, const GnDevice& D, const DlDev& L) {
  hipLaunchKernelGGL(k_dl_decide, dim3(1), dim3(kDecideT), 0, st, (D.nE + 255) / 256, D.term + (size_t)33 * D.nE, L.qpart, D.status,
                     L.S, L.rec_chi, L.rec_delta, L.rec_trials, L.rec_step);
}

}  // namespace cgmr
