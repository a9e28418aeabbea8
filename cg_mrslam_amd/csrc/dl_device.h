// Device-resident state of a dogleg call (dl_kernels.hip) and its launchers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "gn_device.h"

namespace cgmr {

// One per call, in device memory, set up by the host before the first head (optimize_host.cpp: tr_run) and read back once per round.
struct DlState {
  double delta = 1e4;                        // trust-region radius
  double lambda = 1e-7;                      // currentLambda: the damping once H has not been positive definite
  double lambda_factor = 10;                 // g2o's lamdbaFactor
  double cur_chi = 0;                        // currentChi of the open iteration (after an accepted step: its chi2)
  double hsd_norm = 0, hgn_norm = 0;         // |hsd|, |hgn| of the open iteration
  double h_norm = 0, bh = 0;                 // |h| and b^T h of the current trial's step
  int32_t max_trials = 100;                  // maxTrialsAfterFailure
  int32_t iters = 0;                         // outer iterations asked for
  int32_t iter = 0;                          // outer iterations decided (g2o's count: a terminating one included)
  int32_t trial = 0;                         // trials of the open iteration so far
  int32_t was_pd = 1;                        // _wasPDInAllIterations
  int32_t solved = 0;                        // 1: the open iteration has its Gauss-Newton step (hgn, hsd saved): tails run trials
  int32_t done = 0;                          // 1: terminated, failed or every iteration run -- nothing changes any more
  int32_t terminated = 0;                    // 1: g2o's Terminate (trial limit, or no good step)
  int32_t failed = 0;                        // 1: g2o's Fail (currentLambda above 1e3 with H + lambda I still not PD)
  int32_t halted = 0;                        // 1: a bounded wait ran out in a head: the host repeats it
  int32_t step = 0;                          // CGMR_DL_STEP_* of the current trial
  int32_t accept = -1;                       // verdict of the last tail for k_tr_commit: 1 keep, 0 restore, -1 nothing
  int32_t total_trials = 0;                  // trials decided in this call
  int32_t factorisations = 0;                // heads that served an iteration (a failed damped factorisation included)
};

// The device buffers of a call: records rec_chi [iters + 1], rec_delta / rec_trials / rec_step [iters]; saved poses [3 nV];
// the open iteration's hgn / hsd [3 nf] (permuted columns); the partial sums of k_dl_quad [(nE + 255) / 256].
struct DlDev {
  DlState* S = nullptr;
  double *rec_chi = nullptr, *rec_delta = nullptr, *saved = nullptr, *hgn = nullptr, *hsd = nullptr, *qpart = nullptr;
  int32_t *rec_trials = nullptr, *rec_step = nullptr;
};

// H + currentLambda I on the free diagonal, only while a head serves an iteration and H has not been PD
void launch_dl_damp(hipStream_t st, const GnDevice& D, const DlState* S);
// per-workgroup partial sums of v^T H v over the edges' term records (v: permuted columns, masked ones count as zero)
void launch_dl_quad(hipStream_t st, const GnDevice& D, const double* v, double* qpart);
// after a head's solve: the damping bookkeeping, alpha, hsd, hgn (leaves a stale head's iteration alone)
void launch_dl_begin(hipStream_t st, const GnDevice& D, const DlDev& L);
// per tail: the step for the current delta into D.xvec (for launch_update), b^T h, |h|
void launch_dl_step(hipStream_t st, const GnDevice& D, const DlDev& L);
// per tail: rho, the verdict, delta, termination, the records
void launch_dl_decide(hipStream_t st, const GnDevice& D, const DlDev& L);

}  // namespace cgmr
