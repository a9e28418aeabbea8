// Device-resident state of a Levenberg-Marquardt call (lm_kernels.hip) and its launchers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "gn_device.h"

namespace cgmr {

// One per call, in device memory, set up by the host before the first trial (optimize_host.cpp: tr_run) and read back once per round.
struct LmState {
  double lambda = 0, nu = 2;                 // current damping and its growth factor on a reject
  double tau = 1e-5, initial_lambda = -1;    // g2o's properties (initial_lambda <= 0: tau * max |H_jj|)
  double lower = 1.0 / 3, upper = 2.0 / 3;   // goodStepLowerScale / goodStepUpperScale
  int32_t max_trials = 10;                   // maxTrialsAfterFailure
  int32_t iters = 0;                         // outer iterations asked for
  int32_t iter = 0;                          // outer iterations run (g2o's count: a terminating one included)
  int32_t trial = 0;                         // trials of the current iteration so far
  int32_t done = 0;                          // 1: terminated or every iteration run -- nothing changes any more
  int32_t terminated = 0;                    // 1: g2o's Terminate (trial limit, rho == 0, lambda not finite)
  int32_t halted = 0;                        // 1: a bounded wait ran out in a trial: the host repeats it
  int32_t need_init = 1;                     // lambda still to be computed (first trial of the call)
  int32_t accept = -1;                       // verdict of the last trial for k_tr_commit: 1 accept, 0 restore, -1 nothing
  int32_t total_trials = 0;                  // trials decided in this call
};

// The device buffers of a call: records rec_chi [iters + 1], rec_lambda / rec_trials [iters]; saved poses [3 nV].
struct LmDev {
  LmState* S = nullptr;
  double *rec_chi = nullptr, *rec_lambda = nullptr, *saved = nullptr;
  int32_t* rec_trials = nullptr;
};

void launch_lm_init(hipStream_t st, const GnDevice& D, LmState* S);
void launch_lm_damp(hipStream_t st, const GnDevice& D, const LmState* S);
void launch_lm_decide(hipStream_t st, const GnDevice& D, const LmDev& L);

}  // namespace cgmr
