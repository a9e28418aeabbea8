// Device-resident state of a graduated non-convexity call (gnc_kernels.hip), the weight formulas the linearisation shares with
// it (gn_kernels.hip: GncArgs) and its launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gn_device.h"

namespace cgmr {

constexpr int kGncTls = 0, kGncGm = 1;                            // include/cgmr.h: CGMR_GNC_TLS / CGMR_GNC_GM
// what a GNC linearisation does with the weights (GncArgs::mode)
constexpr int kGncCompute = 0;   // from mu and r at these poses, stored (unless the call is over)
constexpr int kGncReuse = 1;     // the stored ones (later inner iterations, the final statistics)
constexpr int kGncPlain = 2;     // all 1, nothing read or stored (the start's chi-only pass)

// One per call, in device memory, set up by the host (optimize_host.cpp: GncPolicy) and read back once per round.
struct GncState {
  double mu = 0, factor = 1.4;
  int32_t loss = kGncTls, max_outer = 100, inner_iters = 1;
  int32_t iter = 0;          // outer iterations run
  int32_t done = 0;          // 1: the last outer iteration has run, or a factorisation failed -- nothing changes any more
  int32_t halted = 0;        // 1: a bounded wait ran out in a pass: the host repeats the outer iteration
  int32_t accept = -1;       // for k_tr_commit behind an outer iteration: 1 keep, 0 back to its start, -1 nothing
  int32_t need_init = 1;     // mu0 still to be computed
  int32_t nothing = 0;       // 1: nothing to reject -- every weight 1, one outer iteration, mu recorded as 0
  int32_t last = 0;          // the outer iteration under way is the last one (k_gnc_outer's verdict)
  int32_t failed = 0;        // 1 + the inner iteration (counted over the call) whose factorisation met a non-positive pivot
  int32_t inner_total = 0;   // inner iterations applied in this call
};

// The device buffers of a call: records rec_mu / rec_cost / rec_partial [max_outer + 1]; saved poses [3 nV]; per edge the
// weight, barc^2, r = e^T Omega e and the known-inlier mask; the start's per-workgroup values [ceil(nE / 256)].
struct GncDev {
  GncState* S = nullptr;
  double *rec_mu = nullptr, *rec_cost = nullptr, *saved = nullptr;
  int32_t* rec_partial = nullptr;
  double *weight = nullptr, *barc_sq = nullptr, *r = nullptr, *part = nullptr;
  uint8_t* known = nullptr;
};

// The weight of a free edge [recalled from Yang et al., RA-L 2020, and GTSAM's GncOptimizer; the contract is tests/ref_gnc.py].
// Every operation is rounded on its own, in the order the reference writes it (the linearisation's file contracts a * b + c).
__device__ __forceinline__ double gnc_weight(int loss, double mu, double c, double r) {
#pragma clang fp contract(off)
  if (loss == kGncTls) {
    const double up = (mu + 1.0) / mu * c, lo = mu / (mu + 1.0) * c;
    if (r >= up) return 0.0;
    if (r <= lo) return 1.0;
    return sqrt(c * mu * (mu + 1.0) / r) - mu;
  }
  const double mc = mu * c, q = mc / (r + mc);
  return q * q;
}

void launch_gnc_start(hipStream_t st, const GnDevice& D, const GncDev& G);
void launch_gnc_outer(hipStream_t st, const GnDevice& D, const GncDev& G);
void launch_gnc_step(hipStream_t st, const GnDevice& D, const GncDev& G, bool last_inner);

}  // namespace cgmr
