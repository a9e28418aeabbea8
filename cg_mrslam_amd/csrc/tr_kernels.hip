// HIP kernel (gfx950 / CDNA4) both trust-region iterations end a trial with: keep the step or take it back.
#include "tr_device.h"

namespace cgmr {

__global__ __launch_bounds__(256) void k_tr_commit(int n, double* __restrict__ poses, double* __restrict__ saved,
                                                   const int32_t* __restrict__ accept) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int a = *accept;
  if (a == 1) saved[t] = poses[t];
  else if (a == 0) poses[t] = saved[t];
}

void launch_tr_commit(hipStream_t st, int nV, double* poses, double* saved, const int32_t* accept) {
  if (nV <= 0) return;
  hipLaunchKernelGGL(k_tr_commit, dim3((3 * nV + 255) / 256), dim3(256), 0, st, 3 * nV, poses, saved, accept);
}

}  // namespace cgmr
