// What the two trust-region iterations (lm_kernels.hip, dl_kernels.hip) share on the device, and the one kernel they share
// on the host side (tr_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gn_symbolic.h"

namespace cgmr {

// n = nV poses, behind a verdict (*accept: 1 accept, 0 restore, -1 nothing -- the field of the call's state): accepted ->
// saved = poses; rejected -> poses = saved, bit for bit
void launch_tr_commit(hipStream_t st, int nV, double* poses, double* saved, const int32_t* accept);

constexpr int kDecideT = 1024;                  // threads of the one-workgroup kernels
constexpr int kDoneTag = 1 << 30;               // status[0] once the call is over: no update applies any more

// fixed-order sum / max over one workgroup of kDecideT threads
template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = kDecideT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = MAX ? fmax(sh[threadIdx.x], sh[threadIdx.x + s]) : sh[threadIdx.x] + sh[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// H + lam I for thread t of 3 nf: lam onto diagonal entry t % 3 of the unmasked diagonal block t / 3, where k_assemble put
// the block (blk_dst: the owning front's panel, or the Ablk slot of a top-block front).  Masked columns keep their identity rows.
__device__ __forceinline__ void damp_diagonal(int t, const int32_t* __restrict__ blk_dst, const uint8_t* __restrict__ cmask,
                                              double* __restrict__ Pan, double* __restrict__ Ablk, double lam) {
  const int c = t / 3, r = t - 3 * c;
  if (cmask[c]) return;
  const int dst = blk_dst[c];
  if (dst >= 0) Pan[(size_t)dst + r * kPanStride + r] += lam;
  else Ablk[(size_t)(-dst - 1) * 9 + 4 * r] += lam;
}

}  // namespace cgmr
