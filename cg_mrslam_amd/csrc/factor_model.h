// The factor model of the edge linearisation, written once: the edge kinds by name, a kind's dimension and its error, and the
// pieces k_linearize (gn_kernels.hip) and k_linearize_chordal (init_kernels.hip) share -- the edge prologue, the workgroup's
// chi2 partial sum and the record stream-out.  Everything is header-inlined and takes the including file's -ffp-contract flag;
// the expressions keep the shape the parity tests pin.
//
// Edge kinds (g2o's slam2d factor types, include/cgmr.h: cgmr_factor_types); (rx, ry, rth) = x_i^-1 x_j:
//   CGMR_EDGE_SE2             pose i -> pose j:     e = (R(z_th)^T ((rx, ry) - z_t), normalize(rth - z_th))
//   CGMR_EDGE_SE2_XY          pose i sees point l:  e = (rx, ry) - z (2)
//   CGMR_EDGE_BEARING_SE2_XY  pose i sees point l:  e = normalize(atan2(ry, rx) - z0) (1), 0 with the point on the pose
//   CGMR_EDGE_PRIOR_SE2       unary (i == j):       e = (R(z_th)^T (t_i - z_t), normalize(th_i - z_th))
//   CGMR_EDGE_PRIOR_SE2_XY    unary (i == j):       e = t_i - z (2)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cgmr.h"

namespace cgmr {

// dimension of an edge kind's factor: the leading entries of its error, measurement and information that count
__host__ __device__ constexpr int factor_dim(int kind) {
  return kind == CGMR_EDGE_BEARING_SE2_XY ? 1 : (kind == CGMR_EDGE_SE2_XY || kind == CGMR_EDGE_PRIOR_SE2_XY) ? 2 : 3;
}
// a prior: an edge from a vertex to itself (no assembly key: k_add_unary)
__host__ __device__ constexpr bool factor_is_prior(int kind) { return kind >= CGMR_EDGE_PRIOR_SE2; }

__device__ __forceinline__ double d_normalize_theta(double t) {
  const double pi = 3.14159265358979323846;
  if (t >= -pi && t < pi) return t;
  double m = floor((t + pi) / (2 * pi));
  return t - 2 * pi * m;
}

// e of factor kind fk with measurement (z0, z1, z2), (cz, sz) = (cos z2, sin z2), from what the linearisation has of the two
// vertices: (rx, ry, rth) = x_i^-1 x_j, x_i itself for the priors.  Components beyond the factor's dimension are exact zeros.
__device__ __forceinline__ void factor_error(int fk, double rx, double ry, double rth, double xi0, double xi1, double xi2, double z0,
                                             double z1, double z2, double cz, double sz, double e[3]) {
  const double tx = rx - z0, ty = ry - z1;
  e[0] = cz * tx + sz * ty; e[1] = -sz * tx + cz * ty; e[2] = d_normalize_theta(rth - z2);
  if (fk == CGMR_EDGE_SE2_XY) { e[0] = tx; e[1] = ty; e[2] = 0.0; }
  else if (fk == CGMR_EDGE_BEARING_SE2_XY) {
    e[0] = d_normalize_theta((rx * rx + ry * ry > 0.0 ? atan2(ry, rx) : 0.0) - z0); e[1] = 0.0; e[2] = 0.0;
  } else if (fk == CGMR_EDGE_PRIOR_SE2) {
    const double px = xi0 - z0, py = xi1 - z1;
    e[0] = cz * px + sz * py; e[1] = -sz * px + cz * py; e[2] = d_normalize_theta(xi2 - z2);
  } else if (fk == CGMR_EDGE_PRIOR_SE2_XY) { e[0] = xi0 - z0; e[1] = xi1 - z1; e[2] = 0.0; }
}

// ------------------------------------------------------ shared by k_linearize and k_linearize_chordal
// One thread per edge, 256 per workgroup.  Edges [0, nA) take their measurement / information from (meas, info), edges
// [nA, nE) from (meas_b, info_b); edges [n_active, nE) are switched off (live = k0 < n_active).  The idle lanes of the last workgroup shadow the last edge.
constexpr int kRecordDoubles = 33;
constexpr int kRecordLds = 256 * kRecordDoubles * (int)sizeof(double);   // dynamic LDS of a pass that writes records (above 64 KB)

// edge k's entry of a per-edge array of n doubles each that is split at nA: (a, b) = (meas, meas_b) or (info, info_b)
// (k_linearize's information pointer is this line by hand: through the function its robust instances got other instructions)
__device__ __forceinline__ const double* edge_split(int k, int nA, const double* a, const double* b, int n) {
  return k < nA ? a + n * (size_t)k : b + n * (size_t)(k - nA);
}
// what edge k joins: the estimates of its two vertices and its measurement.  (The three lines in front -- the lane's edge k0,
// live, the shadowed k -- stay in the kernels: moved in here they changed the register allocation of the plain instances.)
struct EdgeEnds { double xi0, xi1, xi2, xj0, xj1, xj2, z0, z1, z2; };
__device__ __forceinline__ EdgeEnds edge_prologue(int k, int nA, const double* poses, const int32_t* ef, const int32_t* et,
                                                  const double* meas, const double* meas_b) {
  EdgeEnds L;
  const int i = ef[k], j = et[k];
  L.xi0 = poses[3 * i]; L.xi1 = poses[3 * i + 1]; L.xi2 = poses[3 * i + 2];
  L.xj0 = poses[3 * j]; L.xj1 = poses[3 * j + 1]; L.xj2 = poses[3 * j + 2];
  const double* zp = edge_split(k, nA, meas, meas_b, 3);
  L.z0 = zp[0]; L.z1 = zp[1]; L.z2 = zp[2];
  return L;
}

// the workgroup's chi2 partial sum into term[33 nE + blockIdx.x], in a fixed order: bit-reproducible.  s_chi: 4 doubles of LDS.
__device__ __forceinline__ void block_chi2_partial(double ch, double* s_chi, double* term, size_t nE) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) ch += __shfl_xor(ch, m, 64);
  if ((threadIdx.x & 63) == 0) s_chi[threadIdx.x >> 6] = ch;
  __syncthreads();
  if (threadIdx.x == 0) term[kRecordDoubles * nE + blockIdx.x] = (s_chi[0] + s_chi[1]) + (s_chi[2] + s_chi[3]);
}

// the workgroup's 256 records, staged in LDS (s_t: [256][33]), out as one contiguous stream (a thread writing its own 264-byte
// record produced 1.5x the bytes at the memory side in partial lines).  The last statement of a kernel; a macro, because as an
// inlined function the loop's exit block lands elsewhere and the schedule of the plain instances changes.
#define CGMR_RECORDS_STREAM_OUT(s_t, term, nE)                                           \
  {                                                                                      \
    __syncthreads();                                                                     \
    const int e0 = blockIdx.x * 256, ne = min(256, (nE) - e0);                           \
    double* out = (term) + (size_t)e0 * kRecordDoubles;                                  \
    for (int q = threadIdx.x; q < ne * kRecordDoubles; q += 256) out[q] = (s_t)[q];      \
  }

}  // namespace cgmr
