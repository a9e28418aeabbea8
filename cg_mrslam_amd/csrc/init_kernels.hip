// HIP kernels (gfx950 / CDNA4) of chordal initialisation: a starting point from two linear least-squares problems, solved by the
// Gauss-Newton pass's own assembly, factorisation and solves (gn_kernels.hip), which run unchanged.
//
// Reference behaviour: chordal relaxation as in GTSAM's InitializePose and LAGO [recalled: from memory, not read from either
// source; the contract is tests/ref_chordal.py and DESIGN.md 2.11]:
//   rotation stage     unknown r_i = (c_i, s_i) per free pose -> k_linearize_chordal<kChordalRotation, ..>, k_apply_rotation
//   translation stage  unknown t_i per free pose, l per free point, headings held
//                                                            -> k_linearize_chordal<kChordalTranslation, ..>, k_update_poses
// Both problems are linear, so one step from the current estimate solves them: the record holds J^T O J and -J^T O e at that
// estimate and the pass ends with x = x0 + dx.  All information comes from the edge's own 3x3 O: omega = O(2,2) for a heading
// term, O[0:2, 0:2] for a position term; the cross terms between the two are ignored by design.
//
// A 2-dimensional unknown owns a 3x3 block column like a point does in a typed Gauss-Newton pass: third row and column zero, the
// dummy's pivot the copy of H(0,0), its right-hand side zero, so its dx is exactly zero -- the translation stage ends with
// k_update_poses itself, which then leaves the heading (a point's dummy) as it is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "factor_model.h"
#include "gn_device.h"
#include "init_device.h"

namespace cgmr {

// The edge prologue, the per-workgroup cost at term[33 nE + blockIdx.x] and the record stream-out are k_linearize's
// (factor_model.h), the record layout is its own (gn_kernels.hip).
// A factor with a term in the stage gives the 2x2 Jacobians Ji, Jj of its 2-vector e, and the 2x2 information (o00, o01, o11):
//   rotation     EDGE_SE2 (i, j)    e = r_j - R(z_th) r_i                         Ji = -R(z_th)          Jj = I      omega I
//                EDGE_PRIOR_SE2     e = r_i - (cos z_th, sin z_th)                Ji = I                             omega I
//   translation  EDGE_SE2           e = R(z_th)^T (R_i^T (t_j - t_i) - z_t)       Ji = -R(z_th)^T R_i^T  Jj = -Ji    O[0:2, 0:2]
//                EDGE_SE2_XY        e = R_i^T (l - t_i) - z                       Ji = -R_i^T            Jj = R_i^T  O[0:2, 0:2]
//                EDGE_PRIOR_SE2     e = R(z_th)^T (t_i - z_t)                     Ji = R(z_th)^T                     O[0:2, 0:2]
//                EDGE_PRIOR_SE2_XY  e = t_i - z                                   Ji = I                             O[0:2, 0:2]
// Every other factor of a stage writes an exact zero record and adds nothing to the cost.
template <int STAGE, bool TYPED>
__global__ __launch_bounds__(256) void k_linearize_chordal(int nE, int nA, int n_active, const double* __restrict__ poses,
                                                           const int32_t* __restrict__ ef, const int32_t* __restrict__ et,
                                                           const double* __restrict__ meas, const double* __restrict__ info,
                                                           const double* __restrict__ meas_b, const double* __restrict__ info_b,
                                                           const uint8_t* __restrict__ edge_kind, double* __restrict__ term) {
  __shared__ double s_chi[4];
  extern __shared__ __attribute__((aligned(16))) double s_t[];        // [256][33]
  const int k0 = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = k0 < n_active;
  const int k = k0 < nE ? k0 : nE - 1;                   // idle lanes of the last workgroup shadow the last edge
  const EdgeEnds L = edge_prologue(k, nA, poses, ef, et, meas, meas_b);
  const double xi0 = L.xi0, xi1 = L.xi1, xi2 = L.xi2, xj0 = L.xj0, xj1 = L.xj1, xj2 = L.xj2;
  const double z0 = L.z0, z1 = L.z1, z2 = L.z2;
  const double* u = edge_split(k, nA, info, info_b, 6);
  int fk = CGMR_EDGE_SE2;
  if constexpr (TYPED) fk = k < nA ? (int)edge_kind[k] : CGMR_EDGE_SE2;
  const double c = cos(xi2), s = sin(xi2);
  const double cz = cos(z2), sz = sin(z2);
  double Ji[4] = {0, 0, 0, 0}, Jj[4] = {0, 0, 0, 0}, e[2] = {0, 0}, o00 = 0, o01 = 0, o11 = 0;
  if constexpr (STAGE == kChordalRotation) {
    if (fk == CGMR_EDGE_SE2) {
      e[0] = cos(xj2) - (cz * c - sz * s);
      e[1] = sin(xj2) - (sz * c + cz * s);
      Ji[0] = -cz; Ji[1] = sz; Ji[2] = -sz; Ji[3] = -cz;
      Jj[0] = 1.0; Jj[3] = 1.0;
      o00 = o11 = u[5];
    } else if (fk == CGMR_EDGE_PRIOR_SE2) {
      e[0] = c - cz;
      e[1] = s - sz;
      Ji[0] = 1.0; Ji[3] = 1.0;
      o00 = o11 = u[5];
    }
  } else {
    const double dx = xj0 - xi0, dy = xj1 - xi1;
    const double tx = (c * dx + s * dy) - z0, ty = (-s * dx + c * dy) - z1;
    if (fk == CGMR_EDGE_SE2) {
      e[0] = cz * tx + sz * ty;
      e[1] = -sz * tx + cz * ty;
      Jj[0] = cz * c - sz * s; Jj[1] = cz * s + sz * c;           // R(z_th)^T R_i^T
      Jj[2] = -sz * c - cz * s; Jj[3] = -sz * s + cz * c;
#pragma unroll
      for (int q = 0; q < 4; q++) Ji[q] = -Jj[q];
    } else if (fk == CGMR_EDGE_SE2_XY) {
      e[0] = tx;
      e[1] = ty;
      Jj[0] = c; Jj[1] = s; Jj[2] = -s; Jj[3] = c;
#pragma unroll
      for (int q = 0; q < 4; q++) Ji[q] = -Jj[q];
    } else if (fk == CGMR_EDGE_PRIOR_SE2) {
      const double px = xi0 - z0, py = xi1 - z1;
      e[0] = cz * px + sz * py;
      e[1] = -sz * px + cz * py;
      Ji[0] = cz; Ji[1] = sz; Ji[2] = -sz; Ji[3] = cz;
    } else if (fk == CGMR_EDGE_PRIOR_SE2_XY) {
      e[0] = xi0 - z0;
      e[1] = xi1 - z1;
      Ji[0] = 1.0; Ji[3] = 1.0;
    }
    if (fk != CGMR_EDGE_BEARING_SE2_XY) { o00 = u[0]; o01 = u[1]; o11 = u[3]; }
  }
  const double Oe0 = o00 * e[0] + o01 * e[1], Oe1 = o01 * e[0] + o11 * e[1];
  block_chi2_partial(live ? e[0] * Oe0 + e[1] * Oe1 : 0.0, s_chi, term, nE);
  double* mine = s_t + threadIdx.x * 33;
#pragma unroll
  for (int q = 0; q < 33; q++) mine[q] = 0.0;            // a switched-off edge, the third row / column, a factor without a term
  if (live && k0 < nE) {
    // J^T O, row r = unknown r: (J[0][r], J[1][r]) (o00 o01; o01 o11)
    double JiO[4], JjO[4];
#pragma unroll
    for (int r = 0; r < 2; r++) {
      JiO[2 * r] = Ji[r] * o00 + Ji[2 + r] * o01;
      JiO[2 * r + 1] = Ji[r] * o01 + Ji[2 + r] * o11;
      JjO[2 * r] = Jj[r] * o00 + Jj[2 + r] * o01;
      JjO[2 * r + 1] = Jj[r] * o01 + Jj[2 + r] * o11;
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
#pragma unroll
      for (int q = 0; q < 2; q++) {
        mine[3 * r + q] = JiO[2 * r] * Ji[q] + JiO[2 * r + 1] * Ji[2 + q];
        mine[9 + 3 * r + q] = JiO[2 * r] * Jj[q] + JiO[2 * r + 1] * Jj[2 + q];
        mine[18 + 3 * r + q] = JjO[2 * r] * Jj[q] + JjO[2 * r + 1] * Jj[2 + q];
      }
      mine[27 + r] = -(JiO[2 * r] * e[0] + JiO[2 * r + 1] * e[1]);
      mine[30 + r] = -(JjO[2 * r] * e[0] + JjO[2 * r + 1] * e[1]);
    }
    mine[8] = mine[0];                                    // the dummy unknowns' pivots: the copies of H(0,0)
    mine[26] = mine[18];
  }
  CGMR_RECORDS_STREAM_OUT(s_t, term, nE)
}

// The rotation stage's pass end, behind the backward solve: theta_v = atan2(sin theta_v + ds, cos theta_v + dc) with (dc, ds)
// the solved step of the vertex's column.  status[0], vperm, cmask and status[1] as in k_update_poses.  A solved (c, s) of
// length exactly zero, or not finite, has no direction: the pose keeps its heading and is counted in status[3].
__global__ __launch_bounds__(256) void k_apply_rotation(int nV, const int32_t* __restrict__ vperm, const uint8_t* __restrict__ cmask,
                                                        const double* __restrict__ xvec, double* __restrict__ poses,
                                                        int* __restrict__ status) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nV) return;
  const int failed = status[0];
  if (v == 0) status[1] = status[1] + 1;
  if (failed != 0) return;
  const int c = vperm[v];
  if (c < 0 || cmask[c]) return;                         // not in the system / fixed / left out of the stage
  const double th = poses[3 * v + 2];
  const double nc = cos(th) + xvec[3 * c], ns = sin(th) + xvec[3 * c + 1];
  const double n2 = nc * nc + ns * ns;
  if (n2 == 0.0 || !isfinite(n2)) {
    atomicAdd(status + kChordalDegenerateWord, 1);
    return;
  }
  poses[3 * v + 2] = atan2(ns, nc);
}

// The instances of k_linearize_chordal, written once: X(when, STAGE, TYPED), the first row whose `when` holds is the pass's
// (launch_linearize_chordal), and every row gets the LDS limit (init_chordal_kernels) -- as CGMR_LINEARIZE_TABLE, gn_kernels.hip.
#define CGMR_CHORDAL_TABLE(X)                      \
  X(rot && Ed.typed, kChordalRotation, true)       \
  X(rot, kChordalRotation, false)                  \
  X(Ed.typed, kChordalTranslation, true)           \
  X(true, kChordalTranslation, false)

// dynamic LDS above 64 KB: once per HIP device of the process, never inside a stream capture (gn_init_kernels)
static void init_chordal_kernels() {
  static std::once_flag once[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::call_once(once[dev & 63], [] {
#define CGMR_X(when, ...) reinterpret_cast<const void*>(k_linearize_chordal<__VA_ARGS__>),
    for (const void* f : {CGMR_CHORDAL_TABLE(CGMR_X)})
#undef CGMR_X
      (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kRecordLds);
  });
}

void launch_linearize_chordal(hipStream_t st, const GnDevice& D, const double* poses, const GnEdges& Ed) {
  if (D.nE == 0) return;
  init_chordal_kernels();
  const bool rot = Ed.chordal_stage == kChordalRotation;
#define CGMR_X(when, ...)                                                                                                        \
  if (when) {                                                                                                                    \
    hipLaunchKernelGGL((k_linearize_chordal<__VA_ARGS__>), dim3((D.nE + 255) / 256), dim3(256), kRecordLds, st, D.nE, Ed.nA,      \
                       Ed.n_active, poses, D.ef, D.et, Ed.meas_a, Ed.info_a, Ed.meas_b, Ed.info_b, Ed.ty.edge_kind, D.term);       \
    return;                                                                                                                      \
  }
  CGMR_CHORDAL_TABLE(CGMR_X)
#undef CGMR_X
}

void launch_apply_rotation(hipStream_t st, const GnDevice& D, double* poses) {
  hipLaunchKernelGGL(k_apply_rotation, dim3((D.nV + 255) / 256), dim3(256), 0, st, D.nV, D.vperm, D.cmask, D.xvec, poses, D.status);
}

}  // namespace cgmr
