// HIP kernels of the all-pose marginals (cgmr_marginals_all): selected inversion of H = L L^T on the supernodal factor
// that the Gauss-Newton pass leaves in Lbuf (gn_kernels.hip), i.e. the Takahashi recurrence that g2o evaluates entry by
// entry for computeMarginals [g2o-recalled], here one dense front at a time.
//
// For a front with w = 3 nc own columns, r = 3 ns border rows, L11 / L21 its factor, Z = L11^-1 (k_invert_fronts) and
// Sigma22 the inverse restricted to its border rows (a subset of its parent's rows, found through rel):
//       Sigma21 = -(Sigma22 L21) Z                  (r x r . r x w, then r x w . w x w)
//       Sigma11 = Z^T (Z - L21^T Sigma21)            (symmetric, w x w)
// Every front keeps Sigma on its whole row list as a dense (w + r)^2 block (SelinvPlan::soff), indexed the way rel indexes a
// parent's rows: own columns first, then the border, both triangles stored.  The tree is walked top-down, two launches
// per level of the full level list (the top block's fronts are ordinary fronts here):
//   k_selinv_border   one workgroup per row tile of 64 border rows of a front: gathers its rows of Sigma22 from the
//                     parent's block (and stores them: the front's children gather from it), Sigma22 L21 and the product
//                     with Z on v_mfma_f64_16x16x4_f64, Sigma21 and its transpose into the front's block
//   k_selinv_own      one workgroup per front: L21^T Sigma21 split over the four wavefronts, summed in a fixed order,
//                     Z^T (Z - ...) , Sigma11 written symmetric (the lower triangle mirrored)
// and one extraction launch (k_selinv_extract).  No workgroup waits on another (ordering by launch boundaries only), no
// atomics: the result is bit-identical from run to run.
//
// f64 MFMA lane maps (cdna_hip 16x16x4 f64): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// C/D element (row = (lane >> 4) + 4 reg, col = lane & 15).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gn_device.h"
#include "gn_symbolic.h"

namespace cgmr {

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {
constexpr int W = kFrontW;                         // padded width of a front's factor panel (48)
constexpr int kL21 = 2 * W * W + W;                // L21 (r rows of W) behind the factor header, Z = L11^-1 (W x W) behind L21
constexpr int CT = W / 16;                         // 16-column tiles of a front's own columns
constexpr int TR = kSelinvTileRows;                // border rows per k_selinv_border workgroup (16 per wavefront)
constexpr int KC = 64;                             // border columns of Sigma22 staged in LDS per round
static_assert(TR == 64 && W % 16 == 0, "selinv tiling");
static_assert(W == 48, "Z = L11^-1 (k_invert_fronts) is made for 48-column panels only");

__device__ __forceinline__ int parent_row(const int32_t* __restrict__ relf, int i) { return 3 * relf[i / 3] + i % 3; }
}  // namespace

// Launch A of a level: workgroup = (front f, border rows [t0, t0 + TR)).  256 threads, wavefront v owns rows t0 + 16 v ..
__global__ __launch_bounds__(256) void k_selinv_border(const int32_t* __restrict__ tiles, int tile_begin,
                                                       const FrontDesc* __restrict__ fronts, const int32_t* __restrict__ rel,
                                                       const double* __restrict__ Lbuf, const int64_t* __restrict__ soff,
                                                       double* __restrict__ Sig) {
  __shared__ double sA[TR][KC + 1];                  // rows of Sigma22 (a KC-column slice); later T = Sigma22 L21 (W columns)
  __shared__ double sB[KC][W];                       // rows of L21, own columns beyond w as zeros
  __shared__ double sZ[W][W];                        // Z, zeros outside w x w
  __shared__ int s_ri[TR], s_ci[KC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ii = lane & 15, kk = lane >> 4;
  const int f = tiles[2 * (tile_begin + blockIdx.x)], t0 = tiles[2 * (tile_begin + blockIdx.x) + 1];
  const FrontDesc F = fronts[f];
  const FrontDesc P = fronts[F.parent];
  const int w = 3 * F.nc, r = 3 * F.ns, n = w + r, np = 3 * (P.nc + P.ns);
  const int32_t* relf = rel + F.rel_off;
  const double* L21 = Lbuf + F.L_off + kL21;
  const double* Z = L21 + (size_t)r * W;
  const double* Sp = Sig + soff[F.parent];
  double* Sf = Sig + soff[f];
  for (int e = tid; e < W * W; e += 256) {
    const int k = e / W, j = e - k * W;
    sZ[k][j] = (k < w && j < w) ? Z[e] : 0.0;
  }
  if (tid < TR) s_ri[tid] = t0 + tid < r ? parent_row(relf, t0 + tid) : -1;
  double4_t acc[CT];
#pragma unroll
  for (int c = 0; c < CT; c++) acc[c] = double4_t{0, 0, 0, 0};
  for (int kc = 0; kc < r; kc += KC) {
    __syncthreads();                                 // (the previous round's readers are done)
    if (tid < KC) s_ci[tid] = kc + tid < r ? parent_row(relf, kc + tid) : -1;
    for (int e = tid; e < KC * W; e += 256) {
      const int k = e / W, j = e - k * W;
      sB[k][j] = (kc + k < r && j < w) ? L21[(size_t)(kc + k) * W + j] : 0.0;
    }
    __syncthreads();
    // Sigma22[t0 + i][kc + k] = Sigma_parent[ri][ci]: staged, and stored into this front's block
    for (int e = tid; e < TR * KC; e += 256) {
      const int i = e / KC, k = e - i * KC;
      const int ri = s_ri[i], ci = s_ci[k];
      double v = 0.0;
      if (ri >= 0 && ci >= 0) {
        v = Sp[(size_t)ri * np + ci];
        Sf[(size_t)(w + t0 + i) * n + w + kc + k] = v;
      }
      sA[i][k] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int k4 = 0; k4 < KC; k4 += 4) {
      const double a = sA[16 * wave + ii][k4 + kk];
#pragma unroll
      for (int c = 0; c < CT; c++) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[k4 + kk][16 * c + ii], acc[c], 0, 0, 0);
    }
  }
  __syncthreads();
  // T = Sigma22 L21 (this wavefront's 16 rows) into LDS as the next product's A operand
#pragma unroll
  for (int c = 0; c < CT; c++)
#pragma unroll
    for (int g = 0; g < 4; g++) sA[16 * wave + kk + 4 * g][16 * c + ii] = acc[c][g];
  __syncthreads();
  double4_t out[CT];
#pragma unroll
  for (int c = 0; c < CT; c++) out[c] = double4_t{0, 0, 0, 0};
#pragma unroll 4
  for (int k4 = 0; k4 < W; k4 += 4) {
    const double a = sA[16 * wave + ii][k4 + kk];
#pragma unroll
    for (int c = 0; c < CT; c++) out[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sZ[k4 + kk][16 * c + ii], out[c], 0, 0, 0);
  }
  // Sigma21 = -T Z and Sigma12 = its transpose
#pragma unroll
  for (int c = 0; c < CT; c++)
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int i = t0 + 16 * wave + kk + 4 * g, j = 16 * c + ii;
      if (i < r && j < w) {
        const double v = -out[c][g];
        Sf[(size_t)(w + i) * n + j] = v;
        Sf[(size_t)j * n + w + i] = v;
      }
    }
}

// Launch B of a level: one workgroup per front of the level (roots included: r = 0, Sigma11 = Z^T Z).
__global__ __launch_bounds__(256) void k_selinv_own(const int32_t* __restrict__ level_fronts, int level_begin,
                                                    const FrontDesc* __restrict__ fronts, const double* __restrict__ Lbuf,
                                                    const int64_t* __restrict__ soff, double* __restrict__ Sig) {
  __shared__ double sZ[W][W + 1];
  __shared__ double sN[W][W + 1];                    // Z - L21^T Sigma21, then Sigma11
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ii = lane & 15, kk = lane >> 4;
  const int f = level_fronts[level_begin + blockIdx.x];
  const FrontDesc F = fronts[f];
  const int w = 3 * F.nc, r = 3 * F.ns, n = w + r;
  const double* L21 = Lbuf + F.L_off + kL21;
  const double* Z = L21 + (size_t)r * W;
  double* Sf = Sig + soff[f];
  for (int e = tid; e < W * W; e += 256) {
    const int k = e / W, j = e - k * W;
    const double z = (k < w && j < w) ? Z[e] : 0.0;
    sZ[k][j] = z;
    sN[k][j] = z;
  }
  // M = L21^T Sigma21: wavefront v sums the border rows 4 (v + 4 s) .. + 3, all 9 tiles of M
  double4_t m[CT][CT];
#pragma unroll
  for (int a = 0; a < CT; a++)
#pragma unroll
    for (int b = 0; b < CT; b++) m[a][b] = double4_t{0, 0, 0, 0};
  for (int k4 = 4 * wave; k4 < r; k4 += 16) {
    const int k = k4 + kk;
    double av[CT], bv[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) {
      const int j = 16 * c + ii;
      av[c] = (k < r && j < w) ? L21[(size_t)k * W + j] : 0.0;         // A[i][k] = L21[k][i]
      bv[c] = (k < r && j < w) ? Sf[(size_t)(w + k) * n + j] : 0.0;    // B[k][j] = Sigma21[k][j]
    }
#pragma unroll
    for (int a = 0; a < CT; a++)
#pragma unroll
      for (int b = 0; b < CT; b++) m[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], m[a][b], 0, 0, 0);
  }
  // N = Z - M, the four partial sums subtracted in wavefront order
  for (int v = 0; v < 4; v++) {
    __syncthreads();
    if (wave == v)
#pragma unroll
      for (int a = 0; a < CT; a++)
#pragma unroll
        for (int b = 0; b < CT; b++)
#pragma unroll
          for (int g = 0; g < 4; g++) sN[16 * a + kk + 4 * g][16 * b + ii] -= m[a][b][g];
  }
  __syncthreads();
  // Sigma11 = Z^T N, the lower tiles (a >= b) only: wavefront v takes tiles v, v + 4 of (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
  constexpr int NT = CT * (CT + 1) / 2;
  double4_t s[2];
  int ta[2], tb[2];
  for (int q = 0; q < 2; q++) {
    const int t = wave + 4 * q;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= t) a++;
    ta[q] = a; tb[q] = t - a * (a + 1) / 2;
    s[q] = double4_t{0, 0, 0, 0};
    if (t >= NT) continue;
#pragma unroll 4
    for (int k4 = 0; k4 < W; k4 += 4)
      s[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(sZ[k4 + kk][16 * ta[q] + ii], sN[k4 + kk][16 * tb[q] + ii], s[q], 0, 0, 0);
  }
  __syncthreads();                                   // (every wavefront is done reading N)
  for (int q = 0; q < 2; q++) {
    if (wave + 4 * q >= NT) continue;
#pragma unroll
    for (int g = 0; g < 4; g++) sN[16 * ta[q] + kk + 4 * g][16 * tb[q] + ii] = s[q][g];
  }
  __syncthreads();
  for (int e = tid; e < w * w; e += 256) {
    const int i = e / w, j = e - i * w;
    Sf[(size_t)i * n + j] = i >= j ? sN[i][j] : sN[j][i];
  }
}

// cov_out[v] (v < nV) and cross_out[e] (nV <= thread < nV + nE) from the fronts' blocks.  vcol[v]: permuted column of
// vertex v, -1 when it is fixed or inactive (zeros).  An edge's block sits in the front that owns its lower-numbered
// column, in its own columns or in its border rows (binary search of the ascending rows).
__global__ void k_selinv_extract(int nV, int nE, const int32_t* __restrict__ vcol, const int32_t* __restrict__ ef,
                                 const int32_t* __restrict__ et, const int32_t* __restrict__ col_front,
                                 const FrontDesc* __restrict__ fronts, const int32_t* __restrict__ rows,
                                 const int64_t* __restrict__ soff, const double* __restrict__ Sig, double* __restrict__ cov,
                                 double* __restrict__ cross) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nV + (cross ? nE : 0)) return;
  const bool is_v = t < nV;
  const int cu = is_v ? vcol[t] : vcol[ef[t - nV]];
  const int cv = is_v ? cu : vcol[et[t - nV]];
  double* o = is_v ? cov + 9 * (size_t)t : cross + 9 * (size_t)(t - nV);
  if (cu < 0 || cv < 0) {
#pragma unroll
    for (int q = 0; q < 9; q++) o[q] = 0.0;
    return;
  }
  const int f = col_front[min(cu, cv)];
  const FrontDesc F = fronts[f];
  const int n = 3 * (F.nc + F.ns);
  auto pos = [&](int c) -> int {
    if (c < F.c0 + F.nc) return 3 * (c - F.c0);
    int lo = 0, hi = F.ns;                           // first border row >= c
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (rows[F.rows_off + mid] < c) lo = mid + 1; else hi = mid; }
    return lo < F.ns && rows[F.rows_off + lo] == c ? 3 * (F.nc + lo) : -1;
  };
  const int pu = pos(cu), pv = pos(cv);
  if (pu < 0 || pv < 0) {                            // (not in the pattern of L: cannot happen for an edge of the graph)
#pragma unroll
    for (int q = 0; q < 9; q++) o[q] = __builtin_nan("");
    return;
  }
  const double* S = Sig + soff[f];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) o[3 * a + b] = S[(size_t)(pu + a) * n + pv + b];
}

// ----------------------------------------------------------------------------------- launcher
void launch_selinv(hipStream_t st, const GnDevice& D, const SelinvPlan& P, int nV, int nE, const int32_t* vcol,
                   const int32_t* col_front, double* cov, double* cross) {
  for (int l = D.nlevels_full - 1; l >= 0; l--) {    // root level first
    const int nt = P.h_tile_ptr[l + 1] - P.h_tile_ptr[l];
    if (nt > 0)
      hipLaunchKernelGGL(k_selinv_border, dim3(nt), dim3(256), 0, st, P.tiles, P.h_tile_ptr[l], D.fronts, D.rel, D.Lbuf, P.soff, P.Sig);
    const int nfr = D.h_flevel_ptr[l + 1] - D.h_flevel_ptr[l];
    if (nfr > 0)
      hipLaunchKernelGGL(k_selinv_own, dim3(nfr), dim3(256), 0, st, D.level_fronts, D.h_flevel_ptr[l], D.fronts, D.Lbuf, P.soff, P.Sig);
  }
  const int nt = nV + (cross ? nE : 0);
  if (nt > 0)
    hipLaunchKernelGGL(k_selinv_extract, dim3((nt + 255) / 256), dim3(256), 0, st, nV, nE, vcol, D.ef, D.et, col_front, D.fronts,
                       D.rows, P.soff, P.Sig, cov, cross);
}

}  // namespace cgmr
