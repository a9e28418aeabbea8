// HIP kernels (gfx950) that rank laser scans by what they tell the occupancy map, and the greedy pruning built on the ranking
// (include/cgmr.h: cgmr_scan_information, cgmr_scan_prune).
//
// Counting.  Every scan gets a window of its own in HBM: the bounding box of the map cells its walk visits, an int2 (hits,
// misses) per cell.  k_si_bbox and k_si_windows run the walk of occupancy_walk.h -- the body of k_occ_integrate -- with other
// sinks: the first keeps the extremes of the visited cells in registers, the second counts with 32-bit integer atomics as
// the map does.  Integer sums commute: windows and totals are exact, and the windows of all scans add up to the map.
//
// Delta H.  One workgroup per kSiCellsPerBlock window cells, thread t takes the cells t, t + 256, t + 512, t + 768 of its
// share in that order, the 256 sums meet in a butterfly of shuffles and the four waves' in index order; k_si_delta_sum adds
// a scan's partial sums lane by lane in index order and closes with the same butterfly.  The order depends on the cell's
// place in the window only: two calls give the same bytes, two identical scans the same Delta H.  No floating-point atomics.
//
// The greedy loop is stream order: Delta H pass, k_si_pick (one workgroup: arg-min under (Delta H, s), the stop rules, the
// records), k_si_subtract (takes the chosen scan from device memory).  A round after a stop finds `stopped` set and does
// nothing.  A round recomputes only the alive scans whose window overlaps the window taken last: Delta H of a scan reads the
// totals under its own window and nothing else, so every other value is already the one a recomputation would give.
//
// f is evaluated in double; compiled with the default -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "occupancy_walk.h"
#include "scan_info_device.h"

namespace cgmr {

namespace {

struct SiBoxSink {
  int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
  __device__ __forceinline__ void miss(int x, int y) { x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y); }
  __device__ __forceinline__ void hit(int x, int y, int) { miss(x, y); }
};

// a cell outside the window cannot be visited (the window is the bounding box of exactly these visits): the test keeps a
// mistake in that reasoning a wrong count and not a wild store
struct SiWindowSink {
  const SiWindow W;
  int2* __restrict__ cells;
  __device__ __forceinline__ int2* at(int x, int y) const {
    if (x < W.x0 || x > W.x1 || y < W.y0 || y > W.y1) return nullptr;
    return cells + W.off + (long long)(x - W.x0) * (W.y1 - W.y0 + 1) + (y - W.y0);
  }
  __device__ __forceinline__ void miss(int x, int y) const { int2* c = at(x, y); if (c) atomicAdd(&c->y, 1); }
  __device__ __forceinline__ void hit(int x, int y, int gain) const { int2* c = at(x, y); if (c) atomicAdd(&c->x, gain); }
};

// Bernoulli entropy, in nats, of the posterior mean under a uniform prior
__device__ __forceinline__ double si_f(int h, int m) {
  const double p = (double)(h + 1) / (double)(h + m + 2);
  const double q = 1.0 - p;
  return -p * log(p) - q * log(q);
}

__device__ __forceinline__ long long si_cells(const SiWindow& W) {
  return W.x1 < W.x0 ? 0 : (long long)(W.x1 - W.x0 + 1) * (W.y1 - W.y0 + 1);
}

// does scan s sit this Delta H pass out?  (both kernels of the pass ask the same question)
__device__ __forceinline__ bool si_idle(const SiState* state, const uint8_t* alive, const SiWindow* win, int s, int first_round) {
  if (!state) return false;
  if (state->stopped || !alive[s]) return true;
  if (first_round) return false;
  const SiWindow W = win[s], C = win[state->chosen];
  return W.x1 < C.x0 || C.x1 < W.x0 || W.y1 < C.y0 || C.y1 < W.y0;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
  return v;
}

}  // namespace

__global__ __launch_bounds__(kSiBlock) void k_si_bbox(OccParams P, const float* __restrict__ ranges,
                                                      const OccScan* __restrict__ scans, const float2* __restrict__ beam_cs,
                                                      int4* __restrict__ bbox) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)P.n_scans * P.n_beams) return;
  const int s = (int)(t / P.n_beams), i = (int)(t - (long long)s * P.n_beams);
  const OccScan S = scans[s];
  SiBoxSink sink;
  occ_walk_beam(P, S, i, ranges + (size_t)s * P.n_beams, beam_cs, sink);
  if (sink.x1 < sink.x0) return;
  int* b = reinterpret_cast<int*>(bbox + s);
  atomicMin(b + 0, sink.x0); atomicMin(b + 1, sink.y0); atomicMax(b + 2, sink.x1); atomicMax(b + 3, sink.y1);
}

__global__ __launch_bounds__(kSiBlock) void k_si_windows(OccParams P, int s0, int n, const float* __restrict__ ranges,
                                                         const OccScan* __restrict__ scans, const float2* __restrict__ beam_cs,
                                                         const SiWindow* __restrict__ win, int2* __restrict__ cells) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * P.n_beams) return;
  const int s = s0 + (int)(t / P.n_beams), i = (int)(t % P.n_beams);
  const OccScan S = scans[s];
  SiWindowSink sink{win[s], cells};
  occ_walk_beam(P, S, i, ranges + (size_t)s * P.n_beams, beam_cs, sink);
}

template <bool STATS>
__global__ __launch_bounds__(kSiBlock) void k_si_delta(OccParams P, int s0, const SiWindow* __restrict__ win,
                                                       const int2* __restrict__ cells, const int32_t* __restrict__ hits,
                                                       const int32_t* __restrict__ misses, SiPartial* __restrict__ part,
                                                       const SiState* __restrict__ state, const uint8_t* __restrict__ alive,
                                                       int first_round) {
  __shared__ double sh_d[kSiBlock / 64];
  __shared__ long long sh_h[kSiBlock / 64], sh_m[kSiBlock / 64];
  __shared__ int sh_c[kSiBlock / 64];
  const int s = s0 + blockIdx.x;
  if (si_idle(state, alive, win, s, first_round)) return;
  const SiWindow W = win[s];
  const long long ncell = si_cells(W);
  const int wy = W.y1 - W.y0 + 1;
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int p = blockIdx.y; p < W.n_part; p += gridDim.y) {
    double dh = 0.0;
    long long hs = 0, ms = 0;
    int nc = 0;
    for (int j = 0; j < kSiCellsPerBlock / kSiBlock; j++) {
      const long long c = (long long)p * kSiCellsPerBlock + j * kSiBlock + tid;
      if (c >= ncell) break;
      const int2 own = cells[W.off + c];
      if (own.x == 0 && own.y == 0) continue;
      const size_t k = (size_t)(W.x0 + (int)(c / wy)) * P.cols + (W.y0 + (int)(c % wy));
      const int H = hits[k], M = misses[k];
      dh += si_f(H - own.x, M - own.y) - si_f(H, M);
      if (STATS) { hs += own.x; ms += own.y; nc++; }
    }
    dh = wave_sum(dh);
    if (STATS) { hs = wave_sum(hs); ms = wave_sum(ms); nc = wave_sum(nc); }
    if ((tid & 63) == 0) { sh_d[wave] = dh; if (STATS) { sh_h[wave] = hs; sh_m[wave] = ms; sh_c[wave] = nc; } }
    __syncthreads();
    if (tid == 0) {
      SiPartial o;
      o.dh = ((sh_d[0] + sh_d[1]) + sh_d[2]) + sh_d[3];
      o.hit_sum = o.miss_sum = 0; o.cells = 0; o.pad = 0;
      if (STATS) {
        o.hit_sum = sh_h[0] + sh_h[1] + sh_h[2] + sh_h[3];
        o.miss_sum = sh_m[0] + sh_m[1] + sh_m[2] + sh_m[3];
        o.cells = sh_c[0] + sh_c[1] + sh_c[2] + sh_c[3];
      }
      part[W.part_off + p] = o;
    }
    __syncthreads();
  }
}

// one wave per scan: lane t adds the partial sums t, t + 64, ... in that order
template <bool STATS>
__global__ __launch_bounds__(64) void k_si_delta_sum(int s0, const SiWindow* __restrict__ win, const SiPartial* __restrict__ part,
                                                     const SiState* __restrict__ state, const uint8_t* __restrict__ alive,
                                                     int first_round, double* __restrict__ delta, int32_t* __restrict__ cells_out,
                                                     long long* __restrict__ hit_sum, long long* __restrict__ miss_sum) {
  const int s = s0 + blockIdx.x;
  if (si_idle(state, alive, win, s, first_round)) return;
  const SiWindow W = win[s];
  double dh = 0.0;
  long long hs = 0, ms = 0;
  int nc = 0;
  for (int p = threadIdx.x; p < W.n_part; p += 64) {
    const SiPartial q = part[W.part_off + p];
    dh += q.dh;
    if (STATS) { hs += q.hit_sum; ms += q.miss_sum; nc += q.cells; }
  }
  dh = wave_sum(dh);
  if (STATS) { hs = wave_sum(hs); ms = wave_sum(ms); nc = wave_sum(nc); }
  if (threadIdx.x == 0) {
    delta[s] = dh;
    if (STATS) { cells_out[s] = nc; hit_sum[s] = hs; miss_sum[s] = ms; }
  }
}

__global__ __launch_bounds__(kSiBlock) void k_si_entropy(int ncells, const int32_t* __restrict__ hits,
                                                         const int32_t* __restrict__ misses, double* __restrict__ part) {
  __shared__ double sh[kSiBlock / 64];
  const int tid = threadIdx.x;
  double v = 0.0;
  for (int j = 0; j < kSiCellsPerBlock / kSiBlock; j++) {
    const long long c = (long long)blockIdx.x * kSiCellsPerBlock + j * kSiBlock + tid;
    if (c < ncells) v += si_f(hits[c], misses[c]);
  }
  v = wave_sum(v);
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(kSiBlock) void k_si_entropy_sum(int n_part, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double sh[kSiBlock / 64];
  const int tid = threadIdx.x;
  double v = 0.0;
  for (int p = tid; p < n_part; p += kSiBlock) v += part[p];
  v = wave_sum(v);
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) *out = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// One workgroup.  The minimum of Delta H over the alive, unprotected scans under the total order (Delta H, s): every thread
// over its share, a butterfly of shuffles per wave, the four waves in LDS.  Thread 0 applies the stop rules and keeps the records.
__global__ __launch_bounds__(kSiBlock) void k_si_pick(int n_scans, int max_remove, double budget, const double* __restrict__ delta,
                                                      uint8_t* __restrict__ alive, const uint8_t* __restrict__ protect,
                                                      SiState* __restrict__ state, int32_t* __restrict__ order,
                                                      double* __restrict__ delta_taken) {
  __shared__ double sh_d[kSiBlock / 64];
  __shared__ int sh_s[kSiBlock / 64];
  const int tid = threadIdx.x;
  const bool stopped = state->stopped != 0;
  double bd = 0.0;
  int bs = INT_MAX;                                  // INT_MAX: no candidate yet
  if (!stopped)
    for (int s = tid; s < n_scans; s += kSiBlock) {
      if (!alive[s] || (protect && protect[s])) continue;
      const double d = delta[s];
      if (bs == INT_MAX || d < bd || (d == bd && s < bs)) { bd = d; bs = s; }
    }
  for (int k = 32; k >= 1; k >>= 1) {
    const double od = __shfl_xor(bd, k, 64);
    const int os = __shfl_xor(bs, k, 64);
    if (os != INT_MAX && (bs == INT_MAX || od < bd || (od == bd && os < bs))) { bd = od; bs = os; }
  }
  if ((tid & 63) == 0) { sh_d[tid >> 6] = bd; sh_s[tid >> 6] = bs; }
  __syncthreads();
  if (tid != 0) return;
  state->fresh = 0;
  if (stopped) return;
  for (int w = 1; w < kSiBlock / 64; w++)
    if (sh_s[w] != INT_MAX && (bs == INT_MAX || sh_d[w] < bd || (sh_d[w] == bd && sh_s[w] < bs))) { bd = sh_d[w]; bs = sh_s[w]; }
  const int k = state->n_removed;
  if (k >= max_remove || bs == INT_MAX || (budget >= 0.0 && state->cum + bd > budget)) { state->stopped = 1; return; }
  order[k] = bs;
  delta_taken[k] = bd;
  state->cum += bd;
  state->n_removed = k + 1;
  state->chosen = bs;
  state->fresh = 1;
  alive[bs] = 0;
}

// the chosen scan's counts leave the totals; every map cell under the window belongs to one thread
__global__ __launch_bounds__(kSiBlock) void k_si_subtract(OccParams P, const SiWindow* __restrict__ win, const int2* __restrict__ cells,
                                                          const SiState* __restrict__ state, int32_t* __restrict__ hits,
                                                          int32_t* __restrict__ misses) {
  if (!state->fresh) return;
  const SiWindow W = win[state->chosen];
  const long long ncell = si_cells(W);
  const int wy = W.y1 - W.y0 + 1;
  for (int p = blockIdx.x; p < W.n_part; p += gridDim.x)
    for (int j = 0; j < kSiCellsPerBlock / kSiBlock; j++) {
      const long long c = (long long)p * kSiCellsPerBlock + j * kSiBlock + threadIdx.x;
      if (c >= ncell) break;
      const int2 own = cells[W.off + c];
      if (own.x == 0 && own.y == 0) continue;
      const size_t k = (size_t)(W.x0 + (int)(c / wy)) * P.cols + (W.y0 + (int)(c % wy));
      hits[k] -= own.x;
      misses[k] -= own.y;
    }
}

// ------------------------------------------------------------------------------------------------------------------ launches
void launch_si_bbox(hipStream_t st, const OccParams& P, const float* ranges, const OccScan* scans, const float2* beam_cs, int4* bbox) {
  const long long total = (long long)P.n_scans * P.n_beams;
  if (total <= 0) return;
  hipLaunchKernelGGL(k_si_bbox, dim3((unsigned)((total + kSiBlock - 1) / kSiBlock)), dim3(kSiBlock), 0, st, P, ranges, scans, beam_cs, bbox);
}

void launch_si_windows(hipStream_t st, const OccParams& P, int s0, int n, const float* ranges, const OccScan* scans,
                       const float2* beam_cs, const SiWindow* win, int2* cells) {
  const long long total = (long long)n * P.n_beams;
  if (total <= 0) return;
  hipLaunchKernelGGL(k_si_windows, dim3((unsigned)((total + kSiBlock - 1) / kSiBlock)), dim3(kSiBlock), 0, st, P, s0, n, ranges, scans,
                     beam_cs, win, cells);
}

void launch_si_delta(hipStream_t st, const OccParams& P, int s0, int n, int max_part, const SiWindow* win, const int2* cells,
                     const int32_t* hits, const int32_t* misses, SiPartial* part, const SiState* state, const uint8_t* alive,
                     int first_round, double* delta, int32_t* cells_out, long long* hit_sum, long long* miss_sum) {
  if (n <= 0) return;
  const dim3 grid((unsigned)n, (unsigned)(max_part < 1 ? 1 : max_part > 65535 ? 65535 : max_part));
  if (!state) {
    hipLaunchKernelGGL(k_si_delta<true>, grid, dim3(kSiBlock), 0, st, P, s0, win, cells, hits, misses, part, state, alive, first_round);
    hipLaunchKernelGGL(k_si_delta_sum<true>, dim3((unsigned)n), dim3(64), 0, st, s0, win, part, state, alive, first_round, delta,
                       cells_out, hit_sum, miss_sum);
  } else {
    hipLaunchKernelGGL(k_si_delta<false>, grid, dim3(kSiBlock), 0, st, P, s0, win, cells, hits, misses, part, state, alive, first_round);
    hipLaunchKernelGGL(k_si_delta_sum<false>, dim3((unsigned)n), dim3(64), 0, st, s0, win, part, state, alive, first_round, delta,
                       cells_out, hit_sum, miss_sum);
  }
}

void launch_si_entropy(hipStream_t st, int ncells, const int32_t* hits, const int32_t* misses, double* part, double* out) {
  const int n_part = (ncells + kSiCellsPerBlock - 1) / kSiCellsPerBlock;
  hipLaunchKernelGGL(k_si_entropy, dim3((unsigned)n_part), dim3(kSiBlock), 0, st, ncells, hits, misses, part);
  hipLaunchKernelGGL(k_si_entropy_sum, dim3(1), dim3(kSiBlock), 0, st, n_part, part, out);
}

void launch_si_pick(hipStream_t st, int n_scans, int max_remove, double budget, const double* delta, uint8_t* alive,
                    const uint8_t* protect, SiState* state, int32_t* order, double* delta_taken) {
  hipLaunchKernelGGL(k_si_pick, dim3(1), dim3(kSiBlock), 0, st, n_scans, max_remove, budget, delta, alive, protect, state, order,
                     delta_taken);
}

void launch_si_subtract(hipStream_t st, const OccParams& P, int max_part, const SiWindow* win, const int2* cells, SiState* state,
                        int32_t* hits, int32_t* misses) {
  const unsigned grid = (unsigned)(max_part < 1 ? 1 : max_part > 65535 ? 65535 : max_part);
  hipLaunchKernelGGL(k_si_subtract, dim3(grid), dim3(kSiBlock), 0, st, P, win, cells, state, hits, misses);
}

}  // namespace cgmr
