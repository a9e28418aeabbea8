// HIP kernels (gfx950) for the occupancy map the reference publishes from the optimised graph
// (SURVEY.md 8f row 4):
//   FrequencyMap::integrateScan + fillRobotPose   src/ros_map_publisher/frequency_map.cpp:27-103
//   GridLineTraversal::gridLineCore               src/ros_map_publisher/grid_line_traversal.cpp:31-140
//   frequency -> image                            src/ros_map_publisher/graph2occupancy.cpp:128-147
//
// Design: one thread per (scan, beam).  The thread resolves the beam's range rules, maps the end point with the
// reference's float arithmetic (float subtract / divide, round-half-even), walks the reference's Bresenham
// variant (occupancy_walk.h: the walk is shared with the per-scan windows of scan_info_kernels.hip) and counts with 32-bit integer atomics on HBM -- integer sums commute, so the result is bit-identical
// to the sequential reference whatever the order.  Consecutive lanes are consecutive beams of one scan: near the
// sensor they step through the same cells, which the L2 atomic units absorb; far out the lines fan apart.
// Must be compiled with -ffp-contract=off (Makefile default): no FMA may replace a float op the reference rounds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_device.h"
#include "occupancy_walk.h"

namespace cgmr {

namespace {

// the map itself: 32-bit integer atomics on the HBM counters
struct OccMapSink {
  const OccParams& P;
  int32_t* __restrict__ hits;
  int32_t* __restrict__ misses;
  __device__ __forceinline__ void miss(int x, int y) const { atomicAdd(&misses[(size_t)x * P.cols + y], 1); }
  __device__ __forceinline__ void hit(int x, int y, int gain) const { atomicAdd(&hits[(size_t)x * P.cols + y], gain); }
};

}  // namespace

__global__ __launch_bounds__(256) void k_occ_integrate(OccParams P, const float* __restrict__ ranges,
                                                       const OccScan* __restrict__ scans,
                                                       const float2* __restrict__ beam_cs,
                                                       int32_t* __restrict__ hits, int32_t* __restrict__ misses) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)P.n_scans * P.n_beams) return;
  const int s = (int)(t / P.n_beams), i = (int)(t - (long long)s * P.n_beams);
  const OccScan S = scans[s];
  OccMapSink sink{P, hits, misses};
  occ_walk_beam(P, S, i, ranges + (size_t)s * P.n_beams, beam_cs, sink);
}

__global__ __launch_bounds__(256) void k_occ_image(int ncells, const int32_t* __restrict__ hits,
                                                   const int32_t* __restrict__ misses, float threshold,
                                                   float free_threshold, uint8_t* __restrict__ image) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ncells) return;
  const int h = hits[k], m = misses[k];
  uint8_t v = 255;                                 // unknown (graph2occupancy.h:79-81)
  if (!(m == 0 && h == 0)) {
    const float fraction = (float)h / (float)(h + m);
    if (free_threshold != 0.0f && fraction < free_threshold) v = 0;
    else if (threshold != 0.0f && fraction > threshold) v = 100;
  }
  image[k] = v;
}

void launch_occ_integrate(hipStream_t st, const OccParams& P, const float* ranges, const OccScan* scans,
                          const float2* beam_cs, int32_t* hits, int32_t* misses) {
  const long long total = (long long)P.n_scans * P.n_beams;
  if (total <= 0) return;
  hipLaunchKernelGGL(k_occ_integrate, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P, ranges, scans, beam_cs,
                     hits, misses);
}

void launch_occ_image(hipStream_t st, int ncells, const int32_t* hits, const int32_t* misses, float threshold,
                      float free_threshold, uint8_t* image) {
  if (ncells <= 0) return;
  hipLaunchKernelGGL(k_occ_image, dim3((ncells + 255) / 256), dim3(256), 0, st, ncells, hits, misses, threshold,
                     free_threshold, image);
}

}  // namespace cgmr
