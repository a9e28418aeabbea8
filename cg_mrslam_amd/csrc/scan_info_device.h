// Device side of the scan ranking and the greedy pruning (scan_info_kernels.hip / scan_info_host.cpp; include/cgmr.h:
// cgmr_scan_information, cgmr_scan_prune).
#ifndef CGMR_SCAN_INFO_DEVICE_H
#define CGMR_SCAN_INFO_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_device.h"

namespace cgmr {

constexpr int kSiBlock = 256;             // threads of every workgroup here
constexpr int kSiCellsPerBlock = 1024;    // window cells (or map cells) one workgroup reduces into one partial sum

// A scan's window: the rectangle x0 .. x1, y0 .. y1 of map cells (inclusive; x1 < x0: the scan touches no cell of the map)
// and where its (hits, misses) pairs start, window cell (x, y) at off + (x - x0) * (y1 - y0 + 1) + (y - y0).
struct SiWindow {
  int x0, y0, x1, y1;
  long long off;          // in int2 elements from the windows' base (of the chunk the scan belongs to)
  long long part_off;     // first of the scan's partial sums
  int n_part;             // ceil(cells / kSiCellsPerBlock)
  int pad;
};

// what a workgroup leaves of its share of a window
struct SiPartial {
  double dh;
  long long hit_sum, miss_sum;
  int cells, pad;
};

// the greedy loop's state, resident on the device between the rounds
struct SiState {
  double cum;             // sum of the deltas taken so far, in the order taken
  int n_removed;
  int stopped;
  int chosen;             // the scan taken in the last round that took one (-1: none yet)
  int fresh;              // 1: the last pick took `chosen` and its window is still to be subtracted
};

void launch_si_bbox(hipStream_t st, const OccParams& P, const float* ranges, const OccScan* scans, const float2* beam_cs, int4* bbox);
// the windows of the scans s0 .. s0 + n - 1 (P.n_scans, ranges, scans: all scans; win: all windows)
void launch_si_windows(hipStream_t st, const OccParams& P, int s0, int n, const float* ranges, const OccScan* scans,
                       const float2* beam_cs, const SiWindow* win, int2* cells);
// Delta H of the scans s0 .. s0 + n - 1 against the totals: partial sums per workgroup, then one fixed-order sum per scan.
// state / alive null: every scan, with the integer statistics; else only the alive scans whose window overlaps the one taken
// last (all of them in the first round), nothing once the loop has stopped.
void launch_si_delta(hipStream_t st, const OccParams& P, int s0, int n, int max_part, const SiWindow* win, const int2* cells,
                     const int32_t* hits, const int32_t* misses, SiPartial* part, const SiState* state, const uint8_t* alive,
                     int first_round, double* delta, int32_t* cells_out, long long* hit_sum, long long* miss_sum);
// sum of f over the rows * cols cells: per-workgroup partial sums, then one fixed-order sum
void launch_si_entropy(hipStream_t st, int ncells, const int32_t* hits, const int32_t* misses, double* part, double* out);
void launch_si_pick(hipStream_t st, int n_scans, int max_remove, double budget, const double* delta, uint8_t* alive,
                    const uint8_t* protect, SiState* state, int32_t* order, double* delta_taken);
void launch_si_subtract(hipStream_t st, const OccParams& P, int max_part, const SiWindow* win, const int2* cells, SiState* state,
                        int32_t* hits, int32_t* misses);

}  // namespace cgmr
#endif
