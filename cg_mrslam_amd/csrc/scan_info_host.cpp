// cgmr_scan_information / cgmr_scan_prune (include/cgmr.h): the host side of the scan ranking.  Compiled with hipcc; no kernels.
//
// Both calls share one driver.  Everything that can be refused from the arguments is refused first.  Then the inputs go to the
// staging arena and one pre-pass (k_si_bbox, the map's own walk) gives every scan's bounding box among the map's cells: the one
// read-back the window layout needs.  The windows, the totals and every result live in the matcher arena; the windows are
// bounded by scratch_bytes_limit (0: kSiDefaultScratch).  The ranking works through the scans in chunks of consecutive scans
// that fit, the pruning needs all windows at once and says how many bytes that takes when they do not fit -- before any of its
// own work is queued and before an output is written.  After the layout everything is queued in stream order and waited for once.
#include <algorithm>
#include <cmath>
#include <limits.h>
#include <vector>

#include "gn_host.h"
#include "occupancy_host.h"
#include "scan_info_device.h"

using namespace cgmr;

namespace {

constexpr size_t kSiDefaultScratch = (size_t)1 << 30;   // 1 GiB of windows (include/cgmr.h: CGMR_SCAN_INFO_DEFAULT_SCRATCH)

struct PruneArgs {
  const uint8_t* protect;
  int max_remove;
  double budget;
  int32_t* order_out;
  double* delta_out;
  int32_t* n_removed_out;
  double* entropy_after_out;
};

struct InfoOut {
  double* delta;
  int32_t* cells;
  int64_t *hit_sum, *miss_sum;
};

int scan_info_driver(cgmr_ctx* ctx, const char* who, const cgmr_occupancy_config* cfg, int n_scans, int n_beams, const float* ranges,
                     const double* poses, long long scratch_limit, const InfoOut* info, const PruneArgs* prune, int32_t* hits_out,
                     int32_t* misses_out, double* entropy_out, double* kernel_seconds_out) {
  if (!occ_args_ok(cfg, n_scans, n_beams, ranges, poses) || cfg->gain < 0 || scratch_limit < 0)
    return set_err(ctx, CGMR_E_INVALID, "%s: bad argument", who);
  int n_rounds = 0;
  if (prune) {
    if (prune->max_remove < 0) return set_err(ctx, CGMR_E_INVALID, "%s: max_remove < 0", who);
    if (std::isnan(prune->budget)) return set_err(ctx, CGMR_E_INVALID, "%s: max_entropy_increase is not a number", who);
    int n_cand = 0;
    for (int s = 0; s < n_scans; s++) n_cand += !(prune->protect && prune->protect[s]);
    n_rounds = std::min(prune->max_remove, n_cand);
    if (!prune->n_removed_out || (std::min(prune->max_remove, n_scans) > 0 && (!prune->order_out || !prune->delta_out)))
      return set_err(ctx, CGMR_E_INVALID, "%s: order_out, delta_out and n_removed_out are needed", who);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const OccParams P = occ_params(cfg, n_scans, n_beams);
  const size_t ncells = (size_t)P.rows * P.cols, nS = (size_t)n_scans, nS1 = std::max(nS, (size_t)1);
  hipStream_t st = ctx->stream;

  // ---- inputs (staging arena) and the bounding boxes
  Layout256 A;
  const size_t o_scans = A.add(sizeof(OccScan) * nS1), o_cs = A.add(sizeof(float2) * (size_t)n_beams), o_bbox = A.add(sizeof(int4) * nS1);
  const size_t hbytes = A.off;
  const size_t o_ranges = A.add(4 * nS1 * (size_t)n_beams), o_prot = A.add(nS1);
  int rc = arena_reserve(ctx, ctx->io_arena, A.off + 256);
  if (rc) return rc;
  rc = pinned_reserve(ctx, hbytes);
  if (rc) return rc;
  occ_fill_scans(cfg, n_scans, poses, reinterpret_cast<OccScan*>(ctx->pinned + o_scans));
  occ_fill_beams(cfg, n_beams, reinterpret_cast<float2*>(ctx->pinned + o_cs));
  for (size_t s = 0; s < nS; s++) reinterpret_cast<int4*>(ctx->pinned + o_bbox)[s] = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
  char* a = ctx->io_arena.ptr;
  const float* d_ranges = (const float*)(a + o_ranges);
  const OccScan* d_scans = (const OccScan*)(a + o_scans);
  const float2* d_cs = (const float2*)(a + o_cs);
  std::vector<int4> bbox(nS);
  float ms_pre = 0;
  if (n_scans > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(a, ctx->pinned, hbytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(a + o_ranges, ranges, 4 * nS * (size_t)n_beams, hipMemcpyHostToDevice, st));
    if (prune && prune->protect) HIP_TRY(ctx, hipMemcpyAsync(a + o_prot, prune->protect, nS, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_a, st));
    launch_si_bbox(st, P, d_ranges, d_scans, d_cs, (int4*)(a + o_bbox));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_b, st));
    HIP_TRY(ctx, hipMemcpyAsync(bbox.data(), a + o_bbox, sizeof(int4) * nS, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipGetLastError());
    (void)hipEventElapsedTime(&ms_pre, ctx->ev_a, ctx->ev_b);
  }

  // ---- the windows: where each starts, how many partial sums it gives, the chunks
  const size_t limit = scratch_limit > 0 ? (size_t)scratch_limit : kSiDefaultScratch;
  std::vector<SiWindow> win(nS1);
  std::vector<int> chunk_first;                 // first scan of every chunk
  std::vector<size_t> chunk_size;               // and the bytes of its windows
  size_t total_bytes = 0, largest = 0, chunk_bytes = 0, chunk_cap = 0, n_part_all = 0;
  int max_part = 1;
  for (size_t s = 0; s < nS; s++) {
    SiWindow& W = win[s];
    const int4 b = bbox[s];
    const bool any = b.z >= b.x && b.w >= b.y;
    // the walk reports cells of the map only; the clamp costs nothing and keeps the layout inside it whatever came back
    W.x0 = any ? std::max(b.x, 0) : 0; W.y0 = any ? std::max(b.y, 0) : 0;
    W.x1 = any ? std::min(b.z, P.rows - 1) : -1; W.y1 = any ? std::min(b.w, P.cols - 1) : -1;
    const size_t cells = any ? (size_t)(W.x1 - W.x0 + 1) * (size_t)(W.y1 - W.y0 + 1) : 0, bytes = sizeof(int2) * cells;
    if (cells > (size_t)INT_MAX) return set_err(ctx, CGMR_E_INVALID, "%s: scan %zu has a window of %zu cells", who, s, cells);
    if (bytes > limit)
      return set_err(ctx, CGMR_E_ALLOC, "%s: the window of scan %zu alone needs %zu bytes of scratch, the limit is %zu", who, s, bytes, limit);
    if (chunk_first.empty() || (!prune && chunk_bytes + bytes > limit)) { chunk_first.push_back((int)s); chunk_size.push_back(0); chunk_bytes = 0; }
    W.off = (long long)(chunk_bytes / sizeof(int2));
    W.part_off = (long long)n_part_all;
    W.n_part = (int)((cells + kSiCellsPerBlock - 1) / kSiCellsPerBlock);
    W.pad = 0;
    n_part_all += (size_t)W.n_part;
    max_part = std::max(max_part, W.n_part);
    chunk_bytes += bytes;
    chunk_size.back() = chunk_bytes;
    chunk_cap = std::max(chunk_cap, chunk_bytes);
    total_bytes += bytes;
    largest = std::max(largest, bytes);
  }
  if (prune && total_bytes > limit)
    return set_err(ctx, CGMR_E_ALLOC, "%s: the windows of %d scans need %zu bytes of scratch at once, the limit is %zu", who, n_scans,
                   total_bytes, limit);
  chunk_first.push_back(n_scans);
  const int n_chunks = n_scans > 0 ? (int)chunk_first.size() - 1 : 0;

  // ---- work space (matcher arena)
  const int n_epart = (int)((ncells + kSiCellsPerBlock - 1) / kSiCellsPerBlock);
  const size_t nR = (size_t)std::max(n_rounds, 1);
  Layout256 B;
  const size_t o_hits = B.add(4 * ncells), o_miss = B.add(4 * ncells), o_win = B.add(sizeof(SiWindow) * nS1),
               o_part = B.add(sizeof(SiPartial) * std::max(n_part_all, (size_t)1)), o_epart = B.add(8 * (size_t)n_epart), o_ent = B.add(16),
               o_delta = B.add(8 * nS1), o_ncell = B.add(4 * nS1), o_hs = B.add(8 * nS1), o_ms = B.add(8 * nS1), o_alive = B.add(nS1),
               o_state = B.add(sizeof(SiState)), o_order = B.add(4 * nR), o_taken = B.add(8 * nR), o_cells = B.add(std::max(chunk_cap, (size_t)8));
  rc = arena_reserve(ctx, ctx->mt_arena, B.off + 256);
  if (rc) return rc;
  char* d = ctx->mt_arena.ptr;
  int32_t *d_hits = (int32_t*)(d + o_hits), *d_miss = (int32_t*)(d + o_miss);
  const SiWindow* d_win = (const SiWindow*)(d + o_win);
  int2* d_cells = (int2*)(d + o_cells);
  SiPartial* d_part = (SiPartial*)(d + o_part);
  double *d_ent = (double*)(d + o_ent), *d_delta = (double*)(d + o_delta);
  SiState* d_state = (SiState*)(d + o_state);
  const SiState state0{0.0, 0, 0, -1, 0};

  if (n_scans > 0) HIP_TRY(ctx, hipMemcpyAsync(d + o_win, win.data(), sizeof(SiWindow) * nS, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(d_hits, 0, 4 * ncells, st));
  HIP_TRY(ctx, hipMemsetAsync(d_miss, 0, 4 * ncells, st));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, st));
  launch_occ_integrate(st, P, d_ranges, d_scans, d_cs, d_hits, d_miss);
  launch_si_entropy(st, (int)ncells, d_hits, d_miss, (double*)(d + o_epart), d_ent);
  if (!prune) {
    for (int c = 0; c < n_chunks; c++) {
      const int s0 = chunk_first[c], n = chunk_first[c + 1] - s0;
      const size_t bytes = chunk_size[c];
      if (bytes) HIP_TRY(ctx, hipMemsetAsync(d_cells, 0, bytes, st));
      launch_si_windows(st, P, s0, n, d_ranges, d_scans, d_cs, d_win, d_cells);
      launch_si_delta(st, P, s0, n, max_part, d_win, d_cells, d_hits, d_miss, d_part, nullptr, nullptr, 1, d_delta,
                      (int32_t*)(d + o_ncell), (long long*)(d + o_hs), (long long*)(d + o_ms));
    }
  } else if (n_scans > 0) {
    if (total_bytes) HIP_TRY(ctx, hipMemsetAsync(d_cells, 0, total_bytes, st));
    HIP_TRY(ctx, hipMemsetAsync(d + o_alive, 1, nS, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_state, &state0, sizeof state0, hipMemcpyHostToDevice, st));
    launch_si_windows(st, P, 0, n_scans, d_ranges, d_scans, d_cs, d_win, d_cells);
    const uint8_t* d_prot = prune->protect ? (const uint8_t*)(a + o_prot) : nullptr;
    for (int k = 0; k < n_rounds; k++) {
      launch_si_delta(st, P, 0, n_scans, max_part, d_win, d_cells, d_hits, d_miss, d_part, d_state, (const uint8_t*)(d + o_alive), k == 0,
                      d_delta, nullptr, nullptr, nullptr);
      launch_si_pick(st, n_scans, prune->max_remove, prune->budget, d_delta, (uint8_t*)(d + o_alive), d_prot, d_state,
                     (int32_t*)(d + o_order), (double*)(d + o_taken));
      launch_si_subtract(st, P, max_part, d_win, d_cells, d_state, d_hits, d_miss);
    }
    launch_si_entropy(st, (int)ncells, d_hits, d_miss, (double*)(d + o_epart), d_ent + 1);
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));

  // ---- results: staged on the host, handed out after the one wait
  auto down = [&](void* dst, size_t o, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, d + o, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
  double ent[2] = {0, 0};
  SiState fin = state0;
  std::vector<int32_t> order(nR);
  std::vector<double> taken(nR);
  HIP_TRY(ctx, down(ent, o_ent, 16));
  if (prune && n_scans > 0) {
    HIP_TRY(ctx, down(&fin, o_state, sizeof fin));
    if (n_rounds > 0) { HIP_TRY(ctx, down(order.data(), o_order, 4 * nR)); HIP_TRY(ctx, down(taken.data(), o_taken, 8 * nR)); }
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipGetLastError());
  // the caller's arrays last: a HIP error above leaves them as they were
  HIP_TRY(ctx, down(hits_out, o_hits, 4 * ncells));
  HIP_TRY(ctx, down(misses_out, o_miss, 4 * ncells));
  if (info) {
    HIP_TRY(ctx, down(info->delta, o_delta, 8 * nS));
    HIP_TRY(ctx, down(info->cells, o_ncell, 4 * nS));
    HIP_TRY(ctx, down(info->hit_sum, o_hs, 8 * nS));
    HIP_TRY(ctx, down(info->miss_sum, o_ms, 8 * nS));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (entropy_out) *entropy_out = ent[0];
  if (prune) {
    for (int k = 0; k < fin.n_removed; k++) { prune->order_out[k] = order[k]; prune->delta_out[k] = taken[k]; }
    *prune->n_removed_out = fin.n_removed;
    if (prune->entropy_after_out) *prune->entropy_after_out = n_scans > 0 ? ent[1] : ent[0];
  }
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  if (kernel_seconds_out) *kernel_seconds_out = 1e-3 * ((double)ms + (double)ms_pre);
  ctx->si_stats[0] = (int64_t)total_bytes;
  ctx->si_stats[1] = n_chunks;
  ctx->si_stats[2] = (int64_t)largest;
  ctx->si_stats[3] = n_rounds;
  return CGMR_OK;
}

}  // namespace

extern "C" int cgmr_scan_information(cgmr_ctx* ctx, const cgmr_occupancy_config* cfg, int n_scans, int n_beams, const float* ranges,
                                     const double* robot_poses_xyt, int64_t scratch_bytes_limit, double* delta_out, int32_t* cells_out,
                                     int64_t* hit_sum_out, int64_t* miss_sum_out, int32_t* hits_out, int32_t* misses_out,
                                     double* map_entropy_out, double* kernel_seconds_out) {
  if (!ctx) return CGMR_E_INVALID;
  const InfoOut info{delta_out, cells_out, hit_sum_out, miss_sum_out};
  return scan_info_driver(ctx, "cgmr_scan_information", cfg, n_scans, n_beams, ranges, robot_poses_xyt, scratch_bytes_limit, &info,
                          nullptr, hits_out, misses_out, map_entropy_out, kernel_seconds_out);
}

extern "C" int cgmr_scan_prune(cgmr_ctx* ctx, const cgmr_occupancy_config* cfg, int n_scans, int n_beams, const float* ranges,
                               const double* robot_poses_xyt, const uint8_t* protected_or_null, int max_remove,
                               double max_entropy_increase, int64_t scratch_bytes_limit, int32_t* order_out, double* delta_out,
                               int32_t* n_removed_out, double* entropy_before_out, double* entropy_after_out, int32_t* hits_out,
                               int32_t* misses_out, double* kernel_seconds_out) {
  if (!ctx) return CGMR_E_INVALID;
  const PruneArgs pr{protected_or_null, max_remove, max_entropy_increase, order_out, delta_out, n_removed_out, entropy_after_out};
  return scan_info_driver(ctx, "cgmr_scan_prune", cfg, n_scans, n_beams, ranges, robot_poses_xyt, scratch_bytes_limit, nullptr, &pr,
                          hits_out, misses_out, entropy_before_out, kernel_seconds_out);
}

extern "C" int cgmr_scan_info_last_stats(const cgmr_ctx* ctx, int64_t out[4]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  for (int k = 0; k < 4; k++) out[k] = ctx->si_stats[k];
  return CGMR_OK;
}
