// Parameters shared by the matcher kernels and their host launcher.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace cgmr {

constexpr int kMatchMaxPoints = 1088;        // beams per scan (1081 for the reference's laser), multiple of 64
constexpr int kMatchDirGuardY = 7;           // directory guard band along y: 3 tile columns below, 4 above
constexpr int kMatchMaxDir = 152 * 157;      // 8x8-cell tiles of the largest grid (1200 x 1200 cells) + guard band
constexpr int kMatchTilesLds = 1248;         // tiles resident in LDS; the rest spills to HBM
constexpr int kMatchMaxTheta = 80;           // search angles per region
constexpr int kMatchMaxRefScans = 6;         // scans of a close-matching reference set (graph_slam.cpp:230-244: last vertex + 5)

struct MatchParams {
  int n_pairs, n_beams;
  int n_ref_scans;                           // scans per reference set of the batched close matcher (1..kMatchMaxRefScans)
  int prune;                                 // close matcher: 1 = pruned search (exact winner; the per-pair count of populated bins is not produced)
  int split;                                 // close matcher: workgroups per pair (each takes every split-th batch of search angles);
                                             // 1 in batch mode, > 1 for a single call's latency (k_match_close_batch)
  // grid (ScanMatcher::initializeGrid, src/matcher/scan_matcher.cpp:63-66; gridmap.h:196-214)
  float ll_x, ll_y, res, inv_res;
  int nx, ny;
  int kscale, fill, kdim;                    // fill = K2 = int(kernelRange * kscale)
  int sort32;                                // close matcher: the subsample's sort keys fit 32 bits (cells within +-512, beams < 2048)
  int edt;                                   // 1: the kernel value is a non-decreasing function of the squared cell distance (radius <= 8):
                                             // grids are rasterised by an exact distance transform instead of stamping
  // laser (RobotLaser / LaserParameters) and the pose of the laser on the robot
  double max_range, min_range;
  double lp_c, lp_s, lp_x, lp_y;             // cos/sin of the laser pose angle (host libm), translation
  // search (closeScanMatching: scan_matcher.cpp:148-151)
  double win_x, win_y, win_t, theta_res, max_score, dx, dy, dth, sub_res;
  int x_steps, y_steps;
  int overflow_tiles;
  size_t scratch_stride;
  size_t cellmap_off;                        // multi-scan reference sets: byte offset of the workgroup's cell bitmap (nx * ny bits,
                                             // all zero between pairs) inside its scratch; 0 = none
  // generic multi-region search (k_match_greedy)
  int n_ref, n_qry, n_regions, n_items;
  int ref_cap;                               // packed-cell slots per point list in the HBM scratch (>= n_ref, n_qry)
  int bx0, by0, bt0, nbx, nby, nbt;          // bounding box of the result bins over all regions
  int cand_per_pass;                         // k_match_greedy: candidates a work unit sums (128, 256 or kMatchCandPerPass; 0 = the latter): few
                                             // items with many candidates each are cut finer, so that the launch fills the chip
};

constexpr int kMatchMaxRef = 1 << 22;        // sanity limit on the points of one generic search (any number of scans)

struct RegionDesc {                          // one search region, precomputed on the host exactly like
  int32_t lo_x, lo_y;                        //   CharGrid::greedySearch does (chargrid.cpp:235-239)
  int32_t ni, nj;                            // candidates along x / y
  int32_t nth, th_off;                       // angles of this region: theta[th_off .. th_off + nth)
  int32_t thread;                            // which of the reference's <= 4 OpenMP result maps it feeds
  uint32_t order_base;                       // visit order of its first candidate inside that map
};

// One search of a batched k_match_greedy launch (own reference / query points, regions, result maps)
struct GreedyJob {
  int32_t ref_off, n_ref;                    // points into the launch's reference / query point arrays
  int32_t qry_off, n_qry;
  int32_t item_off, n_items;                 // its (region, angle) work items
  int32_t bx0, by0, bt0, nbx, nby, nbt;      // bounding box of its result bins
  int32_t block0, n_blocks;                  // workgroups [block0, block0 + n_blocks) serve it
  int64_t bins_off;                          // first key of its result maps (num_threads * nbins keys)
  int32_t region_off, n_regions;             // its regions in the launch's region table
  int32_t n_threads;                         // result maps it fills: min(n_regions, 4) (chargrid.cpp:228)
  int32_t n_passes;                          // candidate passes of its largest region (MatchParams::cand_per_pass candidates each): a work unit of the
                                             // launch is (item, pass) -- an item's passes spread over workgroups
};
constexpr int kMatchCandPerPass = 576;       // most candidates a workgroup of k_match_greedy sums at a time (24 x 24)

// The level loop of CharGrid::hierarchicalSearch on the device (chargrid.cpp:310-344, 376-400): between two levels' launches of
// k_match_greedy, k_hier_next decodes a job's result maps, sorts the results by score and writes the next level's tables -- a
// region of half a bin around every result -- or, after the last level, the sorted results.  Every job owns fixed slices of the
// tables (cap_* entries each); a job that outgrows one raises err[8] and the host runs the call level by level instead.
struct HierStep {
  // the level just searched
  const GreedyJob* jobs;
  const RegionDesc* regions;
  const double* theta;
  const unsigned long long* bins;
  int x_steps, y_steps;
  // the next level (final: none, the results go to `results`)
  int final_level;
  GreedyJob* jobs_next;
  RegionDesc* regions_next;
  double* theta_next;
  int32_t* items_next;
  unsigned long long* bins_next;
  int x_steps_next, y_steps_next;
  double half_x, half_y, half_t;             // half a bin of the level just searched
  double theta_res_next, dx_next, dy_next, dth_next;
  int cap_regions, cap_theta, cap_items;     // per job
  long long cap_bins_next;                   // keys per job
  int blocks_per_job;
  int cand_per_pass_next;                    // MatchParams::cand_per_pass of the next level's launch
  // results of the last level: per job a count (in counts[job]) and cap_regions x (x, y, theta, score)
  double* results;
  int* counts;
};

// One verifyMatching of a batched k_match_verify launch
struct VerifyJob {
  int32_t p2_off, n2, p1_off, n1;            // points into the launch's pts2 / pts1 arrays
  int32_t lo_x, lo_y, hi_x, hi_y;            // countPoints window in cells
};

// The response surface of a correlative search (k_match_response / k_match_response_finish; the definition is in include/cgmr.h,
// "Scan-match covariance"): what a workgroup leaves per launch, and the result of a job -- the layout of struct cgmr_match_response.
constexpr int kRespSums = 12;                // mass, 3 first moments, 6 second moments (xx xy xt yy yt tt), border mass, candidate count
struct MatchResponse {
  double mean[3], cov[9], info[9];
  double mass, border_mass;
  int64_t n_candidates;
  int32_t status, reserved;
};

// info = (J (cov + floor) J^T)^-1 with floor = diag(step_x^2, step_y^2, theta_res^2) / 12 and J = blockdiag(R(theta*)^T, 1), the inverse
// by cofactors; cs / sn = cos / sin of theta*.  False (info left zero) when the matrix is not invertible in double.
__host__ __device__ inline bool match_response_information(const double* cov, double cs, double sn, double step_x, double step_y,
                                                           double theta_res, double* info) {
  double C[3][3], M[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[i][j] = cov[3 * i + j];
  C[0][0] += step_x * step_x / 12.;
  C[1][1] += step_y * step_y / 12.;
  C[2][2] += theta_res * theta_res / 12.;
  const double J[3][3] = {{cs, sn, 0.}, {-sn, cs, 0.}, {0., 0., 1.}};
  double JC[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) JC[i][j] = J[i][0] * C[0][j] + J[i][1] * C[1][j] + J[i][2] * C[2][j];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) M[i][j] = JC[i][0] * J[j][0] + JC[i][1] * J[j][1] + JC[i][2] * J[j][2];
  const double c00 = M[1][1] * M[2][2] - M[1][2] * M[2][1], c01 = M[1][2] * M[2][0] - M[1][0] * M[2][2],
               c02 = M[1][0] * M[2][1] - M[1][1] * M[2][0];
  const double det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
  for (int q = 0; q < 9; q++) info[q] = 0.;
  if (!(det > 0.) || !(1. / det < 1.7976931348623157e308)) return false;
  const double id = 1. / det;
  info[0] = c00 * id;
  info[1] = (M[0][2] * M[2][1] - M[0][1] * M[2][2]) * id;
  info[2] = (M[0][1] * M[1][2] - M[0][2] * M[1][1]) * id;
  info[3] = c01 * id;
  info[4] = (M[0][0] * M[2][2] - M[0][2] * M[2][0]) * id;
  info[5] = (M[0][2] * M[1][0] - M[0][0] * M[1][2]) * id;
  info[6] = c02 * id;
  info[7] = (M[0][1] * M[2][0] - M[0][0] * M[2][1]) * id;
  info[8] = (M[0][0] * M[1][1] - M[0][1] * M[1][0]) * id;
  return true;
}

// Refining a match below the grid's resolution (k_match_refine; the definition is in include/cgmr.h, "Refining a match"): the
// numerical settings of a launch and the result of a job -- the layouts of cgmr_refine_params and struct cgmr_match_refined.
constexpr int kRefineSums = 12;              // cost, sum of r, b (3), H (xx xy xt yy yt tt), n_active
struct RefineParams {
  int32_t max_iters, max_halvings;
  double ridge, step_tol, bound_steps;
};
struct MatchRefined {
  double pose[3];
  double cost0, cost, score0, score;
  double hessian[9];
  int32_t n_active, n_iters, n_halvings, stop, at_bound, status;
};

// Refinement and response of up to kPolishMaxWinners winners of a job behind one rasterisation (k_match_polish): the result of a
// winner -- the layout of struct cgmr_match_polished.
constexpr int kPolishMaxWinners = 4;
constexpr int kPolishMaxCandidates = 65536;  // angles x cells of a winner's window: one workgroup sums them all
struct MatchPolished {
  MatchResponse response;
  MatchRefined refined;
};

size_t match_smem_bytes();
void launch_match_verify(hipStream_t st, int n_jobs, const MatchParams& P, const VerifyJob* jobs, const double* pts2, const double* pts1,
                         double nonmatched_score, const uint8_t* kernel_lut, unsigned char* scratch, double* score_out,
                         int* nnm_out, int* err);
void launch_match_greedy(hipStream_t st, int nblocks, const MatchParams& P, const GreedyJob* jobs, const int32_t* block_job,
                         const double* ref_pts, const double* qry_pts, const RegionDesc* regions, const double* theta,
                         const int32_t* items, const uint8_t* kernel_lut, unsigned char* scratch, unsigned long long* bins,
                         int* err, unsigned char* grid_cache = nullptr, size_t grid_cache_stride = 0, int grid_cache_mode = 0);
// The response surface of every job of a k_match_greedy job table (one region per job): `partials` holds kRespSums doubles per
// workgroup of the launch, winners 4 doubles (x, y, theta, score) and found one flag per job -- all device memory.
void launch_match_response(hipStream_t st, int nblocks, int n_jobs, const MatchParams& P, const GreedyJob* jobs, const int32_t* block_job,
                           const double* ref_pts, const double* qry_pts, const RegionDesc* regions, const double* theta,
                           const int32_t* items, const uint8_t* kernel_lut, unsigned char* scratch, int* err, const double* winners,
                           const int32_t* found, double temperature, double* partials, MatchResponse* out);
// The refinement of every job of a k_match_greedy job table, ONE workgroup per job (n_jobs workgroups; the regions, angles and work
// items of the table are not read): winners 4 doubles (x, y, theta, score) and found one flag per job -- all device memory.
void launch_match_refine(hipStream_t st, int n_jobs, const MatchParams& P, const GreedyJob* jobs, const double* ref_pts,
                         const double* qry_pts, const uint8_t* kernel_lut, unsigned char* scratch, int* err, const double* winners,
                         const int32_t* found, const RefineParams& RP, MatchRefined* out);
// Refinement and response of every job's winners, ONE workgroup per job (n_jobs workgroups): the job's regions are its winners'
// windows, winners kPolishMaxWinners x 4 doubles and n_winners one count per job, out kPolishMaxWinners results per job -- all
// device memory.  temperature > 0: take the response; do_refine: refine with RP.
void launch_match_polish(hipStream_t st, int n_jobs, const MatchParams& P, const GreedyJob* jobs, const double* ref_pts,
                         const double* qry_pts, const RegionDesc* regions, const double* theta, const uint8_t* kernel_lut,
                         unsigned char* scratch, int* err, const double* winners, const int32_t* n_winners, double temperature,
                         int do_refine, const RefineParams& RP, MatchPolished* out);
size_t match_grid_image_bytes(const MatchParams& P);     // one job's slot in the grid cache (mode 1: the job's first workgroup stores
                                                         // the rasterised grid there, mode 2: every workgroup loads it instead of rasterising)
void launch_hier_next(hipStream_t st, int n_jobs, const MatchParams& P, const HierStep& H, int* err);
void launch_match_redo_prepare(hipStream_t st, int* err, int n_pairs, int grid_redo, int grid_slow, int slow_cap, const int* redo_list,
                               int* slow_list, uint8_t* out_found, int no_redo);
void launch_match_close_batch(hipStream_t st, int nblocks, int variant, const MatchParams& P, const float* ranges_ref, const double* ref_xform,
                              const float* ranges_qry, const double* guess, const double* beam_cos,
                              const double* beam_sin, const uint8_t* kernel_lut, unsigned char* scratch,
                              double* out_xyt, double* out_score, uint8_t* out_found, int* out_nres, int* err,
                              unsigned long long* gbins, int* arrive, int* redo_list);
bool match_close_lean_ok(const MatchParams& P);
int match_close_max_bins();

}  // namespace cgmr
