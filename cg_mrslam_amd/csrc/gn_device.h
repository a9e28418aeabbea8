// Device-side view of one analysed pose graph (pointers into the context's arena) plus the
// small host-side copies the launch loop needs.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "gn_symbolic.h"

namespace cgmr {

struct GncState;                         // gnc_device.h
struct Switches;                         // switches.h

struct GnDevice {
  const Switches* sw = nullptr;          // the owning context's switches (set by cgmr_ctx_create; copies of the view keep it)
  int nV = 0, nE = 0, nf = 0, nb = 0, nlevels = 0, nfronts = 0;
  // structure (uploaded once per analyse)
  FrontDesc* fronts = nullptr;
  FrontDesc* fronts_lv = nullptr;        // descriptors sorted by level (front q of the level order = fronts[level_fronts[q]])
  int32_t *rows = nullptr, *children = nullptr, *rel = nullptr, *inv = nullptr;
  WorkRec* work = nullptr;          // (front, chunk) work items of k_front_factor, level by level
  int32_t *level_fronts = nullptr, *tiles = nullptr, *blk_dst = nullptr, *b_dst = nullptr, *asm_ptr = nullptr, *asm_src = nullptr, *vperm = nullptr;
  int32_t *ef = nullptr, *et = nullptr;
  int32_t *off_row = nullptr, *off_col = nullptr;   // permuted row / column of every off-diagonal H block
  uint8_t* cmask = nullptr;              // per permuted column: 1 = taken out of the system for this pass (fixed vertex, or
                                         // all of its edges switched off), written before every numeric pass
  // numeric work space
  double *term = nullptr, *Ablk = nullptr, *bvec = nullptr, *yvec = nullptr, *xvec = nullptr, *uvec = nullptr;
  double *Lbuf = nullptr, *Ubuf = nullptr;
  double* Pan = nullptr;                 // assembled panels of all fronts (gn_symbolic.h: FrontDesc::pan_off), zeroed before every assembly
  int64_t pan_doubles = 0;
  bool pan_clean = false;                // the panels are all zero (the last pass's top-block launch cleared them behind itself)
  double* chi2 = nullptr;   // iters+1 values
  int* status = nullptr;
  int* ready = nullptr;                  // per front: work items of the factorisation that have stored their rows of L21 in this pass (k_front_level's hand-off)
  int bwd_chain_level = 0;               // GN levels >= this one are solved backwards in one chained launch (k_solve_bwd<.., 4 or 2>)
  int bwd_chain_wgs = 4;                 // ... by the instance built for this many resident workgroups per CU (choose_bwd_chain)
  // a batch of passes on the same structure (gn_kernels.hip: CGMR_JOB): job j works in this view's numeric buffers moved by
  // j * job_stride bytes, on the poses moved by j * pose_stride bytes; every launch gets a job dimension
  int njobs = 1;
  long long job_stride = 0, pose_stride = 0;
  // top block (k_top_block): the last fronts of the root's chain, handled by one workgroup in LDS
  int top_nfronts = 0, top_c0 = 0, top_ncols = 0, top_nchild = 0, top_nblk = 0;
  int32_t *top_fronts = nullptr, *top_children = nullptr, *top_blocks = nullptr;
  // host copies
  int nlevels_full = 0;                  // tree levels including the top block's (the marginals walk every front)
  std::vector<int32_t> h_flevel_ptr;     // full level lists (level_fronts on the device is the full list as well)
  std::vector<int32_t> h_level_ptr, h_tile_ptr, h_work_ptr;   // Gauss-Newton levels (without the top block)
  std::vector<uint8_t> h_level_leaf;     // per level: 1 if no front of the level has children (leaf variant of the factor kernel)
  std::vector<int32_t> h_level_chunk;    // per level: border rows per work item (kChunkRows, fewer for a level of leaves)
  std::vector<uint8_t> h_level_mergeable; // per level: no front whose tiles run in the level's launch has more than kWorkChildren children
  std::vector<uint8_t> h_level_merge;     // per level: factorisation and update tiles in one launch (choose_fwd_merge)
  std::vector<int32_t> h_level_chrows;   // per level: rows of the factor kernel's F21 staging area (max chunk rows + rhs row)
};

// The trailing arguments of k_linearize's instances (gn_kernels.hip; the comments there say what each does to the pass).  Plain
// structs, passed by value: their names, namespace and field order are the kernels' ABI.  All pointers are device memory.
struct RobustArgs {
  const uint8_t* kind = nullptr;   // [nA] or null: edges [0, nA) take kind[k]; every other edge takes kind0
  const double* delta = nullptr;   // [nA] or null: edges [0, nA) take delta[k]; every other edge takes delta0
  double* stats = nullptr;         // [2 nE] or null: e2 of every edge, then rho1 of every edge (a batch writes none)
  double delta0 = 1.0;
  int kind0 = 0;
};
struct TypedArgs {
  const uint8_t* edge_kind = nullptr;   // [nA]; edges [nA, nE) are CGMR_EDGE_SE2
};
struct GncArgs {
  double* weight = nullptr;          // [nE] (a batch: [nA])
  const double* barc_sq = nullptr;   // [nE]
  const uint8_t* known = nullptr;    // [nE]: 1 = known inlier, weight 1
  const GncState* S = nullptr;
  double* r_out = nullptr;           // [nE] or null: r of every edge
  int mode = 0;                      // gnc_device.h: kGncCompute / kGncReuse / kGncPlain
};
struct MixArgs {
  const int32_t* cptr = nullptr;     // [nE + 1]
  const double* cmeas = nullptr;     // [3 nC]
  const double* cinfo = nullptr;     // [6 nC]
  const double* coff = nullptr;      // [nC]: max_j a_j - a_p >= 0, a = 2 ln w + ln det O (own dimension); 0 for an edge of one component
  int32_t* sel_out = nullptr;        // [nE] or null
};
// The priors of a typed pass, grouped by vertex for k_add_unary: vertex[u] owns the edges edge[ptr[u] .. ptr[u + 1]), ascending.
struct UnaryLists {
  int n = 0;
  const int32_t *vertex = nullptr, *ptr = nullptr, *edge = nullptr;
};

// Numeric edge data of one pass: edges [0, nA) from (meas_a, info_a), [nA, nE) from (meas_b, info_b); edges
// [n_active, nE) are switched off.  Each variant of the linearisation is its argument struct and a flag that says it is
// there; launch_linearize picks the instance from the flags (the table in gn_kernels.hip) and passes the structs as they are.
// Which go together is k_linearize's static_assert: GNC never with robust; a mixture never with robust or GNC, nA == nE, its
// meas_a / info_a not read; typed, a mixture and a chordal stage run one job.  A batch (GnDevice::njobs > 1, the robot graph's
// condensed graphs) is plain, robust without statistics, or gnc_own_only: stored weights ga.weight [nA] shared by every job
// (that instance whatever the job count), edges [nA, nE) weight 1, nothing else of ga read.
struct GnEdges {
  const double *meas_a = nullptr, *info_a = nullptr, *meas_b = nullptr, *info_b = nullptr;
  int nA = 0, n_active = 0;
  bool robust = false, typed = false, gnc = false, gnc_own_only = false, mix = false;
  RobustArgs rk;
  TypedArgs ty;
  UnaryLists unary;
  GncArgs ga;
  MixArgs mx;
  // chordal initialisation (include/cgmr.h: cgmr_chordal_initialize; init_kernels.hip): 0 the Gauss-Newton linearisation, else
  // the linear stage whose records the pass solves -- init_device.h: kChordalRotation / kChordalTranslation.  One job, never
  // with `robust`, `gnc` or `mix`; a rotation pass ends with k_apply_rotation in the place of k_update_poses.
  int chordal_stage = 0;
};
// gn_structure.hip: the assembly lists (asm_ptr: nf + nb + 1, asm_src: one entry per (edge, key)) from the permutation, the
// edge list and the off-diagonal blocks (offbase: nf + 1 column starts into off_row); work space: ekey nE, cnt nf + nb + 3,
// longlist 3 nE / 16 + 1, tmp 3 nE (all int32, device memory).  The tests hold the result of this and of launch_build_maps to
// the host's serial reference, entry for entry (gn_symbolic.h: structure_reference)
struct AsmBuild {
  int nE = 0, nf = 0, nb = 0;
  const int32_t *vperm = nullptr, *ef = nullptr, *et = nullptr, *off_row = nullptr, *offbase = nullptr;
  int32_t *asm_ptr = nullptr, *asm_src = nullptr, *ekey = nullptr, *cnt = nullptr, *longlist = nullptr, *tmp = nullptr;
};
void launch_build_asm(hipStream_t st, const AsmBuild& B);
// rel / inv / blk_dst / b_dst of the uploaded front table (D.fronts, rows, children, top_fronts, off_row), one workgroup per front
// ... and the work records of every front (D.work; rec0: per front its first record and its record count, device memory)
void launch_build_maps(hipStream_t st, const GnDevice& D, const int32_t* offbase, const int32_t* rec0);
void launch_linearize(hipStream_t st, const GnDevice& D, const double* poses, const GnEdges& Ed, int chi_only);
void launch_chi2(hipStream_t st, const GnDevice& D, double* out);
void launch_assemble(hipStream_t st, const GnDevice& D);
void launch_add_unary(hipStream_t st, const GnDevice& D, const GnEdges& Ed);   // the priors' records, behind launch_assemble (typed passes)
void gn_init_kernels();
void launch_factor_level(hipStream_t st, const GnDevice& D, int level, bool write_l11c);
void launch_update_level(hipStream_t st, const GnDevice& D, int level);
void launch_front_level(hipStream_t st, const GnDevice& D, int level, bool write_l11c);
void choose_fwd_merge(GnDevice& D, int slots_div, bool off, bool any_size = false);
void launch_bwd_level(hipStream_t st, const GnDevice& D, int level);
void launch_bwd_chain(hipStream_t st, const GnDevice& D);
int bwd_chain_capacity(int per_cu);
void choose_bwd_chain(GnDevice& D, int slots_div, bool levelwise);
void launch_update(hipStream_t st, const GnDevice& D, double* poses);
void launch_top_block(hipStream_t st, const GnDevice& D, bool store_l, bool write_l11c, bool clear_panels, bool make_z);
// Z = L11^-1 of every front below the top block; with top_too, of the top block's fronts as well (their factor must be in
// Lbuf: launch_top_block(.., store_l))
void launch_invert_fronts(hipStream_t st, const GnDevice& D, bool top_too = false);
// marginals_kernels.hip
// A batch of marginals / labelling passes, one per job of a batched GnDevice (D.njobs): job j's query list, Y, U, Gram and
// covariance buffers are the first job's moved by j * marg_stride bytes; its query count, gauge and output slot come from
// jobs[j] (device memory); est / info of job j go to the given pointers moved by out_slot * est_stride / info_stride bytes.
struct CondJobDev { int32_t nq, gauge, gauge_id, out_slot; };
struct MargBatch {
  const CondJobDev* jobs = nullptr;
  long long marg_stride = 0, est_stride = 0, info_stride = 0, wire_stride = 0;
};
// nK: the query count (batch: the largest of the jobs); batch == nullptr: one pass.  live: D.nfronts * (m / 16) bytes of
// scratch (which fronts carry anything of a group of right-hand sides), no initialisation needed
void launch_marginals(hipStream_t st, const GnDevice& D, int nK, const int32_t* d_qcol, int m, double* Y, double* Uv,
                      double* part, double* G, double* cov, int chunk, int nchunk, uint8_t* live, const MargBatch* batch = nullptr,
                      bool y_is_zero = false);   // y_is_zero: the caller has cleared Y already
void launch_label(hipStream_t st, int nK, const int32_t* d_qvert, int gauge, const double* poses, const double* cov,
                  double* est, double* info, int* flags, const GnDevice* D = nullptr, const MargBatch* batch = nullptr);
// The first half of launch_marginals alone: Y = L^-1 E for the query columns (clear Y, unit columns, forward solve level by level)
void launch_marginals_solve(hipStream_t st, const GnDevice& D, int nK, const int32_t* d_qcol, int m, double* Y, double* Uv,
                            uint8_t* live, const MargBatch* batch = nullptr, bool y_is_zero = false);
// joint_marginals_kernels.hip: 16x16 tiles of Y^T Y beyond the diagonal ones.  A tile is 256 doubles, (row, col) at row * 16 + col.
//   tiles != nullptr: the ntile listed tiles (I, J), J <= I (device memory, 2 ints each), tile t at position t of G
//   tiles == nullptr: every lower tile of the T = m / 16 tile rows, ntile = T (T + 1) / 2, tile (I, J) at I (I + 1) / 2 + J
// The n rows of Y are contracted in nsplit ranges of `rows` rows (joint_gram_split); part: nsplit * ntile tiles of scratch
// (not used with nsplit == 1).
struct JointGram {
  const int32_t* tiles = nullptr;
  long long ntile = 0;
  int rows = 0, nsplit = 1;
  double *part = nullptr, *G = nullptr;
};
// rows per range and number of ranges for nwg workgroups per range: many workgroups walk more rows each
void joint_gram_split(int n, long long nwg, int* rows_out, int* nsplit_out);
void launch_joint_gram(hipStream_t st, int n, int m, const double* Y, const JointGram& J);
// cov [3 nK x 3 nK] from the dense tile set; slot[k]: the query's 4-column group of Y or -1 (zeros)
void launch_joint_extract(hipStream_t st, int nK, const int32_t* slot, const double* G, double* cov);
// aa / ab / bb [nP * 9] from a tile list; pr: per pair the slots of a and b (or -1) and the positions of the tiles of (a, a), (a, b), (b, b)
void launch_pairs_extract(hipStream_t st, int nP, const int32_t* pr, const double* G, double* aa, double* ab, double* bb);
// z = x_a^-1 x_b [nP * 3], its covariance [nP * 9], and with a hypothesis (hyp_meas, hyp_info nullable) its squared Mahalanobis
// distance d2 [nP]; rel / rel_cov / d2 nullable (d2 needs hyp_meas)
void launch_relative_cov(hipStream_t st, int nP, const int32_t* pa, const int32_t* pb, const double* poses, const double* aa,
                         const double* ab, const double* bb, const double* hyp_meas, const double* hyp_info, double* rel,
                         double* rel_cov, double* d2);
// the same per pair of kind[p] = 0; kind 1 / 2: the predicted EDGE_SE2_XY / EDGE_BEARING_SE2_XY observation of point b from pose
// a, its covariance and d2 in the factor's own dimension, padded with zeros (cgmr_observation_covariance)
void launch_observation_cov(hipStream_t st, int nP, const int32_t* pa, const int32_t* pb, const uint8_t* kind, const double* poses,
                            const double* aa, const double* ab, const double* bb, const double* hyp_meas, const double* hyp_info,
                            double* z, double* cov, double* d2);
// selinv_kernels.hip: all-pose marginals by selected inversion of the factor in D.Lbuf (gn_pass(.., write_l11c) followed by
// launch_invert_fronts(.., top_too)).  Sig: every front's dense (w + r)^2 block of H^-1 at soff[front] doubles;
// tiles: (front, first border row) pairs of every front with a border, level by level, kSelinvTileRows rows each, the
// level's entries at [h_tile_ptr[l], h_tile_ptr[l + 1]) (device memory except h_tile_ptr).
constexpr int kSelinvTileRows = 64;
struct SelinvPlan {
  double* Sig = nullptr;
  const int64_t* soff = nullptr;
  const int32_t* tiles = nullptr;
  std::vector<int32_t> h_tile_ptr;
};
// vcol: per vertex its permuted column or -1 (fixed / inactive: zeros); col_front: per permuted column its front.
// cov [nV * 9]; cross (nullable) [nE * 9] for the edges D.ef / D.et.
void launch_selinv(hipStream_t st, const GnDevice& D, const SelinvPlan& P, int nV, int nE, const int32_t* vcol,
                   const int32_t* col_front, double* cov, double* cross);

}  // namespace cgmr
