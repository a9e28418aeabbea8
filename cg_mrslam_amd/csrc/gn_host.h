// Host-side drivers of the Gauss-Newton path shared by the solver's translation units (gn_host.cpp, optimize_host.cpp,
// marginals_host.cpp, cgmr_api.cpp, cgmr_debug.cpp) and the robot graph's (robot_graph.h).
#pragma once
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "cgmr_ctx.h"

#define HIP_TRY(ctx, call)                                                                      \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) return set_err(ctx, CGMR_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

namespace cgmr {

// a robust kernel kind (include/cgmr.h: CGMR_RK_*) with its delta as the entry points accept them: a known kind, and a finite
// delta > 0 unless the kind is CGMR_RK_NONE
inline bool robust_valid(int kind, double delta) {
  return kind == CGMR_RK_NONE || (kind > CGMR_RK_NONE && kind <= CGMR_RK_DCS && std::isfinite(delta) && delta > 0);
}

int pinned_mask_reserve(cgmr_ctx* ctx, size_t bytes);
// ordering + symbolic analysis + structure upload for the edge list, or nothing when the context still holds them
// hub_vertices (nullable): vertices the ordering keeps out of the dissection and eliminates last (gn_symbolic.h: analyze)
int prepare_structure(cgmr_ctx* ctx, int nV, int nE, const int32_t* ef, const int32_t* et, int iters,
                      const int32_t* hub_vertices = nullptr, int n_hub_vertices = 0);
// per numeric pass on the context's own view and stream: column mask (fixed vertices; vertices without an edge among the first
// n_active), status words; ctx->vmask keeps the per-vertex flags
int prepare_pass(cgmr_ctx* ctx, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et, int n_active);
// n extra copies of the numeric work space of the uploaded structure: D = the first copy's view, *stride_out = bytes from one
// copy to the next
int gn_replicas(cgmr_ctx* ctx, int n, GnDevice& D, size_t* stride_out);
// A block of device or pinned memory laid out field by field, every field on a 256-byte boundary.
struct Layout256 {
  size_t off = 0;
  explicit Layout256(size_t base = 0) : off(base) {}
  size_t add(size_t bytes) { off = (off + 255) & ~size_t(255); const size_t o = off; off += bytes; return o; }
};
// The work space of launch_marginals and launch_label for nq query vertices, from `base` on: query columns | query vertices |
// Y (3 nf x m) | border vectors (rows: Symbolic::rows.size()) | partial Gram sums | G | covariances | the labelled edges'
// estimates, information matrices and flags | live tiles per front; `end`: the first byte behind it.  The two users keep the
// order they always had behind the covariances (flags_first: flags | estimates | information, else estimates | information |
// flags).
struct MargLayout {
  static constexpr int chunk = 2048;
  int m = 0, n = 0, nchunk = 0;
  size_t o_qc = 0, o_qv = 0, o_Y = 0, o_U = 0, o_part = 0, o_G = 0, o_cov = 0, o_est = 0, o_info = 0, o_fl = 0, o_live = 0, end = 0;
  MargLayout() = default;
  MargLayout(int nq, int nf, size_t rows, int nfronts, size_t base = 0, bool flags_first = false)
      : m(((4 * nq + 15) / 16) * 16),   // 4 columns of Y per query (3 + 1 padding): a query never straddles a 16-column tile
        n(3 * nf), nchunk((n + chunk - 1) / chunk) {
    Layout256 L(base);
    o_qc = L.add(4 * (size_t)nq); o_qv = L.add(4 * (size_t)nq); o_Y = L.add(8 * (size_t)n * m);
    o_U = L.add(8 * (3 * rows + 3) * m); o_part = L.add(8 * (size_t)nchunk * 16 * m); o_G = L.add(8 * (size_t)16 * m);
    o_cov = L.add(72 * (size_t)nq);
    if (flags_first) o_fl = L.add(4 * (size_t)nq);
    o_est = L.add(24 * (size_t)nq); o_info = L.add(48 * (size_t)nq);
    if (!flags_first) o_fl = L.add(4 * (size_t)nq);
    o_live = L.add((size_t)(nfronts > 1 ? nfronts : 1) * (m / 16));
    end = L.off;
  }
};
// What a pass does behind its linearisation.  The order of its launches: [panel memset] -> assemble -> after_assemble ->
// the levels -> top block / inversion -> backward solve -> pose update.
struct GnPassOpts {
  int chi_slot = 0;            // slot of D.chi2 that the chi2 launch of a chi-only pass (or of an empty system) writes
  bool chi_only = false;       // linearise + chi2, nothing else
  bool solve = true;           // forward and backward solve behind the factorisation
  bool update_poses = true;    // apply the solved step (false: the caller makes its own step of it first)
  bool write_l11c = false;     // keep what the marginals read of the factor
  // queued between the assembly and the first level (a damping of H's diagonal)
  void (*after_assemble)(hipStream_t st, const GnDevice& D, void* arg) = nullptr;
  void* after_assemble_arg = nullptr;
};
// one pass on a device view (the context's, or a replica with its own numeric work space) and stream: linearise + chi2
// [+ assemble + factor [+ solve [+ update]]]
void gn_pass_on(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, double* d_poses, const GnEdges& Ed, const GnPassOpts& o);
// the same on the context's own view and stream
void gn_pass(cgmr_ctx* ctx, double* d_poses, const GnEdges& Ed, const GnPassOpts& o);
// A bounded device-side wait ran out (status[2]): a hand-off between workgroups that never arrived, not a numerical failure.
inline void count_timeout(cgmr_ctx* ctx) {
  ctx->gn_timeouts++;
  ctx->fwd_merge_any = false;                                  // (the next structures merge only what is certainly resident)
}
// What was not applied is repeated with one launch per kernel and level -- no in-kernel waits.  arm() counts the event,
// switches the view to "no chained backward solve, no merged level" and queues fresh status words (status[1] = it0); the
// view gets back what arm() found when the scope ends, on whichever way the function is left.
struct LevelwiseScope {
  cgmr_ctx* ctx;
  GnDevice& D;
  bool armed = false;
  int chain_was = 0;
  std::vector<uint8_t> merge_was;
  LevelwiseScope(cgmr_ctx* c, GnDevice& d) : ctx(c), D(d) {}
  LevelwiseScope(const LevelwiseScope&) = delete;
  LevelwiseScope& operator=(const LevelwiseScope&) = delete;
  int arm(hipStream_t st, int it0 = 0);
  ~LevelwiseScope() {
    if (!armed) return;
    D.bwd_chain_level = chain_was;
    D.h_level_merge.swap(merge_was);
  }
};
// What a driver solves, on the device: the vertices with their estimates and fixed flags (host), the edge list (host), and the
// vertices the ordering keeps out of the dissection and eliminates last (nullable; gn_symbolic.h: analyze).
struct GnSystem {
  int nV; double* d_poses; const uint8_t* fixed; int nE; const int32_t *ef, *et;
  const int32_t* hub_vertices = nullptr; int n_hub_vertices = 0;
};
inline int prepare_structure(cgmr_ctx* ctx, const GnSystem& S, int iters) {
  return prepare_structure(ctx, S.nV, S.nE, S.ef, S.et, iters, S.hub_vertices, S.n_hub_vertices);
}
// the caller's arrays every *_run fills (all nullable): chi2 [iters + 1], the per-iteration records [iters], *iters_done
struct LmOut { double *chi2, *lambda; int32_t *trials, *iters_done; };
struct DlOut { double *chi2, *delta; int32_t *trials, *step, *iters_done; };
// mu [max_outer], cost [max_outer + 1], partial [max_outer], *outer_done, and -- host memory, written when the call ends well
// or with a Cholesky code, behind the call's own final wait -- weight / edge_chi2 [nE]
struct GncOut { double *mu, *cost; int32_t *partial, *outer_done; double *weight, *edge_chi2; };
int gn_run(cgmr_ctx* ctx, const GnSystem& S, const GnEdges& Ed, int iters, double* chi2_out);
// Chordal initialisation on the same structure preparation and factorisation (include/cgmr.h: cgmr_chordal_initialize): one pass
// per stage of `stages`; in_rot / in_tr [nV] host: the vertices some term of the stage touches; chi2_out [2], counts_out [3] nullable
int chordal_run(cgmr_ctx* ctx, const GnSystem& S, const GnEdges& Ed, int stages, const uint8_t* in_rot, const uint8_t* in_tr,
                double* chi2_out, int32_t* counts_out);
// Levenberg-Marquardt on the same structure preparation and factorisation (g2o's OptimizationAlgorithmLevenberg); never a
// Cholesky status
int lm_run(cgmr_ctx* ctx, const GnSystem& S, const GnEdges& Ed, int iters, const cgmr_lm_params* params, const LmOut& out);
// Dogleg on the same structure preparation and factorisation (g2o's OptimizationAlgorithmDogleg); CGMR_E_CHOLESKY_BASE - i on
// g2o's Fail
int dl_run(cgmr_ctx* ctx, const GnSystem& S, const GnEdges& Ed, int iters, const cgmr_dl_params* params, const DlOut& out);
// null, or parameters dl_run accepts
bool dl_params_ok(const cgmr_dl_params* params);
// Graduated non-convexity with Gauss-Newton inside (include/cgmr.h: cgmr_gnc_optimize), on the same structure preparation:
// P checked by the caller (its per-edge pointers are not read), barc_sq / known host arrays [nE] (every entry set), Ed without a
// robust description.  CGMR_E_CHOLESKY_BASE - i: the poses are those of the last good update.
int gnc_run(cgmr_ctx* ctx, const GnSystem& S, const GnEdges& Ed, const cgmr_gnc_params& P, const double* barc_sq,
            const uint8_t* known, const GncOut& out);
// null, or parameters gnc_run accepts (the per-edge pointers aside); the defaults
bool gnc_params_ok(const cgmr_gnc_params* params);
cgmr_gnc_params gnc_params_default();
// the chi2 0.99 quantile of a factor of dimension 1..3: the default barc^2
double gnc_default_barc_sq(int dim);
// SparseOptimizer::computeInitialGuess from the fixed vertices over the given edges [g2o-recalled]
void initial_guess_host(int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et,
                        const double* meas);
// The analysis of the system's edge list (N: its nV, nE, ef, et and hubs) into `sym`, which holds the analysis of (prev_nV, pef,
// pet) when have_prev: extended from it where the two lists allow that, from scratch otherwise
int analyze_next(Symbolic& sym, const Switches& sw, bool have_prev, int prev_nV, const std::vector<int32_t>& pef, const std::vector<int32_t>& pet,
                 const GnSystem& N, const AnalyzeHooks* hooks = nullptr);
// the 16 figures of cgmr_gn_symbolic_info for an analysis, and its vertex permutation (nullable)
void symbolic_info_out(const Symbolic& S, int nV, int64_t out[16], int32_t* perm_out);
// gn_symbolic.cpp: the helper pool as it runs -- threads an analysis uses (caller included), 1 if the helpers are pinned around
// a last-level cache, the caller's home CPU while it analyses (-1: not pinned), CPUs the process may use, moves of the pool
void host_pool_info(int out[5]);
// profiling mode: add up the event pairs of the launches since the last collection (call after a stream sync)
void profile_collect(cgmr_ctx* ctx);

struct BlobLayout {
  size_t off = 0;
  template <typename T>
  size_t add(size_t count) {
    off = (off + 15) & ~size_t(15);
    size_t o = off;
    off += count * sizeof(T);
    return o;
  }
};

struct KTimer {   // optional per-launch-class timing (profiling mode only)
  cgmr_ctx* ctx;
  hipStream_t st;
  template <typename Fn>
  void run(int cls, int nlaunch, Fn&& fn) {
    if (ctx->sw.trace_launches) {                                 // debugging aid: name every launch, sync after it
      fprintf(stderr, "[cgmr] launch class %d (0 lin 1 asm 2 chi2 3 factor 4 update 5 top 6 bwd 7 poses 8 factor+update)\n", cls);
      fn();
      hipError_t e = hipStreamSynchronize(st);
      fprintf(stderr, "[cgmr]   done: %s\n", hipGetErrorString(e));
      return;
    }
    if (!ctx->profiling || st != ctx->stream || 2 * (ctx->ev_cls.size() + 1) > ctx->ev_pool.size()) { fn(); return; }
    const size_t k = ctx->ev_cls.size();
    (void)hipEventRecord(ctx->ev_pool[2 * k], ctx->stream);
    fn();
    (void)hipEventRecord(ctx->ev_pool[2 * k + 1], ctx->stream);
    ctx->ev_cls.push_back(cls);
    ctx->klaunch[cls] += nlaunch;
  }
};

// What an optimisation call does around its device work, whatever the algorithm: the structure and the masks with their
// wall-clock marks, the timing events, the caller's host copy of the estimates, the wait, cgmr_gn_timing's five entries.
struct GnCall {
  cgmr_ctx* ctx;
  const GnSystem& sys;
  double t0, t1 = 0, t2 = 0;
  double* poses_host = nullptr;
  struct Readback { void* dst; const void* src; size_t bytes; };

  GnCall(cgmr_ctx* c, const GnSystem& s) : ctx(c), sys(s), t0(wall_s()) {}
  // chi_slots: iterations whose chi2 slot the structure's work space must hold
  int prepare(int n_active, int chi_slots) {
    int rc = prepare_structure(ctx, sys, chi_slots);
    if (rc) return rc;
    t1 = wall_s();
    rc = prepare_pass(ctx, sys.fixed, sys.nE, sys.ef, sys.et, n_active);
    t2 = wall_s();
    return rc;
  }
  // the device work starts here (ev0; its end: the last hipEventRecord of ev1 before a wait)
  int begin() {
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    // the caller's host copy of the estimates rides in every wait (a robot graph whose peers have asked for condensed graphs
    // picks their gauges from it right after the solve)
    poses_host = ctx->poses_out_host;
    ctx->poses_out_host = nullptr;
    return 0;
  }
  int wait(std::initializer_list<Readback> what) {
    hipStream_t st = ctx->stream;
    for (const Readback& r : what)
      if (r.bytes) HIP_TRY(ctx, hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost, st));
    if (poses_host && sys.nV > 0) HIP_TRY(ctx, hipMemcpyAsync(poses_host, sys.d_poses, 24 * (size_t)sys.nV, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipGetLastError());
    return 0;
  }
  void finish() {
    const Symbolic& S = ctx->sym;
    if (ctx->profiling) profile_collect(ctx);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->timing[0] = S.t_order;
    ctx->timing[1] = S.t_struct;
    ctx->timing[2] = (t2 - t1) + S.t_upload;     // structure blob (host staging + H2D enqueue) + per-pass masks
    ctx->timing[3] = 1e-3 * ms;
    ctx->timing[4] = wall_s() - t0;
  }
};

}  // namespace cgmr
