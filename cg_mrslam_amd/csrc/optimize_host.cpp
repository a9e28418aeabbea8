// The drivers behind gn_run (gn_host.h): chordal initialisation, and tr_run with its Levenberg-Marquardt, dogleg and GNC policies.
// Compiled with hipcc; contains no kernels.
#include "dl_device.h"
#include "gn_host.h"
#include "gnc_device.h"
#include "init_device.h"
#include "lm_device.h"
#include "tr_device.h"

#include <algorithm>
#include <cstring>

namespace cgmr {

// Chordal initialisation (include/cgmr.h: cgmr_chordal_initialize; init_kernels.hip): one structure, then one pass per
// requested stage -- the stage's mask, gn_pass with the stage in GnEdges -- between two chi-only passes of the ordinary
// linearisation, and one wait.  in_rot / in_tr [nV]: the vertices some term of the stage touches; the others are left out of it
// through its mask like the fixed ones.  The chi2 slots: pass p's own cost in slot p (k_assemble, from status[1]), the SE(2)
// chi2 at the start and at the result in slots 4 and 5.  A non-positive pivot in pass p: status[0] = p + 1, that pass and the
// later ones change nothing (k_apply_rotation and k_update_poses skip), the call returns GN's code for iteration p.
int chordal_run(cgmr_ctx* ctx, const GnSystem& sys, const GnEdges& Ed, int stages, const uint8_t* in_rot, const uint8_t* in_tr,
                double* chi2_out, int32_t* counts_out) {
  constexpr int kSlotStart = 4, kSlotEnd = 5, kSlots = 6;
  GnCall call(ctx, sys);
  int rc = prepare_structure(ctx, sys, kSlots);
  if (rc) return rc;
  call.t1 = wall_s();
  const Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  int seq[2], npass = 0;
  if (stages & kChordalRotation) seq[npass++] = kChordalRotation;
  if (stages & kChordalTranslation) seq[npass++] = kChordalTranslation;
  // the passes' column masks, side by side in pinned memory: they stay as they are until the call's last wait
  rc = pinned_mask_reserve(ctx, (size_t)2 * S.nf + 1);
  if (rc) return rc;
  int solved[2] = {0, 0};
  for (int p = 0; p < npass; p++) {
    const uint8_t* in = seq[p] == kChordalRotation ? in_rot : in_tr;
    ctx->vmask.assign(S.nV, 0);
    for (int v = 0; v < S.nV; v++) ctx->vmask[v] = (sys.fixed[v] || !in[v]) ? 1 : 0;
    char* pm = ctx->pinned_mask + (size_t)p * S.nf;
    for (int c = 0; c < S.nf; c++) {
      pm[c] = (char)ctx->vmask[S.perm[c]];
      solved[p] += pm[c] ? 0 : 1;
    }
  }
  HIP_TRY(ctx, hipMemsetAsync(D.status, 0, 16, st));
  call.t2 = wall_s();
  bool queue_failed = false;
  // the passes p0 .. npass - 1, then the chi-only pass at the estimate they leave
  auto queue_from = [&](int p0) {
    GnPassOpts o;
    for (int p = p0; p < npass; p++) {
      if (S.nf > 0 && hipMemcpyAsync(D.cmask, ctx->pinned_mask + (size_t)p * S.nf, (size_t)S.nf, hipMemcpyHostToDevice, st) != hipSuccess) queue_failed = true;
      GnEdges Es = Ed;
      Es.chordal_stage = seq[p];
      o.chi_slot = p;
      gn_pass(ctx, sys.d_poses, Es, o);
    }
    o.chi_only = true;
    o.chi_slot = kSlotEnd;
    gn_pass(ctx, sys.d_poses, Ed, o);
  };
  rc = call.begin();
  if (rc) return rc;
  {
    GnPassOpts o;
    o.chi_only = true;
    o.chi_slot = kSlotStart;
    gn_pass(ctx, sys.d_poses, Ed, o);
  }
  queue_from(0);
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
  double chi[kSlots] = {0, 0, 0, 0, 0, 0};
  int status4[4] = {0, 0, 0, 0};
  const std::initializer_list<GnCall::Readback> results = {{chi, D.chi2, sizeof chi}, {status4, D.status, sizeof status4}};
  rc = call.wait(results);
  if (rc) return rc;
  int degenerate_kept = 0;
  if (status4[2] != 0 && status4[0] > 0) {
    // A bounded wait of the chained backward solve ran out in pass status[0] - 1: that pass and the later ones were not applied
    // and are repeated level-wise (gn_run).  The fresh status words drop the count of an earlier rotation pass: kept here.
    const int p0 = std::min(status4[0] - 1, npass - 1);
    if (p0 > 0) degenerate_kept = status4[kChordalDegenerateWord];
    LevelwiseScope levelwise(ctx, D);
    rc = levelwise.arm(st, p0);
    if (rc) return rc;
    queue_from(p0);
    rc = call.wait(results);
    if (rc) return rc;
    if (status4[2] != 0) return set_err(ctx, CGMR_E_TIMEOUT, "backward solve: a bounded device-side wait ran out twice");
  }
  if (queue_failed) return set_err(ctx, CGMR_E_HIP, "cgmr_chordal_initialize: a stage's mask could not be queued");
  const int status = status4[0];
  call.finish();
  if (chi2_out) { chi2_out[0] = chi[kSlotStart]; chi2_out[1] = chi[kSlotEnd]; }
  if (counts_out) {
    counts_out[0] = counts_out[1] = 0;
    for (int p = 0; p < npass; p++)
      if (status == 0 || p < status - 1) counts_out[seq[p] == kChordalRotation ? 0 : 1] = solved[p];
    counts_out[2] = status4[kChordalDegenerateWord] + degenerate_kept;
  }
  if (status != 0)
    return set_err(ctx, CGMR_E_CHOLESKY_BASE - (status - 1),
                   "Cholesky failed (non-positive pivot) in the %s stage of the chordal initialisation; poses left as they were before it",
                   seq[std::min(status - 1, npass - 1)] == kChordalRotation ? "rotation" : "translation");
  return CGMR_OK;
}

// Levenberg-Marquardt and dogleg are two policies of one driver.  A policy P supplies
//   State, L (its device buffers; L.S the state, L.saved the saved poses), kName;
//   reserve():      its arena laid out as state | records | work space, L bound to it; the bytes of state + records
//   start():        the state a call begins with;
//   queue_round():  the launches of one round, from the host's copy of the state;
//   also_read():    what a round's wait reads back beside state + records;
//   empty_system(): the closed-form answer when nothing can move, into the host's copy of state + records;
//   finish():       records and statistics out, the call's return code;
//   kRunsEmpty:     its rounds also serve a system with nothing to move (else: empty_system()).
// The driver owns the rest: upload, the saved poses, the rounds with their one wait each, a timed-out round's repeat
// (LevelwiseScope), the final pass of the robust statistics.
template <typename P>
static int tr_run(cgmr_ctx* ctx, P& pol, const GnSystem& sys, const GnEdges& Ed, int iters) {
  GnCall call(ctx, sys);
  // (the chi2 slots a trial uses: slot 0 only -- the cache entry of a Gauss-Newton call on the same edge list serves)
  int rc = call.prepare(Ed.n_active, 1);
  if (rc) return rc;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  size_t rec_bytes = 0;
  rc = pol.reserve(ctx, iters, sys, D.nf, &rec_bytes);
  if (rc) return rc;
  char* const d = (char*)pol.L.S;
  std::vector<char> h(rec_bytes, 0);                          // the host's copy of state + records
  typename P::State hs = pol.start(iters);
  memcpy(h.data(), &hs, sizeof hs);
  HIP_TRY(ctx, hipMemcpyAsync(d, h.data(), rec_bytes, hipMemcpyHostToDevice, st));
  if (sys.nV > 0) HIP_TRY(ctx, hipMemcpyAsync(pol.L.saved, sys.d_poses, 24 * (size_t)sys.nV, hipMemcpyDeviceToDevice, st));
  rc = call.begin();
  if (rc) return rc;
  int64_t waits = 0;
  if ((D.nf == 0 || iters == 0) && !P::kRunsEmpty) {
    // nothing to move (or nothing asked): chi2 at x, and what g2o makes of an empty system
    GnPassOpts chi_pass;
    chi_pass.chi_only = true;
    gn_pass(ctx, sys.d_poses, Ed, chi_pass);
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
    double chi0 = 0;
    rc = call.wait({{&chi0, D.chi2, sizeof(double)}});
    if (rc) return rc;
    waits = 1;
    pol.empty_system(hs, h.data(), chi0, iters);
  } else {
    LevelwiseScope levelwise(ctx, D);
    GnEdges Ei = Ed;                                         // (robust statistics: one chi-only pass on the final poses below)
    Ei.rk.stats = nullptr;
    Ei.mx.sel_out = nullptr;                                    // (a mixture's selection: the same pass)
    for (;;) {
      pol.queue_round(ctx, D, st, sys, Ei, hs, iters);
      HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
      rc = call.wait({{h.data(), d, rec_bytes}, pol.also_read(D)});
      if (rc) return rc;
      waits++;
      memcpy(&hs, h.data(), sizeof hs);
      if (hs.halted) {
        // A bounded wait ran out in a pass (status[2]): not a numerical verdict.  The poses are those the trial started from
        // and nothing queued behind it changed anything; the call goes on from the state as it stands, level-wise.
        if (levelwise.armed) return set_err(ctx, CGMR_E_TIMEOUT, "%s: a bounded device-side wait ran out twice", P::kName);
        rc = levelwise.arm(st);
        if (rc) return rc;
        hs.halted = 0;
        hs.accept = -1;
        HIP_TRY(ctx, hipMemcpyAsync(pol.L.S, &hs, sizeof hs, hipMemcpyHostToDevice, st));
        continue;
      }
      if (hs.done) break;
    }
    if (Ed.rk.stats || Ed.mx.sel_out) launch_linearize(st, D, sys.d_poses, Ed, 1);   // (read back by the caller, behind the stream)
  }
  call.finish();
  return pol.finish(ctx, hs, h.data(), std::min(hs.iter, iters), iters, waits);
}

// records [0, ran) of an iteration's array to the caller's (nullable), zeros behind them
template <typename T>
static void records_out(T* out, const T* rec, int ran, int iters) {
  if (out) for (int k = 0; k < iters; k++) out[k] = k < ran ? rec[k] : T(0);
}
static void chi2_records_out(double* out, const double* rec, int ran, int iters) {
  if (out) for (int k = 0; k <= iters; k++) out[k] = rec[std::min(k, ran)];
}

// g2o's OptimizationAlgorithmLevenberg defaults [g2o-recalled]
static cgmr_lm_params lm_defaults() {
  cgmr_lm_params p;
  p.tau = 1e-5; p.initial_lambda = -1; p.max_trials = 10; p.good_step_lower = 1.0 / 3; p.good_step_upper = 2.0 / 3;
  return p;
}

struct LmPolicy {
  using State = LmState;
  static constexpr const char* kName = "Levenberg-Marquardt";
  static constexpr bool kRunsEmpty = false;
  cgmr_lm_params P;
  LmOut out;
  LmDev L;
  size_t o_chi = 0, o_lam = 0, o_tri = 0;
  int status4[4] = {0, 0, 0, 0};

  // lm arena: state | chi2 records [iters + 1] | lambda records [iters] | trial records [iters] | saved poses [3 nV]
  int reserve(cgmr_ctx* ctx, int iters, const GnSystem& sys, int, size_t* rec_bytes) {
    BlobLayout B;
    B.add<LmState>(1);
    o_chi = B.add<double>((size_t)iters + 1); o_lam = B.add<double>((size_t)iters + 1); o_tri = B.add<int32_t>((size_t)iters + 1);
    *rec_bytes = B.off;
    const size_t o_saved = B.add<double>(3 * (size_t)std::max(sys.nV, 1));
    int rc = arena_reserve(ctx, ctx->lm_arena, B.off + 256);
    if (rc) return rc;
    char* d = ctx->lm_arena.ptr;
    L.S = (LmState*)d; L.rec_chi = (double*)(d + o_chi); L.rec_lambda = (double*)(d + o_lam);
    L.rec_trials = (int32_t*)(d + o_tri); L.saved = (double*)(d + o_saved);
    return 0;
  }
  LmState start(int iters) const {
    LmState hs;
    hs.tau = P.tau; hs.initial_lambda = P.initial_lambda; hs.max_trials = P.max_trials;
    hs.lower = P.good_step_lower; hs.upper = P.good_step_upper; hs.iters = iters;
    return hs;
  }
  static void damp(hipStream_t st, const GnDevice& D, void* self) { launch_lm_damp(st, D, ((LmPolicy*)self)->L.S); }
  static void init_and_damp(hipStream_t st, const GnDevice& D, void* self) {
    launch_lm_init(st, D, ((LmPolicy*)self)->L.S);
    damp(st, D, self);
  }
  // One trial, the same launches whatever happens (lm_kernels.hip): linearise + assemble + damp + factor + solve + update at x,
  // chi-only linearise at x', the verdict, then restore x or keep x'.
  void trial(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, int nV, double* d_poses, const GnEdges& Ed, bool init) {
    GnPassOpts o;
    o.after_assemble = init ? init_and_damp : damp;
    o.after_assemble_arg = this;
    gn_pass_on(ctx, D, st, d_poses, Ed, o);
    launch_linearize(st, D, d_poses, Ed, 1);
    launch_lm_decide(st, D, L);
    launch_tr_commit(st, nV, d_poses, L.saved, &L.S->accept);
  }
  // one trial per iteration still to run; a rejected trial leaves its iteration to the next round
  void queue_round(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, const GnSystem& sys, const GnEdges& Ed, const LmState& hs, int iters) {
    const int n_trials = iters - hs.iter;
    for (int t = 0; t < n_trials; t++) trial(ctx, D, st, sys.nV, sys.d_poses, Ed, t == 0);   // (k_lm_init: a no-op once lambda is set)
  }
  GnCall::Readback also_read(const GnDevice& D) { return {status4, D.status, sizeof status4}; }
  // with iterations asked, the first trial's step is zero, rho = 0: g2o terminates after it, lambda grown once by nu
  void empty_system(LmState& hs, char* h, double chi0, int iters) const {
    hs.iter = iters > 0 ? 1 : 0;
    hs.lambda = 2 * (P.initial_lambda > 0 ? P.initial_lambda : 0.0);
    hs.total_trials = hs.iter;
    double* rc_chi = (double*)(h + o_chi);
    rc_chi[0] = chi0;
    if (hs.iter) { rc_chi[1] = chi0; ((double*)(h + o_lam))[0] = hs.lambda; ((int32_t*)(h + o_tri))[0] = 1; }
  }
  int finish(cgmr_ctx* ctx, const LmState& hs, const char* h, int ran, int iters, int64_t waits) const {
    chi2_records_out(out.chi2, (const double*)(h + o_chi), ran, iters);
    records_out(out.lambda, (const double*)(h + o_lam), ran, iters);
    records_out(out.trials, (const int32_t*)(h + o_tri), ran, iters);
    if (out.iters_done) *out.iters_done = ran;
    ctx->lm_stats[0] = waits;
    ctx->lm_stats[1] = hs.total_trials;
    return CGMR_OK;
  }
};

int lm_run(cgmr_ctx* ctx, const GnSystem& S, const GnEdges& Ed, int iters, const cgmr_lm_params* params, const LmOut& out) {
  const cgmr_lm_params P = params ? *params : lm_defaults();
  if (!(P.max_trials >= 1) || !(P.tau >= 0) || !(P.good_step_lower > 0) || !(P.good_step_upper > 0) || !std::isfinite(P.tau) ||
      !std::isfinite(P.initial_lambda) || !std::isfinite(P.good_step_lower) || !std::isfinite(P.good_step_upper))
    return set_err(ctx, CGMR_E_INVALID, "cgmr_lm_optimize: max_trials must be >= 1, tau >= 0, the step scales > 0, all finite");
  LmPolicy pol{P, out};
  return tr_run(ctx, pol, S, Ed, iters);
}

// g2o's OptimizationAlgorithmDogleg defaults [g2o-recalled]
static cgmr_dl_params dl_defaults() {
  cgmr_dl_params p;
  p.initial_delta = 1e4; p.max_trials = 100; p.initial_lambda = 1e-7; p.lambda_factor = 10;
  return p;
}

static bool dl_params_valid(const cgmr_dl_params& P) {
  return P.max_trials >= 1 && std::isfinite(P.initial_delta) && P.initial_delta > 0 && std::isfinite(P.initial_lambda) &&
         P.initial_lambda > 0 && std::isfinite(P.lambda_factor) && P.lambda_factor > 1;
}

bool dl_params_ok(const cgmr_dl_params* p) { return !p || dl_params_valid(*p); }

struct DlPolicy {
  using State = DlState;
  static constexpr const char* kName = "dogleg";
  static constexpr bool kRunsEmpty = false;
  cgmr_dl_params P;
  DlOut out;
  DlDev L;
  size_t o_chi = 0, o_del = 0, o_tri = 0, o_stp = 0;
  int n_cont = 1;                                            // tails the last round gave an open iteration

  // dl arena: state | chi2 [iters + 1] | delta, trials, steps [iters] | saved poses [3 nV] | hgn, hsd [3 nf] | quad partials
  int reserve(cgmr_ctx* ctx, int iters, const GnSystem& sys, int nf, size_t* rec_bytes) {
    BlobLayout B;
    B.add<DlState>(1);
    o_chi = B.add<double>((size_t)iters + 1); o_del = B.add<double>((size_t)iters + 1);
    o_tri = B.add<int32_t>((size_t)iters + 1); o_stp = B.add<int32_t>((size_t)iters + 1);
    *rec_bytes = B.off;
    const size_t nf3 = 3 * (size_t)std::max(nf, 1);
    const size_t o_saved = B.add<double>(3 * (size_t)std::max(sys.nV, 1)), o_hgn = B.add<double>(nf3), o_hsd = B.add<double>(nf3),
                 o_q = B.add<double>((size_t)std::max((sys.nE + 255) / 256, 1));
    int rc = arena_reserve(ctx, ctx->dl_arena, B.off + 256);
    if (rc) return rc;
    char* d = ctx->dl_arena.ptr;
    L.S = (DlState*)d; L.rec_chi = (double*)(d + o_chi); L.rec_delta = (double*)(d + o_del);
    L.rec_trials = (int32_t*)(d + o_tri); L.rec_step = (int32_t*)(d + o_stp); L.saved = (double*)(d + o_saved);
    L.hgn = (double*)(d + o_hgn); L.hsd = (double*)(d + o_hsd); L.qpart = (double*)(d + o_q);
    return 0;
  }
  DlState start(int iters) const {
    DlState hs;
    hs.delta = P.initial_delta; hs.lambda = P.initial_lambda; hs.lambda_factor = P.lambda_factor; hs.max_trials = P.max_trials;
    hs.iters = iters;
    return hs;
  }
  static void damp(hipStream_t st, const GnDevice& D, void* self) { launch_dl_damp(st, D, ((DlPolicy*)self)->L.S); }
  // A head (dl_kernels.hip): linearise + assemble + [damp] + factor + solve at x (the step is left to the tails), b^T H b,
  // k_dl_begin.
  void head(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, double* d_poses, const GnEdges& Ed) {
    GnPassOpts o;
    o.update_poses = false;
    o.after_assemble = damp;
    o.after_assemble_arg = this;
    gn_pass_on(ctx, D, st, d_poses, Ed, o);
    launch_dl_quad(st, D, D.bvec, L.qpart);
    launch_dl_begin(st, D, L);
  }
  // A tail: the step for the current delta, h^T H h, update, chi-only linearise at x (+) h, the verdict, keep or restore x.
  void tail(GnDevice& D, hipStream_t st, int nV, double* d_poses, const GnEdges& Ed) {
    launch_dl_step(st, D, L);
    launch_dl_quad(st, D, D.xvec, L.qpart);
    launch_update(st, D, d_poses);
    launch_linearize(st, D, d_poses, Ed, 1);
    launch_dl_decide(st, D, L);
    launch_tr_commit(st, nV, d_poses, L.saved, &L.S->accept);
  }
  // an open iteration (its GN step solved, no good step yet) gets tails only, doubling in number from round to round; every
  // iteration not started yet gets a head and a tail
  void queue_round(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, const GnSystem& sys, const GnEdges& Ed, const DlState& hs, int iters) {
    const bool open = hs.solved != 0;
    if (open) {
      n_cont = std::min(2 * n_cont, P.max_trials - hs.trial);
      for (int t = 0; t < n_cont; t++) tail(D, st, sys.nV, sys.d_poses, Ed);
    }
    const int n_new = iters - hs.iter - (open ? 1 : 0);
    for (int t = 0; t < n_new; t++) {
      head(ctx, D, st, sys.d_poses, Ed);
      tail(D, st, sys.nV, sys.d_poses, Ed);
    }
  }
  GnCall::Readback also_read(const GnDevice&) { return {nullptr, nullptr, 0}; }
  // with iterations asked, g2o's empty system gives h = 0 and rho = 0 on every trial: one iteration of max_trials GN trials,
  // delta halved on each, Terminate
  void empty_system(DlState& hs, char* h, double chi0, int iters) const {
    double* rc_chi = (double*)(h + o_chi);
    rc_chi[0] = chi0;
    if (iters == 0) return;
    for (int q = 0; q < P.max_trials; q++) hs.delta *= 0.5;
    hs.iter = 1;
    hs.total_trials = P.max_trials;
    hs.terminated = 1;
    rc_chi[1] = chi0;
    ((double*)(h + o_del))[0] = hs.delta;
    ((int32_t*)(h + o_tri))[0] = P.max_trials;
    ((int32_t*)(h + o_stp))[0] = CGMR_DL_STEP_GN;
  }
  int finish(cgmr_ctx* ctx, const DlState& hs, const char* h, int ran, int iters, int64_t waits) const {
    chi2_records_out(out.chi2, (const double*)(h + o_chi), ran, iters);
    records_out(out.delta, (const double*)(h + o_del), ran, iters);
    records_out(out.trials, (const int32_t*)(h + o_tri), ran, iters);
    records_out(out.step, (const int32_t*)(h + o_stp), ran, iters);
    if (out.iters_done) *out.iters_done = ran;
    ctx->dl_stats[0] = waits;
    ctx->dl_stats[1] = hs.total_trials;
    ctx->dl_stats[2] = hs.factorisations;
    if (hs.failed)
      return set_err(ctx, CGMR_E_CHOLESKY_BASE - ran,
                     "dogleg: H + currentLambda I not positive definite with currentLambda at 1e3 in iteration %d (g2o's Fail); "
                     "poses left at the last accepted step", ran);
    return CGMR_OK;
  }
};

int dl_run(cgmr_ctx* ctx, const GnSystem& S, const GnEdges& Ed, int iters, const cgmr_dl_params* params, const DlOut& out) {
  const cgmr_dl_params P = params ? *params : dl_defaults();
  if (!dl_params_valid(P))
    return set_err(ctx, CGMR_E_INVALID,
                   "cgmr_dl_optimize: max_trials must be >= 1, initial_delta / initial_lambda > 0, lambda_factor > 1, all finite");
  DlPolicy pol{P, out};
  return tr_run(ctx, pol, S, Ed, iters);
}


// ------------------------------------------------------------------------------------------------ graduated non-convexity
cgmr_gnc_params gnc_params_default() {
  cgmr_gnc_params p;
  p.loss = CGMR_GNC_TLS; p.mu_factor = 1.4; p.max_outer = 100; p.inner_iters = 1; p.outer_per_wait = 8;
  p.barc_sq = nullptr; p.default_barc_sq = 0.0; p.known_inlier = nullptr; p.weight_out = nullptr; p.edge_chi2_out = nullptr;
  return p;
}

// gnc arena: state | mu, cost [max_outer + 1] | partial [max_outer + 1] || saved poses [3 nV] | weight, barc^2, r [nE] | the
// start's per-workgroup values | known mask [nE]
struct GncLayout {
  size_t o_mu, o_cost, o_part, rec_bytes, o_saved, o_w, o_c, o_r, o_wg, o_known, bytes;
  GncLayout(int max_outer, int nV, int nE) {
    BlobLayout B;
    B.add<GncState>(1);
    const size_t n = (size_t)max_outer + 1, e = (size_t)std::max(nE, 1);
    o_mu = B.add<double>(n); o_cost = B.add<double>(n); o_part = B.add<int32_t>(n);
    rec_bytes = B.off;
    o_saved = B.add<double>(3 * (size_t)std::max(nV, 1));
    o_w = B.add<double>(e); o_c = B.add<double>(e); o_r = B.add<double>(e); o_wg = B.add<double>((e + 255) / 256);
    o_known = B.add<uint8_t>(e);
    bytes = B.off + 256;
  }
};

// The third policy of tr_run.  A round: [the start: one chi-only pass for r, mu0;] up to outer_per_wait outer iterations.
struct GncPolicy {
  using State = GncState;
  static constexpr const char* kName = "graduated non-convexity";
  static constexpr bool kRunsEmpty = true;
  cgmr_gnc_params P;
  GncOut out;
  GncDev L;
  GncLayout lay;
  int ran = 0;                                               // outer iterations run (finish())

  // (gnc_run has reserved the arena -- the per-edge arrays went up before the driver started -- and bound L)
  int reserve(cgmr_ctx*, int, const GnSystem&, int, size_t* rec_bytes) { *rec_bytes = lay.rec_bytes; return 0; }
  GncState start(int) const {
    GncState hs;
    hs.factor = P.mu_factor; hs.loss = P.loss; hs.max_outer = P.max_outer; hs.inner_iters = P.inner_iters;
    return hs;
  }
  GnEdges edges(const GnEdges& Ed, int mode, double* r_out) const {
    GnEdges E = Ed;
    E.gnc = true; E.ga = {L.weight, L.barc_sq, L.known, L.S, r_out, mode};
    return E;
  }
  static void outer_records(hipStream_t st, const GnDevice& D, void* self) { launch_gnc_outer(st, D, ((GncPolicy*)self)->L); }
  // One outer iteration, the same launches whatever happens (gnc_kernels.hip).  With nothing to move a pass is its
  // linearisation alone.
  void outer(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, int nV, double* d_poses, const GnEdges& Ed) {
    for (int i = 0; i < P.inner_iters; i++) {
      const GnEdges E = edges(Ed, i == 0 ? kGncCompute : kGncReuse, nullptr);
      if (D.nf > 0) {
        GnPassOpts o;
        if (i == 0) { o.after_assemble = outer_records; o.after_assemble_arg = this; }
        gn_pass_on(ctx, D, st, d_poses, E, o);
      } else if (i == 0) {
        launch_linearize(st, D, d_poses, E, 1);
        launch_gnc_outer(st, D, L);
      }
      launch_gnc_step(st, D, L, i + 1 == P.inner_iters);
    }
    launch_tr_commit(st, nV, d_poses, L.saved, &L.S->accept);
  }
  void queue_round(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, const GnSystem& sys, const GnEdges& Ed, const GncState& hs, int) {
    if (hs.need_init) {
      launch_linearize(st, D, sys.d_poses, edges(Ed, kGncPlain, L.r), 1);
      launch_gnc_start(st, D, L);
    }
    const int n = std::min(P.outer_per_wait, P.max_outer - hs.iter);
    for (int t = 0; t < n; t++) outer(ctx, D, st, sys.nV, sys.d_poses, Ed);
  }
  GnCall::Readback also_read(const GnDevice&) { return {nullptr, nullptr, 0}; }
  void empty_system(GncState&, char*, double, int) const {}
  int finish(cgmr_ctx* ctx, const GncState& hs, const char* h, int ran_, int iters, int64_t waits) {
    ran = ran_;
    records_out(out.mu, (const double*)(h + lay.o_mu), ran, iters);
    records_out(out.partial, (const int32_t*)(h + lay.o_part), ran, iters);
    if (out.cost) for (int k = 0; k < ran; k++) out.cost[k] = ((const double*)(h + lay.o_cost))[k];   // (the rest: gnc_run)
    if (out.outer_done) *out.outer_done = ran;
    ctx->gnc_stats[0] = waits;
    ctx->gnc_stats[1] = hs.inner_total;
    if (hs.failed)
      return set_err(ctx, CGMR_E_CHOLESKY_BASE - (hs.failed - 1),
                     "graduated non-convexity: Cholesky failed (non-positive pivot) in inner iteration %d; poses left at the last good update",
                     hs.failed - 1);
    return CGMR_OK;
  }
};

bool gnc_params_ok(const cgmr_gnc_params* params) {
  if (!params) return true;
  const cgmr_gnc_params& P = *params;
  return (P.loss == CGMR_GNC_TLS || P.loss == CGMR_GNC_GM) && std::isfinite(P.mu_factor) && P.mu_factor > 1 && P.max_outer >= 1 &&
         P.inner_iters >= 1 && P.outer_per_wait >= 1 && std::isfinite(P.default_barc_sq);
}
double gnc_default_barc_sq(int dim) {
  const double quantile[4] = {0.0, 6.634896601021213, 9.21034037197618, 11.344866730144373};   // chi2 0.99, by dimension
  return quantile[dim < 1 ? 1 : dim > 3 ? 3 : dim];
}

// The driver of cgmr_gnc_optimize* and cgmr_graph_optimize_gnc: the arena, the per-edge arrays up, tr_run with GncPolicy, then
// the final statistics at the poses the call returns, with the weights of its last outer iteration.
int gnc_run(cgmr_ctx* ctx, const GnSystem& S, const GnEdges& Ed, const cgmr_gnc_params& P, const double* barc_sq,
            const uint8_t* known, const GncOut& out) {
  hipStream_t st = ctx->stream;
  GncPolicy pol{P, out, GncDev(), GncLayout(P.max_outer, S.nV, S.nE)};
  int r = arena_reserve(ctx, ctx->gnc_arena, pol.lay.bytes);
  if (r) return r;
  char* d = ctx->gnc_arena.ptr;
  GncDev& L = pol.L;
  L.S = (GncState*)d; L.rec_mu = (double*)(d + pol.lay.o_mu); L.rec_cost = (double*)(d + pol.lay.o_cost);
  L.rec_partial = (int32_t*)(d + pol.lay.o_part); L.saved = (double*)(d + pol.lay.o_saved); L.weight = (double*)(d + pol.lay.o_w);
  L.barc_sq = (double*)(d + pol.lay.o_c); L.r = (double*)(d + pol.lay.o_r); L.part = (double*)(d + pol.lay.o_wg);
  L.known = (uint8_t*)(d + pol.lay.o_known);
  if (S.nE > 0) {   // (pageable host memory: the copies have left the arrays when they return)
    HIP_TRY(ctx, hipMemcpyAsync(L.barc_sq, barc_sq, 8 * (size_t)S.nE, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(L.known, known, (size_t)S.nE, hipMemcpyHostToDevice, st));
  }
  r = tr_run(ctx, pol, S, Ed, P.max_outer);
  if (r != CGMR_OK && r > CGMR_E_CHOLESKY_BASE) return r;
  // the final statistics, at the poses the call returns and with the weights of its last outer iteration
  GnDevice& D = ctx->gn;
  double cost_end = 0.0;
  launch_linearize(st, D, S.d_poses, pol.edges(Ed, kGncReuse, L.r), 1);
  launch_chi2(st, D, D.chi2);
  HIP_TRY(ctx, hipMemcpyAsync(&cost_end, D.chi2, sizeof(double), hipMemcpyDeviceToHost, st));
  if (S.nE > 0 && out.weight) HIP_TRY(ctx, hipMemcpyAsync(out.weight, L.weight, 8 * (size_t)S.nE, hipMemcpyDeviceToHost, st));
  if (S.nE > 0 && out.edge_chi2) HIP_TRY(ctx, hipMemcpyAsync(out.edge_chi2, L.r, 8 * (size_t)S.nE, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (out.cost) for (int k = pol.ran; k <= P.max_outer; k++) out.cost[k] = cost_end;
  return r;
}

}  // namespace cgmr
