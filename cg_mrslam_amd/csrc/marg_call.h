// MargCall: what every driver of the marginals family does around its own launches (marginals_host.cpp, jcbb_host.cpp).
#pragma once
#include "host_call.h"

namespace cgmr {

// What a marginals entry point does around its own launches, whichever blocks of H^-1 it is after: the robust description, a
// private copy of the poses, the structure and the masks, the head of the staging block (poses | meas | info; the driver
// adds its own fields to L behind it), one pass that keeps the factor with what reads it, the statistics and the ending.
struct MargCall {
  cgmr_ctx* ctx;
  const HostCall& c;
  TypedHost typed;
  GnEdges Ed;
  std::vector<double> work;          // pushState: the caller's poses stay untouched
  Layout256 L;
  size_t o_p = 0, o_m = 0, o_i = 0;
  char* d = nullptr;                 // the staging block on the device and the poses in it, from stage() on
  double* dp = nullptr;
  bool factor = true;                // false: no free vertex, nothing to factor -- run() queues no pass, close() reads no statistics
  int status4[4] = {0, 0, 0, 0};

  // The opening every driver shares, in four steps -- args, types, open, structure -- with the driver's own checks between them
  // where they have always stood (which error wins, and which outputs are zeroed before a later step fails, stay as they were).
  MargCall(cgmr_ctx* x, const HostCall& call) : ctx(x), c(call) {}
  // the arguments every marginals entry point takes, with the driver's own null test; `who` heads the text
  int args(bool own_bad, const char* who) {
    if (!ctx) return CGMR_E_INVALID;
    if (c.nV <= 0 || c.nE < 0 || own_bad || !c.poses || (c.nE > 0 && (!c.ef || !c.et || !c.meas || !c.info)))
      return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", who);
    return 0;
  }
  // the factor types, checked on the host
  int types(const char* who) { return typed_check(ctx, who, c, typed); }
  // [the factor types under `who_typed`,] the private copy of the poses; robust kernels: rho1 at the pass's linearisation point
  int open(const char* who, const char* who_typed = nullptr) {
    if (const int rc = who_typed ? types(who_typed) : 0) return rc;
    work.assign(c.poses, c.poses + 3 * (size_t)c.nV);
    o_p = L.add(24 * (size_t)c.nV); o_m = L.add(24 * (size_t)c.nE); o_i = L.add(48 * (size_t)c.nE);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = robust_setup(ctx, c.rk, c.nE, false, Ed, who);
    return rc ? rc : typed_upload(ctx, &typed, Ed);
  }
  int structure(const uint8_t* fixed) {
    const int rc = prepare_structure(ctx, c.nV, c.nE, c.ef, c.et, 1);
    return rc ? rc : prepare_pass(ctx, fixed, c.nE, c.ef, c.et, c.nE);
  }
  // the staging block as L describes it by now; the head goes up
  int stage() {
    const int rc = arena_reserve(ctx, ctx->io_arena, L.off + 256);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    d = ctx->io_arena.ptr;
    dp = (double*)(d + o_p);
    HIP_TRY(ctx, hipMemcpyAsync(dp, work.data(), 24 * (size_t)c.nV, hipMemcpyHostToDevice, st));
    if (c.nE > 0) {
      HIP_TRY(ctx, hipMemcpyAsync(d + o_m, c.meas, 24 * (size_t)c.nE, hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(d + o_i, c.info, 48 * (size_t)c.nE, hipMemcpyHostToDevice, st));
    }
    Ed.meas_a = (const double*)(d + o_m); Ed.info_a = (const double*)(d + o_i); Ed.nA = c.nE; Ed.n_active = c.nE;
    return 0;
  }
  // gn_pass(.., write_l11c) at dp, then queue(): the driver's launches that read the factor and its result copies; the status
  // words come back with them.
  template <typename Queue>
  int run(GnPassOpts pass, Queue&& queue) {
    GnDevice& D = ctx->gn;
    hipStream_t st = ctx->stream;
    pass.write_l11c = true;
    auto once = [&]() -> int {
      if (factor) gn_pass(ctx, dp, Ed, pass);
      const int rc = queue();
      if (rc) return rc;
      if (factor) HIP_TRY(ctx, hipMemcpyAsync(status4, D.status, sizeof status4, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
      HIP_TRY(ctx, hipGetLastError());
      return 0;
    };
    int rc = once();
    if (rc || status4[2] == 0) return rc;
    // A bounded wait ran out (status[2]): a hand-off between workgroups of a merged level launch (the forward pass: factor
    // work items -> update tiles) or of the chained backward solve that never arrived -- not a numerical failure.  As gn_run
    // does, the pass is repeated from the same poses with one launch per kernel and level (no in-kernel waits).  The cached
    // structure keeps only the forward merges that are certainly resident from now on; the chained backward solve (mode 2)
    // stays, as in gn_run: its waits are bounded as well, and a later time-out there falls back the same way.
    choose_fwd_merge(D, ctx->side_used ? 2 : 1, false, false);
    LevelwiseScope levelwise(ctx, D);                             // (ends with those merges and the chained solve back)
    rc = levelwise.arm(st);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(dp, work.data(), 24 * (size_t)c.nV, hipMemcpyHostToDevice, st));
    rc = once();
    if (rc) return rc;
    if (status4[2] != 0)
      return set_err(ctx, CGMR_E_TIMEOUT, "marginals: a bounded device-side wait (forward hand-off or chained backward solve) ran out twice");
    return 0;
  }
  // the statistics (also after a failed Cholesky: e2 / rho1 of that H), then the factorisation's verdict
  int close() {
    const int rc = factor ? robust_stats_out(ctx, c.rk, c.nE, Ed) : 0;
    if (rc) return rc;
    if (status4[0] != 0) return set_err(ctx, CGMR_E_CHOLESKY_BASE, "Cholesky failed while computing marginals");
    return 0;
  }
};

}  // namespace cgmr
