// C ABI of libcgmr.so (include/cgmr.h): context management, and the solver's entry points -- what each was given is checked and
// staged here, then handed to the drivers (gn_host.cpp, optimize_host.cpp, marginals_host.cpp).  Compiled with hipcc; contains no kernels.
#include "factor_model.h"
#include "host_call.h"

#include <algorithm>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>

namespace cgmr {

// The robust description of an entry point (include/cgmr.h: cgmr_robust) into Ed, checked before anything is queued.  The host
// entry points' kind / delta arrays are staged through rk_arena; the device ones are read back once to be checked.  The
// statistics (2 nE doubles: e2, then rho1) land in rk_arena behind them.  rk == nullptr: nothing (the plain call).
int robust_setup(cgmr_ctx* ctx, const cgmr_robust* rk, int nE, bool dev, GnEdges& Ed, const char* who) {
  if (!rk) return 0;
  const size_t n = (size_t)std::max(nE, 0);
  std::vector<uint8_t> hk;
  std::vector<double> hd;
  const uint8_t* ck = rk->kind;
  const double* cd = rk->delta;
  if (dev && n > 0 && (rk->kind || rk->delta)) {
    if (rk->kind) { hk.resize(n); HIP_TRY(ctx, hipMemcpyAsync(hk.data(), rk->kind, n, hipMemcpyDeviceToHost, ctx->stream)); ck = hk.data(); }
    if (rk->delta) { hd.resize(n); HIP_TRY(ctx, hipMemcpyAsync(hd.data(), rk->delta, 8 * n, hipMemcpyDeviceToHost, ctx->stream)); cd = hd.data(); }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  bool ok = rk->default_kind >= CGMR_RK_NONE && rk->default_kind <= CGMR_RK_DCS;
  if (ok && !rk->kind && !rk->delta) ok = robust_valid(rk->default_kind, rk->default_delta);
  for (size_t k = 0; ok && k < n && (ck || cd); k++)
    ok = robust_valid(ck ? ck[k] : rk->default_kind, cd ? cd[k] : rk->default_delta);
  if (!ok)
    return set_err(ctx, CGMR_E_INVALID, "%s: a robust kernel kind must be 0..7, its delta finite and > 0 (kind 0 excepted)", who);
  const bool stats = n > 0 && (rk->edge_chi2_out || rk->weight_out);
  const size_t ok_ = 0, od = (n + 255) & ~size_t(255), os = od + ((8 * n + 255) & ~size_t(255));
  if (stats || (!dev && (rk->kind || rk->delta))) {
    int rc = arena_reserve(ctx, ctx->rk_arena, os + 16 * n + 256);
    if (rc) return rc;
  }
  char* d = ctx->rk_arena.ptr;
  Ed.robust = true;
  Ed.rk.kind0 = rk->default_kind; Ed.rk.delta0 = rk->default_delta;
  if (dev) { Ed.rk.kind = rk->kind; Ed.rk.delta = rk->delta; }
  else {
    if (rk->kind && n > 0) { HIP_TRY(ctx, hipMemcpyAsync(d + ok_, rk->kind, n, hipMemcpyHostToDevice, ctx->stream)); Ed.rk.kind = (const uint8_t*)(d + ok_); }
    if (rk->delta && n > 0) { HIP_TRY(ctx, hipMemcpyAsync(d + od, rk->delta, 8 * n, hipMemcpyHostToDevice, ctx->stream)); Ed.rk.delta = (const double*)(d + od); }
  }
  Ed.rk.stats = stats ? (double*)(d + os) : nullptr;
  return 0;
}

// the statistics of the call's final pass to the caller's host arrays
int robust_stats_out(cgmr_ctx* ctx, const cgmr_robust* rk, int nE, const GnEdges& Ed) {
  if (!rk || !Ed.rk.stats) return 0;
  if (rk->edge_chi2_out) HIP_TRY(ctx, hipMemcpyAsync(rk->edge_chi2_out, Ed.rk.stats, 8 * (size_t)nE, hipMemcpyDeviceToHost, ctx->stream));
  if (rk->weight_out) HIP_TRY(ctx, hipMemcpyAsync(rk->weight_out, Ed.rk.stats + nE, 8 * (size_t)nE, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// The factor types of a typed entry point, checked on the host before the device is touched (host_call.h: TypedHost)
int typed_check(cgmr_ctx* ctx, const char* who, const HostCall& c, TypedHost& T) {
  if (!c.ft) return 0;                                          // (the plain call: nothing is built)
  T.vk.assign((size_t)std::max(c.nV, 0), 0);
  T.ek.assign((size_t)std::max(c.nE, 0), 0);
  if (c.ft->vertex_kind) T.vk.assign(c.ft->vertex_kind, c.ft->vertex_kind + c.nV);
  if (c.ft->edge_kind) T.ek.assign(c.ft->edge_kind, c.ft->edge_kind + c.nE);
  for (int v = 0; v < c.nV; v++)
    if (T.vk[v] > 1) return set_err(ctx, CGMR_E_INVALID, "%s: vertex %d has kind %d (0 = SE2 pose, 1 = point)", who, v, (int)T.vk[v]);
  std::vector<int32_t> cnt((size_t)std::max(c.nV, 0) + 1, 0);
  int n_prior = 0;
  for (int k = 0; k < c.nE; k++) {
    const int kind = T.ek[k], a = c.ef[k], b = c.et[k];
    if (a < 0 || a >= c.nV || b < 0 || b >= c.nV) return set_err(ctx, CGMR_E_INVALID, "%s: edge %d has a vertex index out of range", who, k);
    if (kind > CGMR_EDGE_PRIOR_SE2_XY) return set_err(ctx, CGMR_E_INVALID, "%s: edge %d has unknown kind %d", who, k, kind);
    if (kind == CGMR_EDGE_SE2_XY || kind == CGMR_EDGE_BEARING_SE2_XY) {
      if (T.vk[a] != 0 || T.vk[b] != 1)
        return set_err(ctx, CGMR_E_INVALID, "%s: edge %d (%s) must go from a pose to a point", who, k, kind == CGMR_EDGE_SE2_XY ? "EDGE_SE2_XY" : "EDGE_BEARING_SE2_XY");
    } else {
      if (T.vk[a] != 0 || T.vk[b] != 0)
        return set_err(ctx, CGMR_E_INVALID, "%s: edge %d (kind %d) touches a point; only EDGE_SE2_XY and EDGE_BEARING_SE2_XY may", who, k, kind);
      if (factor_is_prior(kind)) {
        if (a != b) return set_err(ctx, CGMR_E_INVALID, "%s: edge %d is a prior (kind %d) and must have from == to", who, k, kind);
        cnt[a + 1]++;
        n_prior++;
      }
    }
    if (kind) T.any = true;
  }
  if (!T.any) return 0;
  // CSR of the priors by vertex: vertices ascending, a vertex's edges ascending
  std::vector<int32_t> slot((size_t)c.nV, -1);
  for (int v = 0; v < c.nV; v++)
    if (cnt[v + 1]) { slot[v] = (int32_t)T.uv_vertex.size(); T.uv_vertex.push_back(v); T.uv_ptr.push_back(0); }
  T.uv_ptr.push_back(0);
  for (size_t u = 0; u < T.uv_vertex.size(); u++) T.uv_ptr[u + 1] = T.uv_ptr[u] + cnt[T.uv_vertex[u] + 1];
  T.uv_edge.assign((size_t)n_prior, 0);
  std::vector<int32_t> cur(T.uv_ptr.begin(), T.uv_ptr.end());
  for (int k = 0; k < c.nE; k++) if (factor_is_prior(T.ek[k])) T.uv_edge[cur[slot[c.ef[k]]]++] = k;
  return 0;
}
// ... staged through ty_arena into Ed (nothing when every kind is zero)
int typed_upload(cgmr_ctx* ctx, const TypedHost* T, GnEdges& Ed) {
  if (!T || !T->any) return 0;
  Layout256 L;
  const size_t nU = T->uv_vertex.size();
  const size_t o_ek = L.add(T->ek.size()), o_uv = L.add(4 * std::max<size_t>(nU, 1)), o_up = L.add(4 * (nU + 1)),
               o_ue = L.add(4 * std::max<size_t>(T->uv_edge.size(), 1));
  int rc = arena_reserve(ctx, ctx->ty_arena, L.off + 256);
  if (rc) return rc;
  char* d = ctx->ty_arena.ptr;
  hipStream_t st = ctx->stream;
  // (pageable host memory: the copies have left the vectors when they return)
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ek, T->ek.data(), T->ek.size(), hipMemcpyHostToDevice, st));
  if (nU > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(d + o_uv, T->uv_vertex.data(), 4 * nU, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d + o_up, T->uv_ptr.data(), 4 * (nU + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d + o_ue, T->uv_edge.data(), 4 * T->uv_edge.size(), hipMemcpyHostToDevice, st));
  }
  Ed.typed = true;
  Ed.ty.edge_kind = (const uint8_t*)(d + o_ek);
  Ed.unary = {(int)nU, (const int32_t*)(d + o_uv), (const int32_t*)(d + o_up), (const int32_t*)(d + o_ue)};
  return 0;
}

// The mixture of a mixture entry point (include/cgmr.h: cgmr_mixture), checked on the host before the device is touched.  `any`:
// some edge has more than one component (none: the call is the typed / plain one on meas / info, bit for bit).  off: per
// component c = max_j a_j - a, a = 2 ln w + ln det Omega over the factor's own dimension, in double on the host; 0 on an edge
// of one component, whose weight and Omega are not looked at.
struct MixHost {
  bool any = false;
  const cgmr_mixture* mix = nullptr;
  size_t nC = 0;
  std::vector<double> off;
};
static int mix_check(cgmr_ctx* ctx, const char* who, const cgmr_mixture* mix, int nE, const TypedHost& typed, MixHost& M) {
  if (!mix || !mix->comp_ptr) return 0;
  const int32_t* cp = mix->comp_ptr;
  if (cp[0] != 0) return set_err(ctx, CGMR_E_INVALID, "%s: comp_ptr[0] must be 0 (edge 0)", who);
  for (int k = 0; k < nE; k++) {
    if (cp[k + 1] <= cp[k])
      return set_err(ctx, CGMR_E_INVALID, "%s: edge %d has no component (comp_ptr must increase from 0)", who, k);
    if (cp[k + 1] - cp[k] > 1) M.any = true;
  }
  if (!M.any) return 0;
  if (!mix->comp_meas || !mix->comp_info || !mix->comp_weight)
    return set_err(ctx, CGMR_E_INVALID, "%s: a mixture needs comp_meas, comp_info and comp_weight", who);
  M.mix = mix;
  M.nC = (size_t)cp[nE];
  M.off.assign(M.nC, 0.0);
  for (int k = 0; k < nE; k++) {
    const int p0 = cp[k], p1 = cp[k + 1];
    if (p1 - p0 < 2) continue;
    const int dim = factor_dim(typed.any ? typed.ek[k] : CGMR_EDGE_SE2);
    double amax = 0;
    for (int p = p0; p < p1; p++) {
      const double w = mix->comp_weight[p];
      const double* u = mix->comp_info + 6 * (size_t)p;
      const double det = dim == 1 ? u[0]
                         : dim == 2
                             ? u[0] * u[3] - u[1] * u[1]
                             : u[0] * (u[3] * u[5] - u[4] * u[4]) - u[1] * (u[1] * u[5] - u[4] * u[2]) + u[2] * (u[1] * u[4] - u[3] * u[2]);
      if (!(std::isfinite(w) && w > 0))
        return set_err(ctx, CGMR_E_INVALID, "%s: edge %d, component %d: the weight must be finite and > 0", who, k, p - p0);
      if (!(std::isfinite(det) && det > 0))
        return set_err(ctx, CGMR_E_INVALID, "%s: edge %d, component %d: det Omega (the factor's own dimension) must be finite and > 0", who, k, p - p0);
      const double a = 2 * std::log(w) + std::log(det);
      M.off[p] = a;
      if (p == p0 || a > amax) amax = a;
    }
    for (int p = p0; p < p1; p++) M.off[p] = amax - M.off[p];
  }
  return 0;
}
// ... staged through mix_arena into Ed (nothing without a multi-component edge); the selection lands behind the lists
static int mix_upload(cgmr_ctx* ctx, const MixHost* M, int nE, GnEdges& Ed) {
  if (!M || !M->any) return 0;
  Layout256 L;
  const size_t nC = M->nC, n = (size_t)nE;
  const size_t o_ptr = L.add(4 * (n + 1)), o_meas = L.add(24 * nC), o_info = L.add(48 * nC), o_off = L.add(8 * nC), o_sel = L.add(4 * n);
  int rc = arena_reserve(ctx, ctx->mix_arena, L.off + 256);
  if (rc) return rc;
  char* d = ctx->mix_arena.ptr;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ptr, M->mix->comp_ptr, 4 * (n + 1), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_meas, M->mix->comp_meas, 24 * nC, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_info, M->mix->comp_info, 48 * nC, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_off, M->off.data(), 8 * nC, hipMemcpyHostToDevice, st));
  Ed.mix = true;
  Ed.mx.cptr = (const int32_t*)(d + o_ptr);
  Ed.mx.cmeas = (const double*)(d + o_meas); Ed.mx.cinfo = (const double*)(d + o_info); Ed.mx.coff = (const double*)(d + o_off);
  Ed.mx.sel_out = M->mix->selected_out ? (int32_t*)(d + o_sel) : nullptr;
  return 0;
}
// every edge's first component: what a call routed to the typed / plain path, or one that fails, leaves in selected_out
static void mix_selection_zero(const cgmr_mixture* mix, int nE) {
  if (mix && mix->selected_out) for (int k = 0; k < nE; k++) mix->selected_out[k] = 0;
}
// the selection of the call's final pass to the caller's host array
static int mix_selection_out(cgmr_ctx* ctx, const MixHost* M, int nE, const GnEdges& Ed) {
  if (!M || !Ed.mx.sel_out || nE <= 0) return 0;
  HIP_TRY(ctx, hipMemcpyAsync(M->mix->selected_out, Ed.mx.sel_out, 4 * (size_t)nE, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// What every optimiser entry point does before it stages: the arguments every one of them takes, checked alike, the verdict of
// its own parameter check (own_error: null, or the text with %s for who_args), the factor types (F.typed), the mixture (F.mix,
// selected_out zeroed), and a verdict that has always come last (late_error: dogleg's parameters).
struct OptimizeFront { TypedHost typed; MixHost mix; };
static int optimize_front(cgmr_ctx* ctx, const HostCall& c, int iters, const char* who_args, const char* own_error, const char* who_typed,
                          const char* who_mix, const char* late_error, OptimizeFront& F) {
  if (!ctx) return CGMR_E_INVALID;
  if (c.nV < 0 || c.nE < 0 || iters < 0 || (c.nV > 0 && (!c.poses || !c.fixed)) || (c.nE > 0 && (!c.ef || !c.et || !c.meas || !c.info)))
    return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", who_args);
  if (own_error) return set_err(ctx, CGMR_E_INVALID, own_error, who_args);
  int rc = typed_check(ctx, who_typed, c, F.typed);
  if (rc) return rc;
  rc = mix_check(ctx, who_mix, c.mix, c.nE, F.typed, F.mix);
  if (rc) return rc;
  mix_selection_zero(c.mix, c.nE);
  return late_error ? set_err(ctx, CGMR_E_INVALID, "%s", late_error) : 0;
}

// Around run(S, Ed) -- a *_run on device arrays --: the robust description, and unless c.dev (poses, meas and info are the
// device's already) the host arrays staged through io_arena and the poses read back.  The poses and the robust statistics are
// returned when the call ended well, and with cholesky_too also on a Cholesky status.
template <typename Run>
static int optimize_staged(cgmr_ctx* ctx, const char* who, bool cholesky_too, const HostCall& c, const OptimizeFront& F, Run&& run) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  GnEdges Ed;
  int rc = robust_setup(ctx, c.rk, c.nE, c.dev, Ed, who);
  if (rc) return rc;
  rc = typed_upload(ctx, &F.typed, Ed);
  if (rc) return rc;
  rc = mix_upload(ctx, &F.mix, c.nE, Ed);
  if (rc) return rc;
  double* d_poses = c.poses;
  const size_t bp = sizeof(double) * 3 * (size_t)c.nV;
  if (c.dev) {
    Ed.meas_a = c.meas; Ed.info_a = c.info;
  } else {
    const size_t bm = sizeof(double) * 3 * (size_t)c.nE, bi = sizeof(double) * 6 * (size_t)c.nE, om = (bp + 255) & ~size_t(255), oi = (om + bm + 255) & ~size_t(255);
    rc = arena_reserve(ctx, ctx->io_arena, oi + bi + 256);
    if (rc) return rc;
    char* d = ctx->io_arena.ptr;
    HIP_TRY(ctx, hipMemcpyAsync(d, c.poses, bp, hipMemcpyHostToDevice, ctx->stream));
    if (Ed.mix) {                        // (a mixture pass reads the component lists alone: the first components stay on the host)
      Ed.meas_a = Ed.mx.cmeas; Ed.info_a = Ed.mx.cinfo;
    } else {
      HIP_TRY(ctx, hipMemcpyAsync(d + om, c.meas, bm, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(d + oi, c.info, bi, hipMemcpyHostToDevice, ctx->stream));
      Ed.meas_a = (const double*)(d + om); Ed.info_a = (const double*)(d + oi);
    }
    d_poses = (double*)d;
  }
  Ed.nA = c.nE; Ed.n_active = c.nE;
  rc = run(GnSystem{c.nV, d_poses, c.fixed, c.nE, c.ef, c.et}, Ed);
  if (rc == CGMR_OK || (cholesky_too && rc <= CGMR_E_CHOLESKY_BASE)) {
    if (!c.dev) {
      hipError_t e = hipMemcpyAsync(c.poses, d_poses, bp, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) return set_err(ctx, CGMR_E_HIP, "pose read-back: %s", hipGetErrorString(e));
    }
    const int rs = robust_stats_out(ctx, c.rk, c.nE, Ed);
    if (rs) return rs;
    const int ms = mix_selection_out(ctx, &F.mix, c.nE, Ed);
    if (ms) return ms;
  }
  return rc;
}

// Gauss-Newton, Levenberg-Marquardt and dogleg entry points, whatever their variant.  The names in the texts are the ones they
// have always had: the factor types report as family + "_mixture" / "_typed_dev" / "_typed", the mixture as family + "_mixture",
// optimize_staged's own errors as family + "_typed" for a typed call, else + plain / plain_dev.
template <typename Run>
static int optimize_impl(cgmr_ctx* ctx, const char* family, const char* plain, const char* plain_dev, bool cholesky_too, const HostCall& c,
                         int iters, const char* late_error, Run&& run) {
  char who_typed[64], who_mix[64], who[64];
  snprintf(who_typed, sizeof who_typed, "%s%s", family, c.mix ? "_mixture" : c.dev ? "_typed_dev" : "_typed");
  snprintf(who_mix, sizeof who_mix, "%s_mixture", family);
  snprintf(who, sizeof who, "%s%s", family, c.ft ? "_typed" : c.dev ? plain_dev : plain);
  OptimizeFront F;
  const int rc = optimize_front(ctx, c, iters, family, nullptr, who_typed, who_mix, late_error, F);
  return rc ? rc : optimize_staged(ctx, who, cholesky_too, c, F, run);
}
static int gn_optimize_impl(cgmr_ctx* ctx, const HostCall& c, int iters, double* chi2_out) {
  return optimize_impl(ctx, "cgmr_gn_optimize", "_robust", "_robust_dev", true, c, iters, nullptr,
                       [&](const GnSystem& S, const GnEdges& Ed) { return gn_run(ctx, S, Ed, iters, chi2_out); });
}
static int lm_optimize_impl(cgmr_ctx* ctx, const HostCall& c, int iters, const cgmr_lm_params* params, const LmOut& out) {
  return optimize_impl(ctx, "cgmr_lm_optimize", "_robust", "_robust_dev", false, c, iters, nullptr,
                       [&](const GnSystem& S, const GnEdges& Ed) { return lm_run(ctx, S, Ed, iters, params, out); });
}
static int dl_optimize_impl(cgmr_ctx* ctx, const HostCall& c, int iters, const cgmr_dl_params* params, const DlOut& out) {
  return optimize_impl(ctx, "cgmr_dl_optimize", "", "_dev", true, c, iters,
                       dl_params_ok(params) ? nullptr : "cgmr_dl_optimize: max_trials must be >= 1, initial_delta / initial_lambda > 0, lambda_factor > 1, all finite",
                       [&](const GnSystem& S, const GnEdges& Ed) { return dl_run(ctx, S, Ed, iters, params, out); });
}

// cgmr_gnc_optimize*: the front with the parameters' check, the per-edge thresholds and known flags, then gnc_run
static int gnc_optimize_impl(cgmr_ctx* ctx, const HostCall& c, const cgmr_gnc_params* params, double* mu_out, double* cost_out,
                             int32_t* partial_out, int32_t* outer_done) {
  const char* who = c.dev ? "cgmr_gnc_optimize_dev" : "cgmr_gnc_optimize";
  const cgmr_gnc_params P = params ? *params : gnc_params_default();
  OptimizeFront F;
  int rc = optimize_front(ctx, c, 0, who, gnc_params_ok(&P) ? nullptr : "%s: loss must be CGMR_GNC_TLS or CGMR_GNC_GM, mu_factor finite and > 1, max_outer / inner_iters / outer_per_wait >= 1, default_barc_sq finite",
                          who, who, nullptr, F);
  if (rc) return rc;
  std::vector<double> hc((size_t)c.nE);
  std::vector<uint8_t> hk((size_t)c.nE, 0);
  for (int k = 0; k < c.nE; k++) {
    hc[k] = P.barc_sq ? P.barc_sq[k] : P.default_barc_sq > 0 ? P.default_barc_sq : gnc_default_barc_sq(factor_dim(F.typed.any ? F.typed.ek[k] : CGMR_EDGE_SE2));
    if (!std::isfinite(hc[k]) || !(hc[k] > 0)) return set_err(ctx, CGMR_E_INVALID, "%s: barc_sq of edge %d must be finite and > 0", who, k);
    if (P.known_inlier) hk[k] = P.known_inlier[k] ? 1 : 0;
  }
  return optimize_staged(ctx, who, true, c, F, [&](const GnSystem& S, const GnEdges& Ed) {
    return gnc_run(ctx, S, Ed, P, hc.data(), hk.data(), {mu_out, cost_out, partial_out, outer_done, P.weight_out, P.edge_chi2_out});
  });
}

// cgmr_chordal_initialize*: the front with the stages' check, then which vertices each stage's terms touch -- a term whose
// information entries for the stage are all zero touches nothing -- from the host's copy of the information (a _dev call reads
// it back once)
static int chordal_impl(cgmr_ctx* ctx, const HostCall& c, int stages, double* chi2_out, int32_t* counts_out) {
  const char* who = c.ft ? (c.dev ? "cgmr_chordal_initialize_typed_dev" : "cgmr_chordal_initialize_typed")
                         : (c.dev ? "cgmr_chordal_initialize_dev" : "cgmr_chordal_initialize");
  OptimizeFront F;
  int rc = optimize_front(ctx, c, 0, who, stages < 1 || stages > 3 ? "%s: stages must be 1 (rotation), 2 (translation) or 3 (both)" : nullptr, who, who, nullptr, F);
  if (rc) return rc;
  for (int k = 0; k < c.nE; k++)
    if (c.ef[k] < 0 || c.ef[k] >= c.nV || c.et[k] < 0 || c.et[k] >= c.nV)
      return set_err(ctx, CGMR_E_INVALID, "%s: edge %d has a vertex index out of range", who, k);
  std::vector<double> hinfo;
  const double* hi = c.info;
  if (c.dev && c.nE > 0) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hinfo.resize(6 * (size_t)c.nE);
    HIP_TRY(ctx, hipMemcpyAsync(hinfo.data(), c.info, 48 * (size_t)c.nE, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    hi = hinfo.data();
  }
  std::vector<uint8_t> in_rot((size_t)c.nV, 0), in_tr((size_t)c.nV, 0);
  for (int k = 0; k < c.nE; k++) {
    const int dim = factor_dim(F.typed.any ? F.typed.ek[k] : CGMR_EDGE_SE2);      // 3: a heading term; 2 and 3: a position term
    const double* u = hi + 6 * (size_t)k;
    if (dim == 3 && u[5] != 0.0) in_rot[c.ef[k]] = in_rot[c.et[k]] = 1;
    if (dim >= 2 && (u[0] != 0.0 || u[1] != 0.0 || u[3] != 0.0)) in_tr[c.ef[k]] = in_tr[c.et[k]] = 1;
  }
  return optimize_staged(ctx, who, true, c, F, [&](const GnSystem& S, const GnEdges& Ed) {
    return chordal_run(ctx, S, Ed, stages, in_rot.data(), in_tr.data(), chi2_out, counts_out);
  });
}

}  // namespace cgmr

using namespace cgmr;

extern "C" {

int cgmr_version(void) { return 105; }   // 105: cgmr_*_optimize_robust*, cgmr_graph_set_edge_robust / _set_received_robust / _edge_stats added, later (same number: callers find them by their symbols) cgmr_marginals_robust, cgmr_marginals_all_robust, cgmr_covariance_estimate_robust, cgmr_condense_robust, cgmr_graph_set_condensed_robust, cgmr_dl_optimize*, cgmr_dl_last_stats, cgmr_graph_set_dogleg_params, cgmr_graph_dl_last (CGMR_ALG_DOGLEG), cgmr_marginals_joint, cgmr_marginals_pairs, cgmr_relative_covariance, cgmr_*_optimize_typed*, cgmr_marginals_typed, cgmr_marginals_all_typed, cgmr_marginals_joint_typed, cgmr_marginals_pairs_typed, cgmr_observation_covariance (and edge kind 2, CGMR_EDGE_BEARING_SE2_XY), cgmr_gnc_optimize*, cgmr_gnc_last_stats, cgmr_graph_set_edge_gnc / _set_received_gnc / _optimize_gnc / _gnc_weights / _keep_gnc_weights / _set_condensed_gnc; 104: cgmr_lm_optimize*, cgmr_lm_last_stats, cgmr_graph_set_algorithm / _lm_last added; 103: cgmr_marginals_all added; 102 (round 5): cgmr_match_last_redo_pairs / _path_counts, cgmr_graph_failed_batches, cgmr_comm_info added; nothing changed or removed

int cgmr_ctx_create(int device, void* hip_stream, cgmr_ctx** out) {
  if (!out) return CGMR_E_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return CGMR_E_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return CGMR_E_NO_DEVICE;
  cgmr_ctx* ctx = new cgmr_ctx();
  ctx->device = device;
  ctx->sw = read_switches();
  ctx->gn.sw = &ctx->sw;
  ctx->fwd_merge_any = ctx->sw.fwd_merge_any;
  if (hip_stream) { ctx->stream = (hipStream_t)hip_stream; ctx->own_stream = false; }
  else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return CGMR_E_HIP; }
    ctx->own_stream = true;
  }
  if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
      hipEventCreate(&ctx->ev_a) != hipSuccess || hipEventCreate(&ctx->ev_b) != hipSuccess) {
    cgmr_ctx_destroy(ctx);
    return CGMR_E_HIP;
  }
  *out = ctx;
  return CGMR_OK;
}

void cgmr_ctx_destroy(cgmr_ctx* ctx) {
  if (!ctx) return;
  // teardown: nothing useful can be done with a failing free, the statuses are dropped on purpose -- and a HIP runtime that
  // is already shutting down (a binding's garbage collector at interpreter exit) throws instead of returning an error
  try {
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->trace_n > 0)
    fprintf(stderr, "[gn] %lld solves: analysis + upload %.3f ms, masks %.3f ms, queueing the launches %.3f ms, waiting %.3f ms per solve\n", (long long)ctx->trace_n,
            1e3 * ctx->trace_sum[0] / ctx->trace_n, 1e3 * ctx->trace_sum[1] / ctx->trace_n, 1e3 * ctx->trace_sum[2] / ctx->trace_n, 1e3 * ctx->trace_sum[3] / ctx->trace_n);
  for (auto& q : ctx->graveyard) (void)hipFree(q.first);
  for (Arena* a : {&ctx->gn_arena, &ctx->io_arena, &ctx->mt_arena, &ctx->mtab_arena, &ctx->rep_arena, &ctx->mg_arena, &ctx->si_arena, &ctx->lm_arena,
                   &ctx->dl_arena, &ctx->gnc_arena, &ctx->rk_arena, &ctx->ty_arena, &ctx->mix_arena, &ctx->st_arena})
    if (a->ptr) (void)hipFree(a->ptr);
  if (ctx->pinned_st) (void)hipHostFree(ctx->pinned_st);
  if (ctx->ev_st_copied) (void)hipEventDestroy(ctx->ev_st_copied);
  if (ctx->side) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamDestroy(ctx->side); }
  for (hipEvent_t e : {ctx->side_fork, ctx->side_tail}) if (e) (void)hipEventDestroy(e);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->pinned_mask) (void)hipHostFree(ctx->pinned_mask);
  for (hipEvent_t e : {ctx->ev0, ctx->ev1, ctx->ev_a, ctx->ev_b})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  } catch (...) {
  }
  delete ctx;
}

const char* cgmr_last_error(const cgmr_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void* cgmr_ctx_stream(const cgmr_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int cgmr_ctx_synchronize(cgmr_ctx* ctx) {
  if (!ctx) return CGMR_E_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CGMR_OK;
}

int cgmr_gn_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE,
                         const int32_t* from_idx, const int32_t* to_idx, const double* d_meas,
                         const double* d_info, int iters, double* chi2_out) {
  return gn_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true}), iters, chi2_out);
}
int cgmr_gn_optimize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                     const int32_t* to_idx, const double* meas, const double* info, int iters, double* chi2_out) {
  return gn_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info), iters, chi2_out);
}

int cgmr_lm_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                         const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, const cgmr_lm_params* params,
                         double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done) {
  return lm_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true}), iters, params,
      {chi2_out, lambda_out, trials_out, iters_done});
}
int cgmr_lm_optimize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                     const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_lm_params* params,
                     double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done) {
  return lm_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info), iters, params, {chi2_out, lambda_out, trials_out, iters_done});
}

int cgmr_gn_optimize_robust(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas, const double* info, int iters, double* chi2_out,
                            const cgmr_robust* rk) {
  return gn_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, rk}), iters, chi2_out);
}
int cgmr_gn_optimize_robust_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, double* chi2_out,
                                const cgmr_robust* rk) {
  return gn_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, rk}), iters, chi2_out);
}

int cgmr_lm_optimize_robust(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_lm_params* params,
                            double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done, const cgmr_robust* rk) {
  return lm_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, rk}), iters, params,
      {chi2_out, lambda_out, trials_out, iters_done});
}
int cgmr_lm_optimize_robust_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                                const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                                int32_t* iters_done, const cgmr_robust* rk) {
  return lm_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, rk}), iters, params,
      {chi2_out, lambda_out, trials_out, iters_done});
}

int cgmr_lm_last_stats(const cgmr_ctx* ctx, int64_t out[2]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  out[0] = ctx->lm_stats[0];
  out[1] = ctx->lm_stats[1];
  return CGMR_OK;
}

int cgmr_dl_optimize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                     const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_dl_params* params,
                     double* chi2_out, double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                     const cgmr_robust* rk) {
  return dl_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, rk}), iters, params,
      {chi2_out, delta_out, trials_out, step_out, iters_done});
}
int cgmr_dl_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                         const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, const cgmr_dl_params* params,
                         double* chi2_out, double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                         const cgmr_robust* rk) {
  return dl_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, rk}), iters, params,
      {chi2_out, delta_out, trials_out, step_out, iters_done});
}

int cgmr_gn_optimize_typed(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                           const int32_t* to_idx, const double* meas, const double* info, int iters, double* chi2_out,
                           const cgmr_factor_types* types, const cgmr_robust* rk) {
  return gn_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, rk, types}), iters, chi2_out);
}
int cgmr_gn_optimize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                               const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, double* chi2_out,
                               const cgmr_factor_types* types, const cgmr_robust* rk) {
  return gn_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, rk, types}), iters, chi2_out);
}

int cgmr_lm_optimize_typed(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                           const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_lm_params* params,
                           double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done,
                           const cgmr_factor_types* types, const cgmr_robust* rk) {
  return lm_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, rk, types}), iters, params,
      {chi2_out, lambda_out, trials_out, iters_done});
}
int cgmr_lm_optimize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                               const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                               const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                               int32_t* iters_done, const cgmr_factor_types* types, const cgmr_robust* rk) {
  return lm_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, rk, types}), iters, params,
      {chi2_out, lambda_out, trials_out, iters_done});
}

int cgmr_dl_optimize_typed(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                           const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_dl_params* params,
                           double* chi2_out, double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                           const cgmr_factor_types* types, const cgmr_robust* rk) {
  return dl_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, rk, types}), iters, params,
      {chi2_out, delta_out, trials_out, step_out, iters_done});
}
int cgmr_dl_optimize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                               const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                               const cgmr_dl_params* params, double* chi2_out, double* delta_out, int32_t* trials_out,
                               int32_t* step_out, int32_t* iters_done, const cgmr_factor_types* types, const cgmr_robust* rk) {
  return dl_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, rk, types}), iters, params,
      {chi2_out, delta_out, trials_out, step_out, iters_done});
}

int cgmr_marginals_typed(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                         const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query,
                         double* cov_out, const cgmr_factor_types* types, const cgmr_robust* rk) {
  return marginal_driver(ctx, 0, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk, types}), -1, nK, query, nullptr, nullptr, nullptr, cov_out);
}

int cgmr_marginals_all_typed(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                             const int32_t* et, const double* meas, const double* info, double* cov_out, double* cross_out,
                             const cgmr_factor_types* types, const cgmr_robust* rk) {
  return marginals_all_driver(ctx, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk, types}), cov_out, cross_out);
}

/* max-mixture edges (include/cgmr.h: cgmr_mixture): the typed entry points without a robust kernel, plus the mixture */
int cgmr_gn_optimize_mixture(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas, const double* info, int iters, double* chi2_out,
                             const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return gn_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, nullptr, ft, mix}), iters, chi2_out);
}
int cgmr_gn_optimize_mixture_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                 const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, double* chi2_out,
                                 const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return gn_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, nullptr, ft, mix}), iters, chi2_out);
}
int cgmr_lm_optimize_mixture(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_lm_params* params,
                             double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done,
                             const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return lm_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, nullptr, ft, mix}), iters, params,
      {chi2_out, lambda_out, trials_out, iters_done});
}
int cgmr_lm_optimize_mixture_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                 const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                                 const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                                 int32_t* iters_done, const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return lm_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, nullptr, ft, mix}), iters, params,
      {chi2_out, lambda_out, trials_out, iters_done});
}
int cgmr_dl_optimize_mixture(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_dl_params* params,
                             double* chi2_out, double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                             const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return dl_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, nullptr, ft, mix}), iters, params,
      {chi2_out, delta_out, trials_out, step_out, iters_done});
}
int cgmr_dl_optimize_mixture_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                 const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                                 const cgmr_dl_params* params, double* chi2_out, double* delta_out, int32_t* trials_out,
                                 int32_t* step_out, int32_t* iters_done, const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return dl_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, nullptr, ft, mix}), iters, params,
      {chi2_out, delta_out, trials_out, step_out, iters_done});
}
/* chi2 and selection at the given poses: Gauss-Newton with no iteration, which is its one chi-only pass */
int cgmr_mixture_select(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                        const int32_t* to_idx, const double* meas, const double* info, const cgmr_factor_types* ft,
                        const cgmr_mixture* mix, double* chi2_out) {
  if (!ctx) return CGMR_E_INVALID;
  if (nV < 0 || (nV > 0 && !poses)) return set_err(ctx, CGMR_E_INVALID, "cgmr_mixture_select: null or negative argument");
  std::vector<double> x(poses, poses + 3 * (size_t)nV);
  return gn_optimize_impl(ctx, host_call(nV, x.data(), fixed, nE, from_idx, to_idx, meas, info, {false, nullptr, ft, mix}), 0, chi2_out);
}

cgmr_gnc_params cgmr_gnc_params_default(void) { return gnc_params_default(); }

int cgmr_gnc_optimize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                      const int32_t* to_idx, const double* meas, const double* info, const cgmr_factor_types* types,
                      const cgmr_gnc_params* params, double* mu_out, double* cost_out, int32_t* partial_out, int32_t* outer_done) {
  return gnc_optimize_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, nullptr, types}), params, mu_out, cost_out, partial_out,
      outer_done);
}
int cgmr_gnc_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                          const int32_t* to_idx, const double* d_meas, const double* d_info, const cgmr_factor_types* types,
                          const cgmr_gnc_params* params, double* mu_out, double* cost_out, int32_t* partial_out,
                          int32_t* outer_done) {
  return gnc_optimize_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, nullptr, types}), params, mu_out, cost_out, partial_out,
      outer_done);
}

int cgmr_chordal_initialize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas, const double* info, int stages, double* chi2_out,
                            int32_t* counts_out) {
  return chordal_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info), stages, chi2_out, counts_out);
}
int cgmr_chordal_initialize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                const int32_t* to_idx, const double* d_meas, const double* d_info, int stages, double* chi2_out,
                                int32_t* counts_out) {
  return chordal_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true}), stages, chi2_out, counts_out);
}

int cgmr_chordal_initialize_typed(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                  const int32_t* to_idx, const double* meas, const double* info, int stages, double* chi2_out,
                                  int32_t* counts_out, const cgmr_factor_types* types) {
  return chordal_impl(ctx, host_call(nV, poses, fixed, nE, from_idx, to_idx, meas, info, {false, nullptr, types}), stages, chi2_out, counts_out);
}
int cgmr_chordal_initialize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE,
                                      const int32_t* from_idx, const int32_t* to_idx, const double* d_meas, const double* d_info,
                                      int stages, double* chi2_out, int32_t* counts_out, const cgmr_factor_types* types) {
  return chordal_impl(ctx, host_call(nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, {true, nullptr, types}), stages, chi2_out, counts_out);
}

int cgmr_initial_guess(int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx, const int32_t* to_idx,
                       const double* meas) {
  if (nV < 0 || nE < 0 || (nV > 0 && (!poses || !fixed)) || (nE > 0 && (!from_idx || !to_idx || !meas))) return CGMR_E_INVALID;
  for (int k = 0; k < nE; k++)
    if (from_idx[k] < 0 || from_idx[k] >= nV || to_idx[k] < 0 || to_idx[k] >= nV) return CGMR_E_INVALID;
  initial_guess_host(nV, poses, fixed, nE, from_idx, to_idx, meas);
  return CGMR_OK;
}

int cgmr_gnc_last_stats(const cgmr_ctx* ctx, int64_t out[2]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  out[0] = ctx->gnc_stats[0];
  out[1] = ctx->gnc_stats[1];
  return CGMR_OK;
}

int cgmr_dl_last_stats(const cgmr_ctx* ctx, int64_t out[3]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  for (int k = 0; k < 3; k++) out[k] = ctx->dl_stats[k];
  return CGMR_OK;
}

int cgmr_gn_symbolic_info(int nV, const uint8_t* fixed, int nE, const int32_t* from_idx, const int32_t* to_idx,
                          int64_t out[16], int32_t* perm_out) {
  if (nV < 0 || nE < 0 || !out) return CGMR_E_INVALID;
  Symbolic S;
  (void)fixed;          // the solver applies the fixed flags numerically: they are not part of the analysis
  int rc = analyze(nV, nullptr, nE, from_idx, to_idx, S, read_switches());
  if (rc) return CGMR_E_INVALID;
  symbolic_info_out(S, nV, out, perm_out);
  return CGMR_OK;
}

int cgmr_gn_symbolic_info_grown(int nV0, int nE0, int n_steps, const int32_t* nV_step, const int32_t* nE_step,
                                const int32_t* from_idx, const int32_t* to_idx, int64_t out[16], int32_t* perm_out,
                                int32_t* n_extended_out) {
  if (nV0 < 0 || nE0 < 0 || n_steps < 0 || !out || (n_steps > 0 && (!nV_step || !nE_step))) return CGMR_E_INVALID;
  Symbolic S;
  const Switches sw = read_switches();
  if (analyze(nV0, nullptr, nE0, from_idx, to_idx, S, sw)) return CGMR_E_INVALID;
  int nV = nV0, next = 0;
  for (int k = 0; k < n_steps; k++) {
    if (nV_step[k] < nV || nE_step[k] < S.nE) return CGMR_E_INVALID;
    Symbolic old = std::move(S);
    if (analyze(nV_step[k], nullptr, nE_step[k], from_idx, to_idx, S, sw, &old)) return CGMR_E_INVALID;
    nV = nV_step[k];
    next += S.extended ? 1 : 0;
  }
  if (n_extended_out) *n_extended_out = next;
  symbolic_info_out(S, nV, out, perm_out);
  return CGMR_OK;
}

int cgmr_marginals(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                   const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query,
                   double* cov_out) {
  return cgmr_marginals_robust(ctx, nV, poses, fixed, nE, ef, et, meas, info, nK, query, cov_out, nullptr);
}

int cgmr_marginals_all(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                       const int32_t* et, const double* meas, const double* info, double* cov_out, double* cross_out) {
  return marginals_all_driver(ctx, host_call(nV, poses, fixed, nE, ef, et, meas, info), cov_out, cross_out);
}

int cgmr_covariance_estimate(cgmr_ctx* ctx, int nV, const double* poses, int nE, const int32_t* ef, const int32_t* et,
                             const double* meas, const double* info, int gauge, int nK, const int32_t* query,
                             double* cov_out) {
  return cgmr_covariance_estimate_robust(ctx, nV, poses, nE, ef, et, meas, info, gauge, nK, query, cov_out, nullptr);
}

int cgmr_condense(cgmr_ctx* ctx, int nV, const double* poses, int nE, const int32_t* ef, const int32_t* et,
                  const double* meas, const double* info, int gauge, int nK, const int32_t* query, int32_t* to_out,
                  double* est_out, double* info_out, double* cov_out) {
  return cgmr_condense_robust(ctx, nV, poses, nE, ef, et, meas, info, gauge, nK, query, to_out, est_out, info_out, cov_out, nullptr);
}

int cgmr_marginals_robust(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                          const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query,
                          double* cov_out, const cgmr_robust* rk) {
  if (!ctx || !cov_out) return CGMR_E_INVALID;
  return marginal_driver(ctx, 0, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk}), -1, nK, query, nullptr, nullptr, nullptr, cov_out);
}

int cgmr_marginals_all_robust(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                              const int32_t* et, const double* meas, const double* info, double* cov_out, double* cross_out,
                              const cgmr_robust* rk) {
  return marginals_all_driver(ctx, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk}), cov_out, cross_out);
}

int cgmr_covariance_estimate_robust(cgmr_ctx* ctx, int nV, const double* poses, int nE, const int32_t* ef, const int32_t* et,
                                    const double* meas, const double* info, int gauge, int nK, const int32_t* query,
                                    double* cov_out, const cgmr_robust* rk) {
  if (!ctx || !cov_out) return CGMR_E_INVALID;
  return marginal_driver(ctx, 1, host_call(nV, poses, nullptr, nE, ef, et, meas, info, {false, rk}), gauge, nK, query, nullptr, nullptr, nullptr, cov_out);
}

int cgmr_condense_robust(cgmr_ctx* ctx, int nV, const double* poses, int nE, const int32_t* ef, const int32_t* et,
                         const double* meas, const double* info, int gauge, int nK, const int32_t* query, int32_t* to_out,
                         double* est_out, double* info_out, double* cov_out, const cgmr_robust* rk) {
  if (!ctx || !to_out || !est_out || !info_out) return CGMR_E_INVALID;
  return marginal_driver(ctx, 2, host_call(nV, poses, nullptr, nE, ef, et, meas, info, {false, rk}), gauge, nK, query, to_out, est_out, info_out, cov_out);
}

int cgmr_marginals_joint(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                         const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query, double* cov_out,
                         const cgmr_robust* rk) {
  return joint_driver(ctx, "cgmr_marginals_joint", 0, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk}), nK, query, nullptr, cov_out, nullptr,
      nullptr, nullptr, nullptr);
}

int cgmr_marginals_pairs(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                         const int32_t* et, const double* meas, const double* info, int nP, const int32_t* pair_a,
                         const int32_t* pair_b, double* cov_aa_out, double* cov_ab_out, double* cov_bb_out, const cgmr_robust* rk) {
  return joint_driver(ctx, "cgmr_marginals_pairs", 1, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk}), nP, pair_a, pair_b, cov_aa_out, cov_ab_out,
      cov_bb_out, nullptr, nullptr);
}

int cgmr_relative_covariance(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                             const int32_t* et, const double* meas, const double* info, int nP, const int32_t* pair_a,
                             const int32_t* pair_b, double* rel_xyt_out, double* rel_cov_out, const double* hyp_meas,
                             const double* hyp_info, double* d2_out, const cgmr_robust* rk) {
  return joint_driver(ctx, "cgmr_relative_covariance", 2, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk}), nP, pair_a, pair_b, rel_xyt_out,
      rel_cov_out, d2_out, hyp_meas, hyp_info);
}

int cgmr_marginals_joint_typed(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                               const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query,
                               double* cov_out, const cgmr_factor_types* types, const cgmr_robust* rk) {
  return joint_driver(ctx, "cgmr_marginals_joint_typed", 0, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk, types}), nK, query, nullptr, cov_out,
      nullptr, nullptr, nullptr, nullptr);
}
int cgmr_marginals_pairs_typed(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                               const int32_t* et, const double* meas, const double* info, int nP, const int32_t* pair_a,
                               const int32_t* pair_b, double* cov_aa_out, double* cov_ab_out, double* cov_bb_out,
                               const cgmr_factor_types* types, const cgmr_robust* rk) {
  return joint_driver(ctx, "cgmr_marginals_pairs_typed", 1, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk, types}), nP, pair_a, pair_b, cov_aa_out,
      cov_ab_out, cov_bb_out, nullptr, nullptr);
}

int cgmr_observation_covariance(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                                const int32_t* et, const double* meas, const double* info, int nP, const int32_t* pair_a,
                                const int32_t* pair_b, const uint8_t* obs_kind, double* z_out, double* cov_out,
                                const double* hyp_meas, const double* hyp_info, double* d2_out, const cgmr_factor_types* types,
                                const cgmr_robust* rk) {
  return joint_driver(ctx, "cgmr_observation_covariance", 2, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk, types}), nP, pair_a, pair_b, z_out,
      cov_out, d2_out, hyp_meas, hyp_info, true, obs_kind);
}

int cgmr_closure_consistency(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                             const int32_t* et, const double* meas, const double* info, int nC, const int32_t* cl_a,
                             const int32_t* cl_b, const double* cl_meas, const double* cl_info, double gamma, double* d2_out,
                             uint64_t* adj_out, int32_t* clique_out, int32_t* clique_size_out, int32_t* seed_out,
                             const cgmr_robust* rk) {
  return pcm_driver(ctx, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk}), nC, cl_a, cl_b, cl_meas, cl_info, gamma, d2_out, adj_out, clique_out,
      clique_size_out, seed_out);
}

int cgmr_max_clique_greedy(cgmr_ctx* ctx, int n, const uint64_t* adj_bits, int32_t* clique_out, int32_t* clique_size_out,
                           int32_t* seed_out) {
  if (!ctx) return CGMR_E_INVALID;
  return clique_driver(ctx, n, adj_bits, clique_out, clique_size_out, seed_out);
}

int cgmr_closure_consistency_exact(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                                   const int32_t* et, const double* meas, const double* info, int nC, const int32_t* cl_a,
                                   const int32_t* cl_b, const double* cl_meas, const double* cl_info, double gamma, double* d2_out,
                                   uint64_t* adj_out, int64_t node_limit, int32_t* clique_out, int32_t* clique_size_out,
                                   int32_t* proven_out, const cgmr_robust* rk) {
  const CliqueExact ex{node_limit, proven_out, nullptr};
  return pcm_driver(ctx, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk}), nC, cl_a, cl_b, cl_meas, cl_info, gamma, d2_out, adj_out, clique_out,
      clique_size_out, nullptr, &ex);
}

int cgmr_closure_consistency_inter(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                                   const int32_t* et, const double* meas, const double* info, int nC, const int32_t* cl_a,
                                   const double* peer_pose, const double* peer_cov, const double* cl_meas, const double* cl_info,
                                   double gamma, double* d2_out, uint64_t* adj_out, int32_t* clique_out, int32_t* clique_size_out,
                                   int32_t* seed_out, const cgmr_robust* rk) {
  const PcmInter inter{peer_pose, peer_cov};
  return pcm_driver(ctx, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk}), nC, cl_a, nullptr, cl_meas, cl_info, gamma, d2_out, adj_out,
      clique_out, clique_size_out, seed_out, nullptr, &inter);
}

int cgmr_closure_consistency_inter_exact(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                                         const int32_t* et, const double* meas, const double* info, int nC, const int32_t* cl_a,
                                         const double* peer_pose, const double* peer_cov, const double* cl_meas,
                                         const double* cl_info, double gamma, double* d2_out, uint64_t* adj_out, int64_t node_limit,
                                         int32_t* clique_out, int32_t* clique_size_out, int32_t* proven_out, const cgmr_robust* rk) {
  const CliqueExact ex{node_limit, proven_out, nullptr};
  const PcmInter inter{peer_pose, peer_cov};
  return pcm_driver(ctx, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk}), nC, cl_a, nullptr, cl_meas, cl_info, gamma, d2_out, adj_out,
      clique_out, clique_size_out, nullptr, &ex, &inter);
}

int cgmr_max_clique_exact(cgmr_ctx* ctx, int n, const uint64_t* adj_bits, int64_t node_limit, int32_t* clique_out,
                          int32_t* clique_size_out, int32_t* proven_out, int64_t* nodes_out) {
  if (!ctx) return CGMR_E_INVALID;
  const CliqueExact ex{node_limit, proven_out, nodes_out};
  return clique_driver(ctx, n, adj_bits, clique_out, clique_size_out, nullptr, &ex);
}

int cgmr_jcbb_dense(cgmr_ctx* ctx, int nM, int nL, int nA, const int32_t* obs_pose_slot, const int32_t* obs_dim,
                    const double* sigma, const double* e, const double* J, const double* R_upper, const double* gamma_by_dof,
                    int64_t node_limit, double* ic_d2_out, int32_t* assign_out, int32_t* count_out, double* d2_out,
                    int32_t* dof_out, int32_t* proven_out, int64_t* nodes_out) {
  const JcOut out{ic_d2_out, assign_out, count_out, d2_out, dof_out, proven_out, nodes_out};
  return jc_dense_driver(ctx, nM, nL, nA, obs_pose_slot, obs_dim, sigma, e, J, R_upper, gamma_by_dof, node_limit, out);
}

int cgmr_joint_compatibility(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                             const int32_t* et, const double* meas, const double* info, int nM, const int32_t* obs_pose,
                             const uint8_t* obs_kind, const double* obs_meas, const double* obs_info, int nL,
                             const int32_t* landmark_idx, const double* gamma_by_dof, int64_t node_limit, double* ic_d2_out,
                             int32_t* assign_out, int32_t* count_out, double* d2_out, int32_t* dof_out, int32_t* proven_out,
                             int64_t* nodes_out, const cgmr_factor_types* types, const cgmr_robust* rk) {
  const JcOut out{ic_d2_out, assign_out, count_out, d2_out, dof_out, proven_out, nodes_out};
  return jc_driver(ctx, host_call(nV, poses, fixed, nE, ef, et, meas, info, {false, rk, types}), nM, obs_pose, obs_kind, obs_meas,
                   obs_info, nL, landmark_idx, gamma_by_dof, node_limit, out);
}

int cgmr_condense_tree(cgmr_ctx* ctx, int nV, const double* poses, int nE, const int32_t* ef, const int32_t* et, const double* meas,
                       const double* info, int gauge, int nK, const int32_t* query, int32_t* from_out, int32_t* to_out,
                       double* est_out, double* info_out, double* weight_out, int32_t* flags_out, const cgmr_robust* rk) {
  return condense_tree_driver(ctx, host_call(nV, poses, nullptr, nE, ef, et, meas, info, {false, rk}), gauge, nK, query, from_out, to_out,
                              est_out, info_out, weight_out, flags_out);
}

int cgmr_min_spanning_tree(cgmr_ctx* ctx, int n, const double* weights, int root, int32_t* parent_out) {
  if (!ctx) return CGMR_E_INVALID;
  return mst_driver(ctx, n, weights, root, parent_out);
}

int cgmr_remove_nodes(cgmr_ctx* ctx, int nV, int nE, const int32_t* ef, const int32_t* et, const double* meas, const double* info, int nR,
                      const int32_t* remove, int cap_out, int32_t* off_out, int32_t* from_out, int32_t* to_out, double* meas_out,
                      double* info_out, double* weight_out, int32_t* flags_out) {
  if (!ctx) return CGMR_E_INVALID;
  return remove_nodes_driver(ctx, nV, nE, ef, et, meas, info, nR, remove, cap_out, off_out, from_out, to_out, meas_out, info_out,
                             weight_out, flags_out);
}

int cgmr_set_symbolic_cache(cgmr_ctx* ctx, int on) {
  if (!ctx) return CGMR_E_INVALID;
  ctx->sym_cache_on = on != 0;
  ctx->sym_valid = false;
  return CGMR_OK;
}

int cgmr_host_threads_info(int32_t out[5]) {
  if (!out) return CGMR_E_INVALID;
  int v[5];
  host_pool_info(v);
  for (int k = 0; k < 5; k++) out[k] = v[k];
  return CGMR_OK;
}

int cgmr_symbolic_cache_stats(const cgmr_ctx* ctx, int64_t out[2]) {     // the two-value ABI of version 100
  if (!ctx || !out) return CGMR_E_INVALID;
  out[0] = ctx->sym_hits; out[1] = ctx->sym_misses + ctx->sym_extended;
  return CGMR_OK;
}

int cgmr_symbolic_cache_stats3(const cgmr_ctx* ctx, int64_t out[3]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  out[0] = ctx->sym_hits; out[1] = ctx->sym_misses; out[2] = ctx->sym_extended;
  return CGMR_OK;
}

int64_t cgmr_gn_timeouts(const cgmr_ctx* ctx) { return ctx ? ctx->gn_timeouts : -1; }

int cgmr_switches(const cgmr_ctx* ctx, char* buf, int cap) {
  if (cap < 0 || (cap > 0 && !buf)) return CGMR_E_INVALID;
  const Switches defaults;
  return list_switches(ctx ? ctx->sw : defaults, ctx ? process_switches() : defaults, buf, cap);
}

int cgmr_gn_last_timing(const cgmr_ctx* ctx, double out[5]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  memcpy(out, ctx->timing, sizeof(double) * 5);
  return CGMR_OK;
}

int cgmr_set_profiling(cgmr_ctx* ctx, int on) {
  if (!ctx) return CGMR_E_INVALID;
  ctx->profiling = on != 0;
  memset(ctx->ksec, 0, sizeof ctx->ksec);
  memset(ctx->klaunch, 0, sizeof ctx->klaunch);
  ctx->ev_cls.clear();
  if (on && ctx->ev_pool.empty()) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->ev_pool.resize(2 * 2048);              // enough for optimize(~30) on a 21-level tree; further launches go untimed
    for (hipEvent_t& e : ctx->ev_pool)
      if (hipEventCreate(&e) != hipSuccess) { ctx->ev_pool.clear(); return set_err(ctx, CGMR_E_HIP, "hipEventCreate failed"); }
  }
  return CGMR_OK;
}

int cgmr_gn_kernel_times(const cgmr_ctx* ctx, double seconds_out[8], int64_t launches_out[8]) {
  if (!ctx || !seconds_out || !launches_out) return CGMR_E_INVALID;
  memcpy(seconds_out, ctx->ksec, sizeof(double) * 8);
  memcpy(launches_out, ctx->klaunch, sizeof(int64_t) * 8);
  return CGMR_OK;
}

// the same with the classes beyond the first eight: 8 = front_level (k_front_level: a tree level's factorisation and its update
// tiles in one launch); classes 9..11 are pcm_driver's / clique_driver's
extern "C" int cgmr_gn_kernel_times_ex(const cgmr_ctx* ctx, double seconds_out[12], int64_t launches_out[12]) {
  if (!ctx || !seconds_out || !launches_out) return CGMR_E_INVALID;
  memcpy(seconds_out, ctx->ksec, sizeof(double) * 12);
  memcpy(launches_out, ctx->klaunch, sizeof(int64_t) * 12);
  return CGMR_OK;
}

}  // extern "C"
