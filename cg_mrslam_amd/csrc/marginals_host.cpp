// The marginals family (host_call.h): the drivers of the marginals, joint, PCM, clique and condensed-tree entry points.
// Compiled with hipcc; contains no kernels.
#include "condense_tree_device.h"
#include "marg_call.h"
#include "pcm_device.h"

#include <algorithm>
#include <cstring>

namespace cgmr {

// a point's dummy unknown out of a 3x3 block of H^-1: third row (the block's row vertex is a point) / third column (its column vertex is)
static void zero_point_dims(double* blk, bool row_point, bool col_point) {
  if (row_point) blk[6] = blk[7] = blk[8] = 0.0;
  if (col_point) blk[2] = blk[5] = blk[8] = 0.0;
}

// fixGauge and the spanning-tree guess from it: the linearisation point of marginal_driver's modes 1 and 2 and of
// condense_tree_driver (call.work: the private copy of the poses)
static void gauge_guess(MargCall& call, int gauge, std::vector<uint8_t>& fixed) {
  const HostCall& c = call.c;
  fixed[gauge] = 1;                                                   // fixGauge: every other vertex is freed
  initial_guess_host(c.nV, call.work.data(), fixed.data(), c.nE, c.ef, c.et, c.meas);
}

// the permuted column of every vertex of `verts`, or -1 (fixed / inactive: zeros)
static std::vector<int32_t> query_columns(const cgmr_ctx* ctx, const std::vector<int32_t>& verts) {
  std::vector<int32_t> qcol(verts.size());
  for (size_t k = 0; k < verts.size(); k++) qcol[k] = ctx->vmask[verts[k]] ? -1 : ctx->sym.vperm[verts[k]];
  return qcol;
}

// The dense Gram half of a joint call -- every lower tile of Y^T Y, in 64x64 macro-tiles -- as joint_driver's mode 0,
// pcm_driver and condense_tree_driver use it: the tile count and the row split for the layout M of the unique vertices ...
static void dense_gram_plan(const MargLayout& M, JointGram& JG) {
  const int T = M.m / 16;
  JG.tiles = nullptr;
  JG.ntile = (long long)T * (T + 1) / 2;
  joint_gram_split(M.n, (long long)((T + 3) / 4) * ((T + 3) / 4 + 1) / 2, &JG.rows, &JG.nsplit);
}
// ... and, behind the pass, the solve half (Y = L^-1 E for the nU vertices' columns) with the tiles after it
static void queue_solve_and_gram(hipStream_t st, const GnDevice& D, int nU, char* d, const MargLayout& ML, const JointGram& JG) {
  launch_marginals_solve(st, D, nU, (const int32_t*)(d + ML.o_qc), ML.m, (double*)(d + ML.o_Y), (double*)(d + ML.o_U),
                         (uint8_t*)(d + ML.o_live));
  launch_joint_gram(st, ML.n, ML.m, (const double*)(d + ML.o_Y), JG);
}

// Shared driver of cgmr_marginals / cgmr_covariance_estimate / cgmr_condense (host pointers).
//   mode 0: marginals at `poses` with `fixed`;  mode 1: covariance estimate (gauge);  mode 2: condense (gauge)
int marginal_driver(cgmr_ctx* ctx, int mode, const HostCall& c, int gauge, int nK, const int32_t* query, int32_t* to_out,
                    double* est_out, double* info_out, double* cov_out) {
  MargCall call(ctx, c);
  int rc = call.args(nK < 0 || (nK > 0 && !query), "marginals");
  if (rc) return rc;
  if (mode != 0 && (gauge < 0 || gauge >= c.nV)) return set_err(ctx, CGMR_E_INVALID, "gauge index out of range");
  for (int k = 0; k < nK; k++)
    if (query[k] < 0 || query[k] >= c.nV) return set_err(ctx, CGMR_E_INVALID, "query index out of range");
  // (the linearisation point: the poses given, or the spanning-tree guess of modes 1 and 2)
  rc = call.open(c.ft ? "cgmr_marginals_typed" : mode == 0 ? "cgmr_marginals_robust" : mode == 1 ? "cgmr_covariance_estimate_robust" : "cgmr_condense_robust",
                 "cgmr_marginals_typed");                               // (the types: mode 0 only, cgmr_marginals_typed)
  if (rc) return rc;
  const TypedHost& typed = call.typed;
  std::vector<uint8_t> fixed(c.nV, 0);
  if (mode == 0) { if (!c.fixed) return set_err(ctx, CGMR_E_INVALID, "fixed flags missing"); fixed.assign(c.fixed, c.fixed + c.nV); }
  else gauge_guess(call, gauge, fixed);
  // query list (condense: everything but the gauge)
  std::vector<int32_t> q;
  for (int k = 0; k < nK; k++) if (mode != 2 || query[k] != gauge) q.push_back(query[k]);
  const int nq = (int)q.size();
  if (cov_out && mode != 2) memset(cov_out, 0, sizeof(double) * 9 * (size_t)nK);
  rc = call.structure(fixed.data());
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  if (D.nf == 0 || nq == 0) { HIP_TRY(ctx, hipStreamSynchronize(st)); return mode == 2 ? 0 : CGMR_OK; }
  // staging: poses | meas | info | the marginals' and labels' work space
  const MargLayout M(nq, D.nf, S.rows.size(), D.nfronts, call.L.off);
  call.L.off = M.end;
  rc = call.stage();
  if (rc) return rc;
  char* d = call.d;
  const std::vector<int32_t> qcol = query_columns(ctx, q);
  HIP_TRY(ctx, hipMemcpyAsync(d + M.o_qc, qcol.data(), 4 * (size_t)nq, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + M.o_qv, q.data(), 4 * (size_t)nq, hipMemcpyHostToDevice, st));
  // the Hessian of this iteration (linearised at the initial guess) is what computeMarginals sees [g2o-recalled];
  // for the condensed graph the iteration is completed first: the factor stays valid, the poses move on
  std::vector<double> cov(9 * (size_t)nq);
  GnPassOpts pass;
  pass.solve = pass.update_poses = mode == 2;
  rc = call.run(pass, [&]() -> int {
    launch_marginals(st, D, nq, (const int32_t*)(d + M.o_qc), M.m, (double*)(d + M.o_Y), (double*)(d + M.o_U), (double*)(d + M.o_part),
                     (double*)(d + M.o_G), (double*)(d + M.o_cov), M.chunk, M.nchunk, (uint8_t*)(d + M.o_live));
    if (mode == 2)
      launch_label(st, nq, (const int32_t*)(d + M.o_qv), gauge, call.dp, (const double*)(d + M.o_cov), (double*)(d + M.o_est),
                   (double*)(d + M.o_info), (int*)(d + M.o_fl));
    HIP_TRY(ctx, hipMemcpyAsync(cov.data(), d + M.o_cov, 72 * (size_t)nq, hipMemcpyDeviceToHost, st));
    if (mode == 2) {
      HIP_TRY(ctx, hipMemcpyAsync(est_out, d + M.o_est, 24 * (size_t)nq, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipMemcpyAsync(info_out, d + M.o_info, 48 * (size_t)nq, hipMemcpyDeviceToHost, st));
    }
    return 0;
  });
  if (rc) return rc;
  rc = call.close();
  if (rc) return rc;
  if (mode == 2) {
    for (int k = 0; k < nq; k++) to_out[k] = q[k];
    if (cov_out) memcpy(cov_out, cov.data(), 72 * (size_t)nq);
    return nq;
  }
  // scatter back in query order; fixed / inactive queries keep zeros
  for (int k = 0; k < nq; k++)
    if (qcol[k] >= 0) {
      memcpy(cov_out + 9 * (size_t)k, cov.data() + 9 * (size_t)k, 72);
      if (typed.any && typed.vk[q[k]]) zero_point_dims(cov_out + 9 * (size_t)k, true, true);
    }
  return CGMR_OK;
}

// cgmr_marginals_all: Sigma of every front by selected inversion of the factor (selinv_kernels.hip), then the diagonal block
// of every vertex and the block of every edge.  The same pass as marginal_driver's mode 0 (gn_pass at `poses` with `fixed`).
int marginals_all_driver(cgmr_ctx* ctx, const HostCall& c, double* cov_out, double* cross_out) {
  MargCall call(ctx, c);
  int rc = call.args(!cov_out, "marginals");
  if (rc) return rc;
  if (!c.fixed) return set_err(ctx, CGMR_E_INVALID, "fixed flags missing");
  rc = call.open(c.ft ? "cgmr_marginals_all_typed" : "cgmr_marginals_all_robust", "cgmr_marginals_all_typed");
  if (rc) return rc;
  const TypedHost& typed = call.typed;
  auto zero_outputs = [&]() {
    memset(cov_out, 0, 72 * (size_t)c.nV);
    if (cross_out) memset(cross_out, 0, 72 * (size_t)c.nE);
  };
  zero_outputs();
  rc = call.structure(c.fixed);
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  if (D.nf == 0) { HIP_TRY(ctx, hipStreamSynchronize(st)); return CGMR_OK; }
  // every front's block of Sigma (own columns, then the border), and the row tiles of k_selinv_border level by level
  const int nfr = (int)S.fronts.size();
  std::vector<int64_t> soff(nfr + 1, 0);
  for (int f = 0; f < nfr; f++) {
    const int64_t n = 3 * (int64_t)(S.fronts[f].nc + S.fronts[f].ns);
    soff[f + 1] = soff[f] + n * n;
  }
  SelinvPlan P;
  std::vector<int32_t> tiles;
  P.h_tile_ptr.assign(D.nlevels_full + 1, 0);
  for (int l = 0; l < D.nlevels_full; l++) {
    for (int q = D.h_flevel_ptr[l]; q < D.h_flevel_ptr[l + 1]; q++) {
      const int f = S.level_fronts[q];
      if (S.fronts[f].parent < 0) continue;                             // (a root has no border)
      for (int t0 = 0; t0 < 3 * S.fronts[f].ns; t0 += kSelinvTileRows) { tiles.push_back(f); tiles.push_back(t0); }
    }
    P.h_tile_ptr[l + 1] = (int)tiles.size() / 2;
  }
  std::vector<int32_t> vcol(c.nV);
  for (int v = 0; v < c.nV; v++) vcol[v] = ctx->vmask[v] ? -1 : S.vperm[v];     // fixed / inactive: zeros
  // staging: poses | meas | info | vcol | col_front | soff | tiles | cov | cross;  Sigma: an arena of its own
  Layout256& L = call.L;
  const size_t o_vc = L.add(4 * (size_t)c.nV), o_cf = L.add(4 * (size_t)D.nf), o_so = L.add(8 * soff.size()), o_t = L.add(4 * tiles.size()),
               o_cov = L.add(72 * (size_t)c.nV), o_cr = L.add(72 * (size_t)c.nE);
  rc = arena_reserve(ctx, ctx->si_arena, 8 * (size_t)soff[nfr]);
  if (rc) return rc;
  rc = call.stage();
  if (rc) return rc;
  char* d = call.d;
  HIP_TRY(ctx, hipMemcpyAsync(d + o_vc, vcol.data(), 4 * (size_t)c.nV, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_cf, S.col_front.data(), 4 * (size_t)D.nf, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_so, soff.data(), 8 * soff.size(), hipMemcpyHostToDevice, st));
  if (!tiles.empty()) HIP_TRY(ctx, hipMemcpyAsync(d + o_t, tiles.data(), 4 * tiles.size(), hipMemcpyHostToDevice, st));
  P.Sig = (double*)ctx->si_arena.ptr;
  P.soff = (const int64_t*)(d + o_so);
  P.tiles = (const int32_t*)(d + o_t);
  GnPassOpts pass;
  pass.solve = false;
  rc = call.run(pass, [&]() -> int {
    launch_invert_fronts(st, D, /*top_too=*/true);                     // Z = L11^-1 of every front, the top block's included
    launch_selinv(st, D, P, c.nV, c.nE, (const int32_t*)(d + o_vc), (const int32_t*)(d + o_cf), (double*)(d + o_cov),
                  cross_out ? (double*)(d + o_cr) : nullptr);
    HIP_TRY(ctx, hipMemcpyAsync(cov_out, d + o_cov, 72 * (size_t)c.nV, hipMemcpyDeviceToHost, st));
    if (cross_out && c.nE > 0) HIP_TRY(ctx, hipMemcpyAsync(cross_out, d + o_cr, 72 * (size_t)c.nE, hipMemcpyDeviceToHost, st));
    return 0;
  });
  if (rc) return rc;
  rc = call.close();
  if (rc == CGMR_E_CHOLESKY_BASE) zero_outputs();
  if (rc == CGMR_OK && typed.any) {
    for (int v = 0; v < c.nV; v++) if (typed.vk[v]) zero_point_dims(cov_out + 9 * (size_t)v, true, true);
    if (cross_out) for (int k = 0; k < c.nE; k++) zero_point_dims(cross_out + 9 * (size_t)k, typed.vk[c.ef[k]] != 0, typed.vk[c.et[k]] != 0);
  }
  return rc;
}

// Shared driver of cgmr_marginals_joint / cgmr_marginals_pairs / cgmr_relative_covariance, their typed forms and
// cgmr_observation_covariance (`who`): the pass of marginal_driver's mode 0
// (gn_pass at `poses` with `fixed`), the solve half of launch_marginals for the unique vertices asked for, then the tiles of
// Y^T Y that hold a requested block (joint_marginals_kernels.hip).
//   mode 0: joint -- va = the nK queries, out_a = cov [(3 nK)^2]
//   mode 1: pairs -- (va, vb) the nP pairs, out_a / out_b / out_c = aa / ab / bb (nullable)
//   mode 2: relative covariance -- the pairs' blocks stay on the device; out_a / out_b / out_c = rel_xyt / rel_cov / d2 (nullable);
//           obs: cgmr_observation_covariance, pair p predicted as a factor of kind obs_kind[p] (null: all 0).  The pairs of
//           kind 0 are k_relative_cov's (it runs over the whole list when there is one), the others k_observation_cov's behind it.
// ft: the factor types (typed_check before the device is touched; a point's dummy third row / column comes back zero).
int joint_driver(cgmr_ctx* ctx, const char* who, int mode, const HostCall& c, int nQ, const int32_t* va, const int32_t* vb,
                 double* out_a, double* out_b, double* out_c, const double* hyp_meas, const double* hyp_info, bool obs,
                 const uint8_t* obs_kind) {
  MargCall call(ctx, c);
  int rc = call.args(nQ < 0 || !c.fixed || (nQ > 0 && (!va || (mode != 0 && !vb))) || (mode == 0 && nQ > 0 && !out_a) ||
                         (mode == 2 && ((out_c && !hyp_meas) || (hyp_info && !hyp_meas))), who);
  if (rc) return rc;
  for (int k = 0; k < nQ; k++)
    if (va[k] < 0 || va[k] >= c.nV || (mode != 0 && (vb[k] < 0 || vb[k] >= c.nV)))
      return set_err(ctx, CGMR_E_INVALID, "%s: vertex index out of range", who);
  rc = call.types(who);
  if (rc) return rc;
  const TypedHost& typed = call.typed;
  bool obs_typed = false, obs_pose = !obs;                        // some pair is a landmark observation / a relative pose
  if (obs)
    for (int k = 0; k < nQ; k++) {
      const int kind = obs_kind ? obs_kind[k] : 0;
      const bool a_pt = c.ft && !typed.vk.empty() && typed.vk[va[k]], b_pt = c.ft && !typed.vk.empty() && typed.vk[vb[k]];
      if (kind > CGMR_EDGE_BEARING_SE2_XY) return set_err(ctx, CGMR_E_INVALID, "%s: pair %d has observation kind %d (0, 1 or 2)", who, k, kind);
      if (a_pt) return set_err(ctx, CGMR_E_INVALID, "%s: pair %d is observed from vertex %d, a point", who, k, va[k]);
      if (kind == CGMR_EDGE_SE2 && b_pt) return set_err(ctx, CGMR_E_INVALID, "%s: pair %d of kind 0 (EDGE_SE2) ends at vertex %d, a point", who, k, vb[k]);
      if (kind != CGMR_EDGE_SE2 && !b_pt) return set_err(ctx, CGMR_E_INVALID, "%s: pair %d of kind %d ends at vertex %d, a pose", who, k, kind, vb[k]);
      if (kind) obs_typed = true; else obs_pose = true;
    }
  if (nQ == 0) return CGMR_OK;
  // the unique vertices, in order of first appearance: 4 columns of Y each
  std::vector<int32_t> slot_of(c.nV, -1), uq;
  auto slot = [&](int v) { if (slot_of[v] < 0) { slot_of[v] = (int32_t)uq.size(); uq.push_back(v); } return slot_of[v]; };
  for (int k = 0; k < nQ; k++) { slot(va[k]); if (mode != 0) slot(vb[k]); }
  const int nU = (int)uq.size();
  if (nU > CGMR_JOINT_MAX_QUERIES)
    return set_err(ctx, CGMR_E_INVALID, "%s: %d unique query vertices, at most CGMR_JOINT_MAX_QUERIES = %d", who, nU, CGMR_JOINT_MAX_QUERIES);
  rc = call.open(who);
  if (rc) return rc;
  rc = call.structure(c.fixed);
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  const size_t nq = (size_t)nQ;
  const size_t b_a = mode == 0 ? 72 * nq * nq : mode == 1 ? 72 * nq : 24 * nq, b_b = 72 * nq, b_c = mode == 1 ? 72 * nq : 8 * nq;
  auto zero_outputs = [&]() {
    if (out_a) memset(out_a, 0, b_a);
    if (mode != 0 && out_b) memset(out_b, 0, b_b);
    if (mode != 0 && out_c) memset(out_c, 0, b_c);
  };
  if (D.nf == 0 && mode != 2) { HIP_TRY(ctx, hipStreamSynchronize(st)); zero_outputs(); return CGMR_OK; }   // no free vertex: zeros
  call.factor = D.nf > 0;
  // the tiles: every lower one (joint), or those of the pairs' blocks, sorted, each once
  const MargLayout M(nU, D.nf, S.rows.size(), D.nfronts, 0);
  const int T = M.m / 16;
  const std::vector<int32_t> qcol = query_columns(ctx, uq);
  std::vector<int32_t> tl, pr;
  JointGram JG;
  if (mode == 0) {
    dense_gram_plan(M, JG);
    pr.resize(nQ);
    for (int k = 0; k < nQ; k++) pr[k] = qcol[slot_of[va[k]]] < 0 ? -1 : slot_of[va[k]];
  } else {
    std::vector<int64_t> keys;
    keys.reserve(3 * nq);
    auto key = [&](int sa, int sb) { const int I = std::max(sa, sb) / 4, J = std::min(sa, sb) / 4; return (int64_t)I * T + J; };
    for (int k = 0; k < nQ; k++) {
      const int sa = slot_of[va[k]], sb = slot_of[vb[k]];
      keys.push_back(key(sa, sa)); keys.push_back(key(sa, sb)); keys.push_back(key(sb, sb));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    JG.ntile = (long long)keys.size();
    tl.resize(2 * keys.size());
    for (size_t t = 0; t < keys.size(); t++) { tl[2 * t] = (int32_t)(keys[t] / T); tl[2 * t + 1] = (int32_t)(keys[t] % T); }
    auto pos = [&](int sa, int sb) { return (int32_t)(std::lower_bound(keys.begin(), keys.end(), key(sa, sb)) - keys.begin()); };
    pr.resize(5 * nq);
    for (int k = 0; k < nQ; k++) {
      const int sa = slot_of[va[k]], sb = slot_of[vb[k]];
      int32_t* P = &pr[5 * (size_t)k];
      P[0] = qcol[sa] < 0 ? -1 : sa; P[1] = qcol[sb] < 0 ? -1 : sb;
      P[2] = pos(sa, sa); P[3] = pos(sa, sb); P[4] = pos(sb, sb);
    }
  }
  if (mode != 0) joint_gram_split(M.n, JG.ntile, &JG.rows, &JG.nsplit);
  // staging: poses | meas | info | query columns, Y, border vectors, live flags (MargLayout) | tile list | pairs / slots |
  // partial tiles | tiles | outputs | the pair vertices and the hypotheses
  Layout256& L = call.L;
  const MargLayout ML(nU, D.nf, S.rows.size(), D.nfronts, L.off);
  L.off = ML.end;
  const size_t o_tl = L.add(4 * tl.size()), o_pr = L.add(4 * pr.size()),
               o_part = L.add(JG.nsplit > 1 ? 2048 * (size_t)JG.nsplit * (size_t)JG.ntile : 0), o_G = L.add(2048 * (size_t)JG.ntile),
               o_a = L.add(mode == 0 ? 72 * nq * nq : 72 * nq), o_b = L.add(mode == 0 ? 0 : 72 * nq), o_c = L.add(mode == 0 ? 0 : 72 * nq),
               o_va = L.add(mode == 2 ? 4 * nq : 0), o_vb = L.add(mode == 2 ? 4 * nq : 0), o_hm = L.add(mode == 2 && hyp_meas ? 24 * nq : 0),
               o_hi = L.add(mode == 2 && hyp_info ? 48 * nq : 0), o_rz = L.add(mode == 2 ? 24 * nq : 0), o_rc = L.add(mode == 2 ? 72 * nq : 0),
               o_d2 = L.add(mode == 2 ? 8 * nq : 0), o_ok = L.add(obs_typed ? nq : 0);
  rc = call.stage();
  if (rc) return rc;
  char* d = call.d;
  HIP_TRY(ctx, hipMemcpyAsync(d + ML.o_qc, qcol.data(), 4 * (size_t)nU, hipMemcpyHostToDevice, st));
  if (!tl.empty()) HIP_TRY(ctx, hipMemcpyAsync(d + o_tl, tl.data(), 4 * tl.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_pr, pr.data(), 4 * pr.size(), hipMemcpyHostToDevice, st));
  if (mode == 2) {
    HIP_TRY(ctx, hipMemcpyAsync(d + o_va, va, 4 * nq, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d + o_vb, vb, 4 * nq, hipMemcpyHostToDevice, st));
    if (hyp_meas) HIP_TRY(ctx, hipMemcpyAsync(d + o_hm, hyp_meas, 24 * nq, hipMemcpyHostToDevice, st));
    if (hyp_info) HIP_TRY(ctx, hipMemcpyAsync(d + o_hi, hyp_info, 48 * nq, hipMemcpyHostToDevice, st));
    if (obs_typed) HIP_TRY(ctx, hipMemcpyAsync(d + o_ok, obs_kind, nq, hipMemcpyHostToDevice, st));
  }
  if (mode != 0) JG.tiles = (const int32_t*)(d + o_tl);
  JG.part = (double*)(d + o_part);
  JG.G = (double*)(d + o_G);
  GnPassOpts pass;
  pass.solve = pass.update_poses = false;
  const bool want_d2 = mode == 2 && out_c;
  rc = call.run(pass, [&]() -> int {
    if (call.factor) {
      queue_solve_and_gram(st, D, nU, d, ML, JG);
      if (mode == 0) launch_joint_extract(st, nQ, (const int32_t*)(d + o_pr), JG.G, (double*)(d + o_a));
      else launch_pairs_extract(st, nQ, (const int32_t*)(d + o_pr), JG.G, (double*)(d + o_a), (double*)(d + o_b), (double*)(d + o_c));
    } else {                                                           // (mode 2 without a free vertex: zero blocks)
      HIP_TRY(ctx, hipMemsetAsync(d + o_a, 0, 72 * nq, st));
      HIP_TRY(ctx, hipMemsetAsync(d + o_b, 0, 72 * nq, st));
      HIP_TRY(ctx, hipMemsetAsync(d + o_c, 0, 72 * nq, st));
    }
    if (mode == 0) HIP_TRY(ctx, hipMemcpyAsync(out_a, d + o_a, b_a, hipMemcpyDeviceToHost, st));
    if (mode == 1) {
      if (out_a) HIP_TRY(ctx, hipMemcpyAsync(out_a, d + o_a, b_a, hipMemcpyDeviceToHost, st));
      if (out_b) HIP_TRY(ctx, hipMemcpyAsync(out_b, d + o_b, b_b, hipMemcpyDeviceToHost, st));
      if (out_c) HIP_TRY(ctx, hipMemcpyAsync(out_c, d + o_c, b_c, hipMemcpyDeviceToHost, st));
    }
    if (mode == 2 && obs_pose)
      launch_relative_cov(st, nQ, (const int32_t*)(d + o_va), (const int32_t*)(d + o_vb), call.dp, (const double*)(d + o_a),
                          (const double*)(d + o_b), (const double*)(d + o_c), hyp_meas ? (const double*)(d + o_hm) : nullptr,
                          hyp_info ? (const double*)(d + o_hi) : nullptr, (double*)(d + o_rz), (double*)(d + o_rc),
                          want_d2 ? (double*)(d + o_d2) : nullptr);
    if (mode == 2 && obs_typed)
      launch_observation_cov(st, nQ, (const int32_t*)(d + o_va), (const int32_t*)(d + o_vb), (const uint8_t*)(d + o_ok), call.dp,
                             (const double*)(d + o_a), (const double*)(d + o_b), (const double*)(d + o_c),
                             hyp_meas ? (const double*)(d + o_hm) : nullptr, hyp_info ? (const double*)(d + o_hi) : nullptr,
                             (double*)(d + o_rz), (double*)(d + o_rc), want_d2 ? (double*)(d + o_d2) : nullptr);
    if (mode == 2) {
      if (out_a) HIP_TRY(ctx, hipMemcpyAsync(out_a, d + o_rz, b_a, hipMemcpyDeviceToHost, st));
      if (out_b) HIP_TRY(ctx, hipMemcpyAsync(out_b, d + o_rc, b_b, hipMemcpyDeviceToHost, st));
      if (want_d2) HIP_TRY(ctx, hipMemcpyAsync(out_c, d + o_d2, b_c, hipMemcpyDeviceToHost, st));
    }
    return 0;
  });
  if (rc) return rc;
  rc = call.close();
  if (rc == CGMR_E_CHOLESKY_BASE) zero_outputs();
  if (rc == CGMR_OK && typed.any && mode == 0) {                  // the points' dummy unknowns: rows and columns 3 k + 2
    const size_t N = 3 * nq;
    for (int k = 0; k < nQ; k++)
      if (typed.vk[va[k]])
        for (size_t q = 0; q < N; q++) out_a[(3 * (size_t)k + 2) * N + q] = out_a[q * N + 3 * (size_t)k + 2] = 0.0;
  }
  if (rc == CGMR_OK && typed.any && mode == 1)
    for (int k = 0; k < nQ; k++) {
      const bool pa = typed.vk[va[k]] != 0, pb = typed.vk[vb[k]] != 0;
      if (out_a) zero_point_dims(out_a + 9 * (size_t)k, pa, pa);
      if (out_b) zero_point_dims(out_b + 9 * (size_t)k, pa, pb);
      if (out_c) zero_point_dims(out_c + 9 * (size_t)k, pb, pb);
    }
  return rc;
}

// What the clique kernels of pcm_kernels.hip work in, behind whatever the caller has put into L: the seeds' member bits and
// sizes and the result (size, seed, members).
// With `exact`, behind them what the exact solver of clique_exact_kernels.hip works in (pcm_device.h: ExactWork), its result
// (size, proven, members) and its node count: the order, the adjacency in bit positions, per round and root the clique found,
// its size, the stopped flag and the nodes, and the search stack -- one P of W words per root and depth, n levels deep, so
// 8 n^2 W bytes (128 MiB at n = 1024), sized here from n and W.
struct CliqueLayout {
  size_t o_sb, o_ss, o_out;
  size_t o_xvp = 0, o_xpv = 0, o_xB = 0, o_xbits = 0, o_xsize = 0, o_xstop = 0, o_xnodes = 0, o_xstack = 0, o_xout = 0, o_xtotal = 0;
  CliqueLayout(Layout256& L, int n, bool exact = false)
      : o_sb(L.add(8 * (size_t)n * ((n + 63) / 64))), o_ss(L.add(4 * (size_t)n)), o_out(L.add(4 * ((size_t)n + 2))) {
    if (!exact) return;
    const size_t N = (size_t)n, W = (N + 63) / 64, R = CGMR_EXACT_ROUNDS;
    o_xvp = L.add(4 * N); o_xpv = L.add(4 * N); o_xB = L.add(8 * N * W); o_xbits = L.add(8 * R * N * W);
    o_xsize = L.add(4 * R * N); o_xstop = L.add(4 * R * N); o_xnodes = L.add(8 * R * N); o_xstack = L.add(8 * N * N * W);
    o_xout = L.add(4 * (N + 2)); o_xtotal = L.add(8);
  }
  ExactWork work(char* d) const {
    ExactWork X;
    X.vtx_of_pos = (int32_t*)(d + o_xvp); X.pos_of_vtx = (int32_t*)(d + o_xpv);
    X.B = (unsigned long long*)(d + o_xB); X.bits = (unsigned long long*)(d + o_xbits);
    X.size = (int32_t*)(d + o_xsize); X.out_of_nodes = (int32_t*)(d + o_xstop);
    X.nodes = (long long*)(d + o_xnodes); X.stack = (unsigned long long*)(d + o_xstack);
    return X;
  }
  // the greedy launches, then with `ex` the exact ones; where the result (n + 2 ints) lies afterwards
  size_t launch(hipStream_t st, char* d, int n, size_t o_adj, const CliqueExact* ex) const {
    launch_clique_greedy(st, n, (const unsigned long long*)(d + o_adj), (unsigned long long*)(d + o_sb), (int32_t*)(d + o_ss),
                         (int32_t*)(d + o_out));
    if (!ex) return o_out;
    launch_clique_exact(st, n, (const unsigned long long*)(d + o_adj), ex->node_limit, (const int32_t*)(d + o_out), work(d),
                        (int32_t*)(d + o_xout), (long long*)(d + o_xtotal));
    return o_xout;
  }
};
// ... and where its result goes on the host once the stream has been waited for (res: n + 2 ints; res[1] the seed, or with `ex`
// proven, and the node count `total`)
static void clique_result_out(const std::vector<int32_t>& res, int n, int32_t* clique_out, int32_t* size_out, int32_t* seed_out,
                              const CliqueExact* ex = nullptr, int64_t total = 0) {
  *size_out = res[0];
  if (ex) { *ex->proven_out = res[1]; if (ex->nodes_out) *ex->nodes_out = total; }
  else *seed_out = res[1];
  memcpy(clique_out, res.data() + 2, 4 * (size_t)n);
}

// cgmr_closure_consistency: the pass and the solve half of joint_driver's mode 0 over the unique endpoints of the candidates,
// every lower Gram tile (the macro-tile path), then the kernels of pcm_kernels.hip on the tiles where they lie: d2 of every
// pair, its rows as bit words, the greedy clique of every seed and the best of them.  In profiling mode the launch classes
// 9 (solve + Gram), 10 (k_closure_consistency) and 11 (bits and clique) of cgmr_gn_kernel_times_ex are timed and collected.
// With `ex` (cgmr_closure_consistency_exact): the exact solver's launches behind the greedy ones, in class 11 as well.
// With `inter` (cgmr_closure_consistency_inter[_exact]): the unique endpoints are those of ca alone (at most nC), the peer's
// poses and, where given, their covariance go up beside the candidates, and class 10 is k_closure_consistency_inter; every
// step before and after is the same statement.
int pcm_driver(cgmr_ctx* ctx, const HostCall& c, int nC, const int32_t* ca, const int32_t* cb, const double* cmeas,
               const double* cinfo, double gamma, double* d2_out, uint64_t* adj_out, int32_t* clique_out, int32_t* size_out,
               int32_t* seed_out, const CliqueExact* ex, const PcmInter* inter) {
  const char* who = inter ? (ex ? "cgmr_closure_consistency_inter_exact" : "cgmr_closure_consistency_inter")
                          : (ex ? "cgmr_closure_consistency_exact" : "cgmr_closure_consistency");
  if (ex) seed_out = ex->proven_out;                               // (the third of the clique's outputs, for the checks below)
  MargCall call(ctx, c);
  const bool no_ends = inter ? !inter->peer_pose : !cb;             // (where the candidates end: the peer's poses, or b)
  int rc = call.args(nC < 0 || !c.fixed || (nC > 0 && (!ca || no_ends || !cmeas || !cinfo)), who);
  if (rc) return rc;
  const bool want_clique = clique_out || size_out || seed_out;
  if (want_clique && !(clique_out && size_out && seed_out))
    return set_err(ctx, CGMR_E_INVALID, "%s: clique_out, clique_size_out and %s are given together or not at all", who,
                   ex ? "proven_out" : "seed_out");
  if (nC > CGMR_PCM_MAX_CLOSURES)
    return set_err(ctx, CGMR_E_INVALID, "%s: %d closures, at most CGMR_PCM_MAX_CLOSURES = %d", who, nC, CGMR_PCM_MAX_CLOSURES);
  for (int k = 0; k < nC && !inter; k++)
    if (ca[k] < 0 || ca[k] >= c.nV || cb[k] < 0 || cb[k] >= c.nV)
      return set_err(ctx, CGMR_E_INVALID, "%s: closure %d (%d -> %d) has an endpoint outside [0, %d)", who, k, ca[k], cb[k], c.nV);
  for (int k = 0; k < nC && inter; k++) {
    if (ca[k] < 0 || ca[k] >= c.nV)
      return set_err(ctx, CGMR_E_INVALID, "%s: closure %d starts at vertex %d, outside [0, %d)", who, k, ca[k], c.nV);
    const double* pp = inter->peer_pose + 3 * (size_t)k;
    if (!(std::isfinite(pp[0]) && std::isfinite(pp[1]) && std::isfinite(pp[2])))
      return set_err(ctx, CGMR_E_INVALID, "%s: closure %d has a peer pose that is not finite", who, k);
  }
  if (inter && inter->peer_cov)                                    // the lower triangle is all that is read
    for (size_t r = 0, N3 = 3 * (size_t)nC; r < N3; r++) {
      const double* row = inter->peer_cov + r * N3;
      for (size_t q = 0; q <= r; q++)
        if (!std::isfinite(row[q]))
          return set_err(ctx, CGMR_E_INVALID, "%s: peer_cov (%zu, %zu), closures %zu and %zu, is not finite", who, r, q, r / 3, q / 3);
      if (row[r] < 0)
        return set_err(ctx, CGMR_E_INVALID, "%s: peer_cov (%zu, %zu), closure %zu, is a negative variance", who, r, r, r / 3);
    }
  if (!(std::isfinite(gamma) && gamma > 0)) return set_err(ctx, CGMR_E_INVALID, "%s: gamma must be finite and > 0", who);
  if (ex && ex->node_limit <= 0) return set_err(ctx, CGMR_E_INVALID, "%s: node_limit must be > 0", who);
  if (nC == 0) { if (size_out) *size_out = 0; return CGMR_OK; }
  // the unique endpoints, in order of first appearance: 4 columns of Y each (at most 2 nC <= CGMR_JOINT_MAX_QUERIES; with
  // `inter` the own ones alone, at most nC)
  std::vector<int32_t> slot_of(c.nV, -1), uq;
  auto slot = [&](int v) { if (slot_of[v] < 0) { slot_of[v] = (int32_t)uq.size(); uq.push_back(v); } return slot_of[v]; };
  for (int k = 0; k < nC; k++) { slot(ca[k]); if (!inter) slot(cb[k]); }
  const int nU = (int)uq.size();
  rc = call.open(who);
  if (rc) return rc;
  rc = call.structure(c.fixed);
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  call.factor = D.nf > 0;                                          // no free vertex: Sigma = 0, the measurement terms alone
  const MargLayout M(nU, D.nf, S.rows.size(), D.nfronts, 0);
  const int W = (nC + 63) / 64;
  const size_t n = (size_t)nC;
  const std::vector<int32_t> qcol = query_columns(ctx, uq);
  std::vector<int32_t> sl(2 * n);                                   // (with `inter`: one slot per candidate, the front half)
  for (int k = 0; k < nC && !inter; k++) {
    const int sa = slot_of[ca[k]], sb = slot_of[cb[k]];
    sl[2 * k] = qcol[sa] < 0 ? -1 : sa; sl[2 * k + 1] = qcol[sb] < 0 ? -1 : sb;
  }
  for (int k = 0; k < nC && inter; k++) { const int sa = slot_of[ca[k]]; sl[k] = qcol[sa] < 0 ? -1 : sa; }
  JointGram JG;
  dense_gram_plan(M, JG);
  // staging: poses | meas | info | query columns, Y, border vectors, live flags (MargLayout) | partial tiles | tiles | the
  // candidates (b, or with `inter` the peer's poses [| their covariance]) | d2 | bit words | the clique's work space
  Layout256& L = call.L;
  const MargLayout ML(nU, D.nf, S.rows.size(), D.nfronts, L.off);
  L.off = ML.end;
  const size_t o_part = L.add(JG.nsplit > 1 ? 2048 * (size_t)JG.nsplit * (size_t)JG.ntile : 0), o_G = L.add(2048 * (size_t)JG.ntile),
               o_sl = L.add(8 * n), o_ca = L.add(4 * n), o_cb = L.add(inter ? 24 * n : 4 * n),
               o_pc = L.add(inter && inter->peer_cov ? 72 * n * n : 0), o_cm = L.add(24 * n), o_ci = L.add(48 * n),
               o_d2 = L.add(8 * n * n), o_adj = L.add(8 * n * W);
  const CliqueLayout CL(L, nC, ex && want_clique);
  rc = call.stage();
  if (rc) return rc;
  char* d = call.d;
  HIP_TRY(ctx, hipMemcpyAsync(d + ML.o_qc, qcol.data(), 4 * (size_t)nU, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_sl, sl.data(), 8 * n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ca, ca, 4 * n, hipMemcpyHostToDevice, st));
  if (!inter) HIP_TRY(ctx, hipMemcpyAsync(d + o_cb, cb, 4 * n, hipMemcpyHostToDevice, st));
  if (inter) HIP_TRY(ctx, hipMemcpyAsync(d + o_cb, inter->peer_pose, 24 * n, hipMemcpyHostToDevice, st));
  if (inter && inter->peer_cov) HIP_TRY(ctx, hipMemcpyAsync(d + o_pc, inter->peer_cov, 72 * n * n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_cm, cmeas, 24 * n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ci, cinfo, 48 * n, hipMemcpyHostToDevice, st));
  JG.part = (double*)(d + o_part);
  JG.G = (double*)(d + o_G);
  PcmClosures C;
  C.n = nC;
  C.a = (const int32_t*)(d + o_ca); C.b = (const int32_t*)(d + o_cb); C.slot = (const int32_t*)(d + o_sl);
  C.meas = (const double*)(d + o_cm); C.info = (const double*)(d + o_ci);
  PcmInterClosures CI;
  CI.n = nC;
  CI.a = C.a; CI.slot = C.slot; CI.meas = C.meas; CI.info = C.info;
  CI.peer = (const double*)(d + o_cb);
  CI.peer_cov = inter && inter->peer_cov ? (const double*)(d + o_pc) : nullptr;
  std::vector<int32_t> res(n + 2, 0);
  int64_t total = 0;
  GnPassOpts pass;
  pass.solve = pass.update_poses = false;
  rc = call.run(pass, [&]() -> int {
    KTimer KT{ctx, st};
    if (call.factor)
      KT.run(9, 2, [&] { queue_solve_and_gram(st, D, nU, d, ML, JG); });
    KT.run(10, 1, [&] {
      if (inter) launch_closure_consistency_inter(st, CI, call.dp, JG.G, (double*)(d + o_d2));
      else launch_closure_consistency(st, C, call.dp, JG.G, (double*)(d + o_d2));
    });
    size_t o_res = CL.o_out;
    if (adj_out || want_clique)
      KT.run(11, want_clique ? (ex ? 6 + CGMR_EXACT_ROUNDS : 3) : 1, [&] {
        launch_consistency_bits(st, nC, (const double*)(d + o_d2), gamma, (unsigned long long*)(d + o_adj));
        if (want_clique) o_res = CL.launch(st, d, nC, o_adj, ex);
      });
    if (d2_out) HIP_TRY(ctx, hipMemcpyAsync(d2_out, d + o_d2, 8 * n * n, hipMemcpyDeviceToHost, st));
    if (adj_out) HIP_TRY(ctx, hipMemcpyAsync(adj_out, d + o_adj, 8 * n * W, hipMemcpyDeviceToHost, st));
    if (want_clique) HIP_TRY(ctx, hipMemcpyAsync(res.data(), d + o_res, 4 * (n + 2), hipMemcpyDeviceToHost, st));
    if (want_clique && ex) HIP_TRY(ctx, hipMemcpyAsync(&total, d + CL.o_xtotal, 8, hipMemcpyDeviceToHost, st));
    return 0;
  });
  if (ctx->profiling) profile_collect(ctx);
  if (rc) return rc;
  rc = call.close();
  if (rc == CGMR_E_CHOLESKY_BASE) {
    if (d2_out) memset(d2_out, 0, 8 * n * n);
    if (adj_out) memset(adj_out, 0, 8 * n * W);
    std::fill(res.begin(), res.end(), 0);
    total = 0;
  }
  if (want_clique && (rc == CGMR_OK || rc == CGMR_E_CHOLESKY_BASE)) clique_result_out(res, nC, clique_out, size_out, seed_out, ex, total);
  return rc;
}

// cgmr_max_clique_greedy: the clique kernels alone on a caller's adjacency words, checked on the host first.  With `ex`
// (cgmr_max_clique_exact): the exact solver's launches behind them.
int clique_driver(cgmr_ctx* ctx, int n, const uint64_t* adj, int32_t* clique_out, int32_t* size_out, int32_t* seed_out,
                  const CliqueExact* ex) {
  const char* who = ex ? "cgmr_max_clique_exact" : "cgmr_max_clique_greedy";
  if (ex) seed_out = ex->proven_out;
  if (n < 0 || !size_out || (n > 0 && (!adj || !clique_out || !seed_out))) return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", who);
  if (n > CGMR_PCM_MAX_CLOSURES) return set_err(ctx, CGMR_E_INVALID, "%s: %d vertices, at most CGMR_PCM_MAX_CLOSURES = %d", who, n, CGMR_PCM_MAX_CLOSURES);
  if (ex && ex->node_limit <= 0) return set_err(ctx, CGMR_E_INVALID, "%s: node_limit must be > 0", who);
  if (n == 0) { *size_out = 0; return CGMR_OK; }
  const int W = (n + 63) / 64;
  auto bit = [&](int k, int l) { return (int)((adj[(size_t)k * W + (l >> 6)] >> (l & 63)) & 1u); };
  for (int k = 0; k < n; k++) {
    if (bit(k, k)) return set_err(ctx, CGMR_E_INVALID, "%s: word %d: vertex %d is adjacent to itself", who, k * W + (k >> 6), k);
    if ((n & 63) && (adj[(size_t)k * W + W - 1] >> (n & 63)))
      return set_err(ctx, CGMR_E_INVALID, "%s: word %d: a padding bit (column >= %d) of row %d is set", who, k * W + W - 1, n, k);
    for (int l = 0; l < k; l++)
      if (bit(k, l) != bit(l, k))
        return set_err(ctx, CGMR_E_INVALID, "%s: word %d: bit (%d, %d) differs from bit (%d, %d)", who, k * W + (l >> 6), k, l, l, k);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Layout256 L;
  const size_t o_adj = L.add(8 * (size_t)n * W);
  const CliqueLayout CL(L, n, ex != nullptr);
  int rc = arena_reserve(ctx, ctx->io_arena, L.off + 256);
  if (rc) return rc;
  char* d = ctx->io_arena.ptr;
  hipStream_t st = ctx->stream;
  std::vector<int32_t> res((size_t)n + 2, 0);
  HIP_TRY(ctx, hipMemcpyAsync(d + o_adj, adj, 8 * (size_t)n * W, hipMemcpyHostToDevice, st));
  KTimer KT{ctx, st};
  size_t o_res = CL.o_out;
  int64_t total = 0;
  KT.run(11, ex ? 5 + CGMR_EXACT_ROUNDS : 2, [&] { o_res = CL.launch(st, d, n, o_adj, ex); });
  HIP_TRY(ctx, hipMemcpyAsync(res.data(), d + o_res, 4 * ((size_t)n + 2), hipMemcpyDeviceToHost, st));
  if (ex) HIP_TRY(ctx, hipMemcpyAsync(&total, d + CL.o_xtotal, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipGetLastError());
  if (ctx->profiling) profile_collect(ctx);
  clique_result_out(res, n, clique_out, size_out, seed_out, ex, total);
  return CGMR_OK;
}

// cgmr_condense_tree: the front half of marginal_driver's mode 2 (the gauge fixed, the spanning-tree guess, one pass with the
// step solved and applied), the solve half and the dense Gram half of joint_driver's mode 0 over the nq unique requested
// vertices, then the kernels of condense_tree_kernels.hip on the tiles where they lie: the weight of every pair of nodes, the
// minimum spanning tree from the gauge (in profiling mode in class 11, as cgmr_min_spanning_tree's) and the label of every
// tree edge at the poses after the step.
int condense_tree_driver(cgmr_ctx* ctx, const HostCall& c, int gauge, int nK, const int32_t* query, int32_t* from_out,
                         int32_t* to_out, double* est_out, double* info_out, double* weight_out, int32_t* flags_out) {
  const char* who = "cgmr_condense_tree";
  MargCall call(ctx, c);
  int rc = call.args(nK < 0 || (nK > 0 && (!query || !from_out || !to_out || !est_out || !info_out)), who);
  if (rc) return rc;
  if (gauge < 0 || gauge >= c.nV) return set_err(ctx, CGMR_E_INVALID, "%s: gauge index out of range", who);
  for (int k = 0; k < nK; k++)
    if (query[k] < 0 || query[k] >= c.nV) return set_err(ctx, CGMR_E_INVALID, "%s: query index out of range", who);
  // the nodes: the gauge, then the unique requested vertices other than it, in order of first appearance
  std::vector<int32_t> vert(1, gauge);
  {
    std::vector<uint8_t> seen(c.nV, 0);
    seen[gauge] = 1;
    for (int k = 0; k < nK; k++)
      if (!seen[query[k]]) { seen[query[k]] = 1; vert.push_back(query[k]); }
  }
  const int n = (int)vert.size(), nq = n - 1;
  if (n > CGMR_TREE_MAX_NODES)
    return set_err(ctx, CGMR_E_INVALID, "%s: %d nodes (the gauge and %d requested vertices), at most CGMR_TREE_MAX_NODES = %d", who, n, nq,
                   CGMR_TREE_MAX_NODES);
  rc = call.open(who);
  if (rc) return rc;
  std::vector<uint8_t> fixed(c.nV, 0);
  gauge_guess(call, gauge, fixed);
  rc = call.structure(fixed.data());
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  if (D.nf == 0 || nq == 0) { HIP_TRY(ctx, hipStreamSynchronize(st)); return 0; }
  const std::vector<int32_t> q(vert.begin() + 1, vert.end());
  const std::vector<int32_t> qcol = query_columns(ctx, q);
  std::vector<int32_t> slot(n, -1);                                // (node 0, the gauge: zero rows of Sigma)
  for (int k = 0; k < nq; k++) slot[k + 1] = qcol[k] < 0 ? -1 : k;
  // staging: poses | meas | info | query columns, Y, border vectors, the edges' estimates, information and flags, live flags
  // (MargLayout) | partial tiles | tiles | node vertices | node slots | weights | parents | chosen weights
  Layout256& L = call.L;
  const MargLayout ML(nq, D.nf, S.rows.size(), D.nfronts, L.off);
  L.off = ML.end;
  JointGram JG;
  dense_gram_plan(ML, JG);
  const size_t o_part = L.add(JG.nsplit > 1 ? 2048 * (size_t)JG.nsplit * (size_t)JG.ntile : 0), o_G = L.add(2048 * (size_t)JG.ntile),
               o_nv = L.add(4 * (size_t)n), o_ns = L.add(4 * (size_t)n), o_W = L.add(8 * (size_t)n * n), o_par = L.add(4 * (size_t)n),
               o_ws = L.add(8 * (size_t)n);
  rc = call.stage();
  if (rc) return rc;
  char* d = call.d;
  HIP_TRY(ctx, hipMemcpyAsync(d + ML.o_qc, qcol.data(), 4 * (size_t)nq, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_nv, vert.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ns, slot.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
  JG.part = (double*)(d + o_part);
  JG.G = (double*)(d + o_G);
  TreeNodes N;
  N.n = n;
  N.vert = (const int32_t*)(d + o_nv); N.slot = (const int32_t*)(d + o_ns);
  std::vector<int32_t> parent(n), flags(nq);
  std::vector<double> wsel(n);
  GnPassOpts pass;
  pass.solve = pass.update_poses = true;
  rc = call.run(pass, [&]() -> int {
    KTimer KT{ctx, st};
    queue_solve_and_gram(st, D, nq, d, ML, JG);
    launch_tree_weights(st, N, call.dp, JG.G, (double*)(d + o_W));
    KT.run(11, 1, [&] { launch_min_spanning_tree(st, n, (const double*)(d + o_W), 0, (int32_t*)(d + o_par), (double*)(d + o_ws)); });
    launch_tree_labels(st, N, (const int32_t*)(d + o_par), (const double*)(d + o_ws), call.dp, JG.G, (double*)(d + ML.o_est),
                       (double*)(d + ML.o_info), (int32_t*)(d + ML.o_fl));
    HIP_TRY(ctx, hipMemcpyAsync(parent.data(), d + o_par, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(wsel.data(), d + o_ws, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(flags.data(), d + ML.o_fl, 4 * (size_t)nq, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(est_out, d + ML.o_est, 24 * (size_t)nq, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(info_out, d + ML.o_info, 48 * (size_t)nq, hipMemcpyDeviceToHost, st));
    return 0;
  });
  if (ctx->profiling) profile_collect(ctx);
  if (rc) return rc;
  rc = call.close();
  if (rc) return rc;
  for (int k = 0; k < nq; k++) {
    from_out[k] = vert[parent[k + 1]];
    to_out[k] = vert[k + 1];
    if (weight_out) weight_out[k] = wsel[k + 1];
    if (flags_out) flags_out[k] = flags[k];
  }
  return nq;
}

// cgmr_min_spanning_tree: k_min_spanning_tree alone on a caller's matrix.  The kernel walks whole rows: the lower triangle is
// mirrored into the upper on the way up (a NaN as +inf), so that only the lower one is ever read.
int mst_driver(cgmr_ctx* ctx, int n, const double* weights, int root, int32_t* parent_out) {
  const char* who = "cgmr_min_spanning_tree";
  if (n < 1 || !weights || !parent_out) return set_err(ctx, CGMR_E_INVALID, "%s: null or non-positive argument", who);
  if (n > CGMR_TREE_MAX_NODES) return set_err(ctx, CGMR_E_INVALID, "%s: %d nodes, at most CGMR_TREE_MAX_NODES = %d", who, n, CGMR_TREE_MAX_NODES);
  if (root < 0 || root >= n) return set_err(ctx, CGMR_E_INVALID, "%s: root %d outside [0, %d)", who, root, n);
  const size_t N = (size_t)n;
  std::vector<double> W(N * N);
  for (size_t a = 0; a < N; a++) {
    W[a * N + a] = INFINITY;
    for (size_t b = 0; b < a; b++) {
      const double w = weights[a * N + b];
      W[a * N + b] = W[b * N + a] = w == w ? w : INFINITY;
    }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Layout256 L;
  const size_t o_W = L.add(8 * N * N), o_par = L.add(4 * N), o_ws = L.add(8 * N);
  int rc = arena_reserve(ctx, ctx->io_arena, L.off + 256);
  if (rc) return rc;
  char* d = ctx->io_arena.ptr;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(d + o_W, W.data(), 8 * N * N, hipMemcpyHostToDevice, st));
  KTimer KT{ctx, st};
  KT.run(11, 1, [&] { launch_min_spanning_tree(st, n, (const double*)(d + o_W), root, (int32_t*)(d + o_par), (double*)(d + o_ws)); });
  HIP_TRY(ctx, hipMemcpyAsync(parent_out, d + o_par, 4 * N, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipGetLastError());
  if (ctx->profiling) profile_collect(ctx);
  return CGMR_OK;
}

}  // namespace cgmr
