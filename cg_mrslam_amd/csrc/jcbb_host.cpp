// The drivers of the joint-compatibility data association (include/cgmr.h: cgmr_jcbb_dense, cgmr_joint_compatibility):
// jc_dense_driver on a caller's Sigma, jc_driver on the graph's -- the pass and the solve half of joint_driver's mode 0 over
// the observing poses and the candidate landmarks, every lower Gram tile, then the kernels of jcbb_kernels.hip on the tiles
// where they lie.  Compiled with hipcc; contains no kernels.
#include "marg_call.h"
#include "jcbb_device.h"

#include <cmath>
#include <cstring>

namespace cgmr {

namespace {

// Where the search's arrays lie in a staging block, behind whatever the caller has put into L (jcbb_device.h: JcProblem,
// JcWork), and the views of them.
struct JcLayout {
  int nM, nL, nA, n;
  size_t o_slot, o_dim, o_sigma, o_R, o_gamma, o_e, o_J, o_ic, o_cand, o_ncand;
  size_t o_ga, o_gh, o_gd, o_cnt, o_dof, o_stop, o_asg, o_d2, o_nodes, o_oa, o_oh, o_od, o_on;
  JcLayout(Layout256& L, int nM_, int nL_, int nA_) : nM(nM_), nL(nL_), nA(nA_), n(3 * nA_ + 2 * nL_) {
    const size_t M = (size_t)nM, P = M * (size_t)nL, Q = CGMR_JC_ROUNDS * P, N = (size_t)n;
    o_slot = L.add(4 * M); o_dim = L.add(4 * M); o_sigma = L.add(8 * N * N); o_R = L.add(24 * M); o_gamma = L.add(8 * (2 * M + 1));
    o_e = L.add(16 * P); o_J = L.add(80 * P); o_ic = L.add(8 * P); o_cand = L.add(4 * P); o_ncand = L.add(4 * M);
    o_ga = L.add(4 * M); o_gh = L.add(16); o_gd = L.add(8);
    o_cnt = L.add(4 * Q); o_dof = L.add(4 * Q); o_stop = L.add(4 * Q); o_asg = L.add(4 * Q * M); o_d2 = L.add(8 * Q); o_nodes = L.add(8 * Q);
    o_oa = L.add(4 * M); o_oh = L.add(16); o_od = L.add(8); o_on = L.add(8);
  }
  JcProblem problem(char* d) const {
    JcProblem P;
    P.nM = nM; P.nL = nL; P.nA = nA; P.n = n;
    P.slot = (const int32_t*)(d + o_slot); P.dim = (const int32_t*)(d + o_dim);
    P.sigma = (const double*)(d + o_sigma); P.R = (const double*)(d + o_R); P.gamma = (const double*)(d + o_gamma);
    P.e = (double*)(d + o_e); P.J = (double*)(d + o_J); P.ic = (double*)(d + o_ic);
    P.cand = (int32_t*)(d + o_cand); P.ncand = (int32_t*)(d + o_ncand);
    return P;
  }
  JcWork work(char* d) const {
    JcWork X;
    X.g_assign = (int32_t*)(d + o_ga); X.g_head = (int32_t*)(d + o_gh); X.g_d2 = (double*)(d + o_gd);
    X.count = (int32_t*)(d + o_cnt); X.dof = (int32_t*)(d + o_dof); X.stopped = (int32_t*)(d + o_stop);
    X.assign = (int32_t*)(d + o_asg); X.d2 = (double*)(d + o_d2); X.nodes = (long long*)(d + o_nodes);
    X.out_assign = (int32_t*)(d + o_oa); X.out_head = (int32_t*)(d + o_oh); X.out_d2 = (double*)(d + o_od);
    X.out_nodes = (long long*)(d + o_on);
    return X;
  }
};

// what comes back from the device, and where it goes once the stream has been waited for
struct JcResult {
  std::vector<int32_t> assign;
  int32_t head[4] = {0, 0, 1, 0};
  double d2 = 0;
  int64_t nodes = 0;
  explicit JcResult(int nM) : assign((size_t)nM, -1) {}
  void zero() { std::fill(assign.begin(), assign.end(), -1); head[0] = head[1] = 0; head[2] = 1; d2 = 0; nodes = 0; }
  // lm: the candidates' vertex indices (null: positions stay positions)
  void out(const JcOut& o, const int32_t* lm) const {
    for (size_t i = 0; i < assign.size(); i++) o.assign[i] = assign[i] < 0 ? -1 : (lm ? lm[assign[i]] : assign[i]);
    *o.count = head[0]; *o.dof = head[1]; *o.proven = head[2]; *o.d2 = d2;
    if (o.nodes) *o.nodes = nodes;
  }
};

// the checks the two entry points share; `who` heads the text
int jc_common_checks(cgmr_ctx* ctx, const char* who, int nM, int nL, const double* gamma, int64_t node_limit, const JcOut& o) {
  if (!o.assign || !o.count || !o.d2 || !o.dof || !o.proven || (nM > 0 && !gamma))
    return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", who);
  if (nM > CGMR_JC_MAX_OBS) return set_err(ctx, CGMR_E_INVALID, "%s: %d observations, at most CGMR_JC_MAX_OBS = %d", who, nM, CGMR_JC_MAX_OBS);
  if (nL > CGMR_JC_MAX_LANDMARKS)
    return set_err(ctx, CGMR_E_INVALID, "%s: %d landmarks, at most CGMR_JC_MAX_LANDMARKS = %d", who, nL, CGMR_JC_MAX_LANDMARKS);
  if (node_limit <= 0) return set_err(ctx, CGMR_E_INVALID, "%s: node_limit must be > 0", who);
  for (int k = 1; k <= 2 * nM; k++)
    if (!std::isfinite(gamma[k]) || !(gamma[k] > (k > 1 ? gamma[k - 1] : 0.0)))
      return set_err(ctx, CGMR_E_INVALID, "%s: gamma_by_dof[%d] is not finite or not above the entry before it", who, k);
  return 0;
}

int jc_upload(cgmr_ctx* ctx, hipStream_t st, char* d, const JcLayout& JL, const int32_t* slot, const int32_t* dim, const double* R,
              const double* gamma) {
  const size_t M = (size_t)JL.nM;
  HIP_TRY(ctx, hipMemcpyAsync(d + JL.o_slot, slot, 4 * M, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + JL.o_dim, dim, 4 * M, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + JL.o_R, R, 24 * M, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + JL.o_gamma, gamma, 8 * (2 * M + 1), hipMemcpyHostToDevice, st));
  return 0;
}

int jc_download(cgmr_ctx* ctx, hipStream_t st, const char* d, const JcLayout& JL, JcResult& res, double* ic_out) {
  const size_t M = (size_t)JL.nM;
  if (ic_out) HIP_TRY(ctx, hipMemcpyAsync(ic_out, d + JL.o_ic, 8 * M * (size_t)JL.nL, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(res.assign.data(), d + JL.o_oa, 4 * M, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(res.head, d + JL.o_oh, 12, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&res.d2, d + JL.o_od, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&res.nodes, d + JL.o_on, 8, hipMemcpyDeviceToHost, st));
  return 0;
}

}  // namespace

int jc_dense_driver(cgmr_ctx* ctx, int nM, int nL, int nA, const int32_t* slot, const int32_t* dim, const double* sigma,
                    const double* e, const double* J, const double* R, const double* gamma, int64_t node_limit, const JcOut& out) {
  const char* who = "cgmr_jcbb_dense";
  if (!ctx) return CGMR_E_INVALID;
  if (nM < 0 || nL < 0 || nA < 0 || (nM > 0 && (!slot || !dim || !R)) || (nM > 0 && nL > 0 && (!sigma || !e || !J)))
    return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", who);
  int rc = jc_common_checks(ctx, who, nM, nL, gamma, node_limit, out);
  if (rc) return rc;
  if (nA > CGMR_JC_MAX_OBS) return set_err(ctx, CGMR_E_INVALID, "%s: %d observing poses, at most CGMR_JC_MAX_OBS = %d", who, nA, CGMR_JC_MAX_OBS);
  for (int i = 0; i < nM; i++) {
    if (dim[i] != 1 && dim[i] != 2) return set_err(ctx, CGMR_E_INVALID, "%s: observation %d has dimension %d (1 or 2)", who, i, dim[i]);
    if (slot[i] < 0 || slot[i] >= nA) return set_err(ctx, CGMR_E_INVALID, "%s: observation %d has pose slot %d, outside [0, %d)", who, i, slot[i], nA);
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(R[3 * (size_t)i + k])) return set_err(ctx, CGMR_E_INVALID, "%s: observation %d has an R that is not finite", who, i);
  }
  JcResult res(nM);
  if (nM == 0 || nL == 0) { res.out(out, nullptr); return CGMR_OK; }
  const size_t n = 3 * (size_t)nA + 2 * (size_t)nL;
  for (size_t r = 0; r < n; r++)                                    // the lower triangle is all that is read
    for (size_t q = 0; q <= r; q++)
      if (!std::isfinite(sigma[r * n + q])) {
        const size_t k = r < 3 * (size_t)nA ? r / 3 : (r - 3 * (size_t)nA) / 2;
        return set_err(ctx, CGMR_E_INVALID, "%s: sigma (%zu, %zu), %s %zu, is not finite", who, r, q, r < 3 * (size_t)nA ? "pose" : "landmark", k);
      }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Layout256 L;
  const JcLayout JL(L, nM, nL, nA);
  rc = arena_reserve(ctx, ctx->io_arena, L.off + 256);
  if (rc) return rc;
  char* d = ctx->io_arena.ptr;
  hipStream_t st = ctx->stream;
  const size_t P = (size_t)nM * nL;
  rc = jc_upload(ctx, st, d, JL, slot, dim, R, gamma);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d + JL.o_sigma, sigma, 8 * n * n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + JL.o_e, e, 16 * P, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + JL.o_J, J, 80 * P, hipMemcpyHostToDevice, st));
  launch_jc(st, JL.problem(d), JcPredict(), node_limit, JL.work(d));
  rc = jc_download(ctx, st, d, JL, res, out.ic);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipGetLastError());
  res.out(out, nullptr);
  return CGMR_OK;
}

int jc_driver(cgmr_ctx* ctx, const HostCall& c, int nM, const int32_t* obs_pose, const uint8_t* obs_kind, const double* obs_meas,
              const double* obs_info, int nL, const int32_t* lm, const double* gamma, int64_t node_limit, const JcOut& out) {
  const char* who = "cgmr_joint_compatibility";
  MargCall call(ctx, c);
  int rc = call.args(nM < 0 || nL < 0 || !c.fixed || (nM > 0 && (!obs_pose || !obs_kind || !obs_meas)) || (nL > 0 && !lm), who);
  if (rc) return rc;
  rc = jc_common_checks(ctx, who, nM, nL, gamma, node_limit, out);
  if (rc) return rc;
  for (int i = 0; i < nM; i++) {
    if (obs_pose[i] < 0 || obs_pose[i] >= c.nV)
      return set_err(ctx, CGMR_E_INVALID, "%s: observation %d is made from vertex %d, outside [0, %d)", who, i, obs_pose[i], c.nV);
    if (obs_kind[i] != CGMR_EDGE_SE2_XY && obs_kind[i] != CGMR_EDGE_BEARING_SE2_XY)
      return set_err(ctx, CGMR_E_INVALID, "%s: observation %d has kind %d (1 or 2)", who, i, (int)obs_kind[i]);
  }
  for (int j = 0; j < nL; j++)
    if (lm[j] < 0 || lm[j] >= c.nV) return set_err(ctx, CGMR_E_INVALID, "%s: landmark %d is vertex %d, outside [0, %d)", who, j, lm[j], c.nV);
  rc = call.types(who);
  if (rc) return rc;
  const TypedHost& typed = call.typed;
  auto is_point = [&](int v) { return c.ft && !typed.vk.empty() && typed.vk[v] != 0; };
  for (int i = 0; i < nM; i++)
    if (is_point(obs_pose[i])) return set_err(ctx, CGMR_E_INVALID, "%s: observation %d is made from vertex %d, a point", who, i, obs_pose[i]);
  // the state: the unique observing poses in order of first appearance, then the candidates; 4 columns of Y each
  std::vector<int32_t> slot_of(c.nV, -1), uq, slot(nM), dim(nM);
  for (int i = 0; i < nM; i++) {
    if (slot_of[obs_pose[i]] < 0) { slot_of[obs_pose[i]] = (int32_t)uq.size(); uq.push_back(obs_pose[i]); }
    slot[i] = slot_of[obs_pose[i]];
    dim[i] = obs_kind[i] == CGMR_EDGE_SE2_XY ? 2 : 1;
  }
  const int nA = (int)uq.size();
  for (int j = 0; j < nL; j++) {
    if (!is_point(lm[j])) return set_err(ctx, CGMR_E_INVALID, "%s: landmark %d is vertex %d, a pose", who, j, lm[j]);
    if (slot_of[lm[j]] >= 0) return set_err(ctx, CGMR_E_INVALID, "%s: landmark %d repeats vertex %d", who, j, lm[j]);
    slot_of[lm[j]] = (int32_t)uq.size();
    uq.push_back(lm[j]);
  }
  const int nU = (int)uq.size();
  if (nU > CGMR_JOINT_MAX_QUERIES)
    return set_err(ctx, CGMR_E_INVALID, "%s: %d unique vertices, at most CGMR_JOINT_MAX_QUERIES = %d", who, nU, CGMR_JOINT_MAX_QUERIES);
  JcResult res(nM);
  if (nM == 0 || nL == 0) { res.out(out, nullptr); return CGMR_OK; }
  // R = Omega^-1 as k_observation_cov forms it
  std::vector<double> R(3 * (size_t)nM, 0.0);
  for (int i = 0; i < nM && obs_info; i++) {
    const double* iu = obs_info + 6 * (size_t)i;
    if (dim[i] == 2) {
      const double a = iu[0], b = iu[1], dd = iu[3];
      const double id = 1.0 / (a * dd - b * b);
      R[3 * (size_t)i] = dd * id; R[3 * (size_t)i + 1] = -(b * id); R[3 * (size_t)i + 2] = a * id;
    } else {
      R[3 * (size_t)i] = 1.0 / iu[0];
    }
  }
  rc = call.open(who);
  if (rc) return rc;
  rc = call.structure(c.fixed);
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  call.factor = D.nf > 0;                                          // no free vertex: Sigma = 0, the measurement terms alone
  const MargLayout M(nU, D.nf, S.rows.size(), D.nfronts, 0);
  const int T = M.m / 16;
  std::vector<int32_t> qcol(nU);
  for (int k = 0; k < nU; k++) qcol[k] = ctx->vmask[uq[k]] ? -1 : S.vperm[uq[k]];      // fixed / inactive: zero columns
  std::vector<int32_t> col(3 * (size_t)nA + 2 * (size_t)nL);
  for (int k = 0; k < nA; k++)
    for (int q = 0; q < 3; q++) col[3 * (size_t)k + q] = qcol[k] < 0 ? -1 : 4 * k + q;
  for (int j = 0; j < nL; j++)
    for (int q = 0; q < 2; q++) col[3 * (size_t)nA + 2 * (size_t)j + q] = qcol[nA + j] < 0 ? -1 : 4 * (nA + j) + q;
  JointGram JG;
  JG.ntile = (long long)T * (T + 1) / 2;
  joint_gram_split(M.n, (long long)((T + 3) / 4) * ((T + 3) / 4 + 1) / 2, &JG.rows, &JG.nsplit);
  // staging: poses | meas | info | query columns, Y, border vectors, live flags (MargLayout) | partial tiles | tiles | the
  // observations and candidates | the state's columns | the search's arrays
  Layout256& L = call.L;
  const MargLayout ML(nU, D.nf, S.rows.size(), D.nfronts, L.off);
  L.off = ML.end;
  const size_t o_part = L.add(JG.nsplit > 1 ? 2048 * (size_t)JG.nsplit * (size_t)JG.ntile : 0), o_G = L.add(2048 * (size_t)JG.ntile),
               o_op = L.add(4 * (size_t)nM), o_lm = L.add(4 * (size_t)nL), o_om = L.add(24 * (size_t)nM), o_col = L.add(4 * col.size());
  const JcLayout JL(L, nM, nL, nA);
  rc = call.stage();
  if (rc) return rc;
  char* d = call.d;
  HIP_TRY(ctx, hipMemcpyAsync(d + ML.o_qc, qcol.data(), 4 * (size_t)nU, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_op, obs_pose, 4 * (size_t)nM, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_lm, lm, 4 * (size_t)nL, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_om, obs_meas, 24 * (size_t)nM, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_col, col.data(), 4 * col.size(), hipMemcpyHostToDevice, st));
  rc = jc_upload(ctx, st, d, JL, slot.data(), dim.data(), R.data(), gamma);
  if (rc) return rc;
  JG.part = (double*)(d + o_part);
  JG.G = (double*)(d + o_G);
  JcPredict G;
  G.obs_pose = (const int32_t*)(d + o_op); G.lm = (const int32_t*)(d + o_lm); G.meas = (const double*)(d + o_om);
  GnPassOpts pass;
  pass.solve = pass.update_poses = false;
  rc = call.run(pass, [&]() -> int {
    if (call.factor) {
      launch_marginals_solve(st, D, nU, (const int32_t*)(d + ML.o_qc), ML.m, (double*)(d + ML.o_Y), (double*)(d + ML.o_U),
                             (uint8_t*)(d + ML.o_live));
      launch_joint_gram(st, ML.n, ML.m, (const double*)(d + ML.o_Y), JG);
      launch_jc_sigma(st, JL.n, (const int32_t*)(d + o_col), JG.G, (double*)(d + JL.o_sigma));
    } else {
      HIP_TRY(ctx, hipMemsetAsync(d + JL.o_sigma, 0, 8 * (size_t)JL.n * JL.n, st));
    }
    G.poses = call.dp;
    launch_jc(st, JL.problem(d), G, node_limit, JL.work(d));
    return jc_download(ctx, st, d, JL, res, out.ic);
  });
  if (ctx->profiling) profile_collect(ctx);                        // (the pass's launch classes; the search has none of its own)
  if (rc) return rc;
  rc = call.close();
  if (rc == CGMR_E_CHOLESKY_BASE) {
    if (out.ic) memset(out.ic, 0, 8 * (size_t)nM * nL);
    res.zero();
    res.head[2] = 0;
  }
  if (rc == CGMR_OK || rc == CGMR_E_CHOLESKY_BASE) res.out(out, lm);
  return rc;
}

}  // namespace cgmr
