// The robot graph's condensed graphs (include/cgmr.h: cgmr_graph_compute_condensed*, _condensed_wait, _get / _set_condensed):
// gauge selection, one batch of passes for all peers, how a batch ends.  Reference behaviour being replaced:
//   CondensedGraphBuffer::selectGaugeCentroid / computeCondensedGraph   condensed_graph_buffer.cpp:318-345, 437-485
//   CondensedGraphCreator::compute                                       condensed_graph_creator.cpp:33-66
#include "robot_graph.h"

using namespace cgmr;

namespace {

// The stored GNC weights as a condensed pass takes them (cgmr_graph_set_condensed_gnc): below drop_below, or zero, the edge is
// removed (0); the others keep their weight.
std::vector<double> cond_gnc_weights(const cgmr_graph* g) {
  std::vector<double> w(g->gnc_w);
  for (double& x : w) if (x < g->cond_drop_below || x == 0.0) x = 0.0;
  return w;
}

// SparseOptimizer::computeInitialGuess from ONE fixed vertex over the own edges (gn_host.h: initial_guess_host is the
// general form): breadth-first from `root`, edges in list order, x_to = x_from * z or x_from = x_to * z^-1.  Walks the
// graph's incidence lists and takes cos / sin of the measurements from the cache; the orientation of a reached vertex is
// carried along as (cos, sin) by the angle-addition formulas (a round's six or seven guesses were 0.17-0.24 ms of its
// 0.4 ms of host work: two libm calls per vertex and edge direction).  The guess differs from the all-libm form by rounding;
// the ONE Gauss-Newton iteration that follows starts far from the optimum and amplifies any rounding difference of its
// linearisation point by cond(H): the condensed measurements of the two forms agree to ~1e-8 m (libm again every eighth
// tree level did not change that: it is not drift), well inside the 1e-6 parity bar against the oracle.
// wt (nullable): per own edge its weight in the pass that follows -- an edge of weight 0 is not in that pass's graph and is
// not walked (a rejected closure would carry half the tree to a wrong place); a vertex the tree then misses keeps its estimate.
void initial_guess_own_edges(const cgmr_graph* g, int root, double* poses, std::vector<int32_t>& queue, std::vector<double>& cs,
                             std::vector<uint8_t>& seen, const double* wt = nullptr) {
  const int nV = (int)g->ids.size();
  const double pi = 3.14159265358979323846;
  seen.assign(nV, 0);
  cs.resize(2 * (size_t)nV);
  queue.clear();
  if (g->adj_head[root] < 0) return;
  seen[root] = 1;
  queue.push_back(root);
  cs[2 * (size_t)root] = std::cos(poses[3 * (size_t)root + 2]);
  cs[2 * (size_t)root + 1] = std::sin(poses[3 * (size_t)root + 2]);
  for (size_t qh = 0; qh < queue.size(); qh++) {
    const int u = queue[qh];
    const double* a = poses + 3 * (size_t)u;
    const double cu = cs[2 * (size_t)u], su = cs[2 * (size_t)u + 1];
    for (int32_t it = g->adj_head[u]; it >= 0; it = g->adj_next[it]) {
      const int k = it >> 1;
      if (wt && wt[k] == 0.0) continue;
      const int w = (g->ef[k] == u) ? g->et[k] : g->ef[k];
      if (seen[w]) continue;
      seen[w] = 1;
      const double* m = g->h_meas.data() + 3 * (size_t)k;
      double zx = m[0], zy = m[1], zt = m[2], cz = g->e_cs[2 * (size_t)k], sz = g->e_cs[2 * (size_t)k + 1];
      if (g->ef[k] != u) {                                       // z^-1
        const double ix = -(cz * zx + sz * zy), iy = -(-sz * zx + cz * zy);
        zx = ix; zy = iy; zt = -zt; sz = -sz;
      }
      double* o = poses + 3 * (size_t)w;
      o[0] = a[0] + cu * zx - su * zy;
      o[1] = a[1] + su * zx + cu * zy;
      const double t = a[2] + zt;
      o[2] = (t >= -pi && t < pi) ? t : t - 2 * pi * std::floor((t + pi) / (2 * pi));
      cs[2 * (size_t)w] = cu * cz - su * sz;
      cs[2 * (size_t)w + 1] = su * cz + cu * sz;
      queue.push_back(w);
    }
  }
}

// How a batch of nj jobs ended, from its status words (4 per job): a pass failed; a bounded device-side wait ran out.
struct BatchStatus { bool failed = false, timed_out = false; };
BatchStatus batch_status(const int32_t* status, size_t nj) {
  BatchStatus s;
  for (size_t j = 0; j < nj; j++) { s.failed = s.failed || status[4 * j] != 0; s.timed_out = s.timed_out || status[4 * j + 2] != 0; }
  return s;
}
// the outcome of a batch (0, CGMR_E_TIMEOUT or CGMR_E_CHOLESKY_BASE) as the graph's error
int batch_outcome(cgmr_graph* g, int code) {
  if (code == CGMR_E_TIMEOUT) return gerr(g, code, "a bounded device-side wait ran out while building a condensed graph");
  return code ? gerr(g, code, "Cholesky failed while building a condensed graph") : 0;
}

// Finish the pending asynchronous batch: wait for it, look at the status words.  A failed pass leaves nothing to send to any
// peer of the batch (as the synchronous call does); the header of a message packed meanwhile was corrected on the device.
int cond_finish(cgmr_graph* g) {
  if (!g->cond_pending) return 0;
  cgmr_ctx* ctx = g->ctx;
  g->cond_pending = false;
  HIP_TRY(ctx, hipEventSynchronize(g->ev_cond_done));
  const BatchStatus s = batch_status(g->cond_status, g->cond_peers.size());
  g->cond_last_rc = 0;
  if (!s.failed) return 0;
  for (int32_t p : g->cond_peers) { g->out[p].n = 0; g->out[p].host_valid = false; }
  g->cond_failed_batches++;
  if (s.timed_out) { g->cond_levelwise = true; count_timeout(ctx); }
  return g->cond_last_rc = batch_outcome(g, s.timed_out ? CGMR_E_TIMEOUT : CGMR_E_CHOLESKY_BASE);
}

}  // namespace

namespace cgmr {

int finish_pending(cgmr_graph* g, bool tolerate_failed_batch) {
  if (!g->ctx || !g->cond_pending) return 0;
  if (int rc = graph_device(g)) return rc;
  const int rc = cond_finish(g);
  return tolerate_failed_batch && (rc == CGMR_E_TIMEOUT || rc == CGMR_E_CHOLESKY_BASE) ? 0 : rc;    // (a HIP error still stops)
}

}  // namespace cgmr

namespace {

// selectGaugeCentroid (condensed_graph_buffer.cpp:318-345): the vertex closest to the centroid of the requested
// vertices' translations, first one (id order) wins ties
int select_gauge_centroid(const std::vector<int32_t>& idx, const double* poses) {
  double sx = 0, sy = 0;
  for (int v : idx) { sx += poses[3 * (size_t)v]; sy += poses[3 * (size_t)v + 1]; }
  const double cx = sx / (double)idx.size(), cy = sy / (double)idx.size();
  int best = -1;
  double bd = 1.79769313486231570815e308;
  for (int v : idx) {
    const double dx = poses[3 * (size_t)v] - cx, dy = poses[3 * (size_t)v + 1] - cy;
    const double d = std::sqrt(dx * dx + dy * dy);
    if (d < bd) { bd = d; best = v; }
  }
  return best;
}

struct CondJob {
  int peer = 0;
  int gauge = 0;                      // vertex index
  std::vector<int32_t> q;             // the other requested vertices (vertex indices, id order)
};

// The staging block of a batch of nj jobs: masks | initial guesses | query columns | query vertices | job descriptors | the
// snapshot of the own edges' GNC weights (nw of them; cgmr_graph_set_condensed_gnc, else none) go up in one copy from pinned
// memory (the first s_st bytes); the status words (4 per job) come back behind them.
struct CondStage {
  size_t s_work = 0, s_qc = 0, s_qv = 0, s_jd = 0, s_w = 0, s_st = 0, s_end = 0;
  CondStage() = default;
  CondStage(int nj, int nf, int nV, int maxq, size_t nw) {
    Layout256 L;
    L.add((size_t)nf * nj);                                      // (the masks: offset 0)
    s_work = L.add((size_t)24 * nV * nj); s_qc = L.add((size_t)4 * maxq * nj); s_qv = L.add((size_t)4 * maxq * nj);
    s_jd = L.add(sizeof(CondJobDev) * (size_t)nj); s_w = L.add(8 * nw); s_st = L.add(16 * (size_t)nj);
    s_end = L.off;
  }
};

// One batch of condensed-graph passes on its way through run_cond_jobs' phases.
struct CondBatch {
  cgmr_graph* g;
  cgmr_ctx* ctx;
  std::vector<CondJob>& jobs;
  bool to_wire;
  int nV, nA, nE = 0, nj, nf = 0, maxq = 1;
  const int32_t *s_ef = nullptr, *s_et = nullptr;   // the edge list the structure was analysed for (own edges first)
  hipStream_t st = nullptr;           // the context's stream, or its side stream for a batch that is not waited for
  GnDevice DB;                        // the batch's view: job 0's, job j moved by j * DB.job_stride
  GnEdges Ed;
  // cgmr_graph_set_condensed_gnc: the stored weights as they are when the batch is queued, thresholded (cond_gnc_weights) -- the
  // snapshot the guesses walk and the passes read from the staging block, whatever a later cgmr_graph_optimize_gnc stores
  bool use_w = false;
  std::vector<double> wt;
  MargLayout M;                       // one job's marginals work space; job j: moved by j * per_job
  size_t per_job = 0;
  CondStage S;
  char *hstage = nullptr, *d0 = nullptr, *ds = nullptr;   // the staging block in pinned memory; on the device: job 0's marginals work space, the staging block's copy behind the jobs'
  // CGMR_COND_TRACE: host seconds of the phases, device events around the pass / the marginals / the labels
  bool trace = false;
  double t0 = 0, t_structure = 0, t_space = 0, t_guess = 0, t_mask = 0, t_up = 0, t_gn = 0, t_marg = 0;
  hipEvent_t evs[4] = {nullptr, nullptr, nullptr, nullptr};

  CondBatch(cgmr_graph* g_, std::vector<CondJob>& j, bool w)
      : g(g_), ctx(g_->ctx), jobs(j), to_wire(w), nV((int)g_->ids.size()), nA((int)g_->ef.size()), nj((int)j.size()) {}
  CondBatch(const CondBatch&) = delete;
  ~CondBatch() { for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e); }
  void mark(int k) { if (trace) (void)hipEventRecord(evs[k], st); }
};

// Structure, work space and edge description of the batch: one symbolic analysis (shared with cgmr_graph_optimize: same edge
// list) serves all jobs -- the gauge and the switched-off received edges are numeric masks --, every job gets a copy of the
// numeric work space and a marginals work space sized for the largest query set; the staging block lies behind them.
int cond_setup(CondBatch& B) {
  cgmr_graph* g = B.g;
  cgmr_ctx* ctx = B.ctx;
  // the edge list the structure is analysed for: the last solve's if nothing of mine has changed since (a hit in the
  // analysis cache; own edges are only ever appended, so equal counts mean equal lists), else the current one
  const bool reuse = g->solved_nV == B.nV && g->solved_nA == B.nA && (int)g->solved_ef.size() >= B.nA;
  const std::vector<int32_t>& s_ef = reuse ? g->solved_ef : g->all_ef;
  const std::vector<int32_t>& s_et = reuse ? g->solved_et : g->all_et;
  B.nE = (int)s_ef.size();
  B.s_ef = s_ef.data(); B.s_et = s_et.data();
  int rc = prepare_structure(ctx, B.nV, B.nE, s_ef.data(), s_et.data(), 1);
  if (rc) return rc;
  const double t1 = wall_s();
  B.t_structure = t1 - B.t0;
  B.nf = ctx->gn.nf;
  const size_t rep_cap0 = ctx->rep_arena.cap, mg_cap0 = ctx->mg_arena.cap;
  size_t rep_stride = 0;
  rc = gn_replicas(ctx, B.nj, B.DB, &rep_stride);
  if (rc) return rc;
  B.DB.njobs = B.nj; B.DB.job_stride = (long long)rep_stride; B.DB.pose_stride = 24LL * B.nV;
  const double t1a = wall_s();
  for (CondJob& J : B.jobs) B.maxq = std::max(B.maxq, (int)J.q.size());
  B.M = MargLayout(B.maxq, B.nf, ctx->sym.rows.size(), ctx->gn.nfronts, 0, /*flags_first=*/true);
  B.per_job = round256(B.M.end);
  B.use_w = g->cond_gnc;
  if (B.use_w) B.wt = cond_gnc_weights(g);
  B.S = CondStage(B.nj, B.nf, B.nV, B.maxq, B.wt.size());
  rc = arena_reserve(ctx, ctx->mg_arena, B.per_job * (size_t)B.nj + B.S.s_end + 256);
  if (rc) return rc;
  B.d0 = ctx->mg_arena.ptr;
  B.ds = B.d0 + B.per_job * (size_t)B.nj;
  const double t1b = wall_s();                                   // (work space: allocations when something grew)
  B.t_space = t1b - t1;
  if (B.trace && t1b - t1 > 300e-6)
    fprintf(stderr, "[cond]   work space: replicas %.0f us (%zu -> %zu MB), marginals arena %.0f us (%zu -> %zu MB)\n", 1e6 * (t1a - t1), rep_cap0 >> 20,
            ctx->rep_arena.cap >> 20, 1e6 * (t1b - t1a), mg_cap0 >> 20, ctx->mg_arena.cap >> 20);
  GnEdges& Ed = B.Ed;
  Ed = graph_edges(g, B.nA);                                     // getMyEdges: the received edges are switched off
  if (g->cond_robust && g->rk_dev) {  // the own edges' kernels (the received ones are switched off: their class never enters)
    Ed.robust = true;
    Ed.rk = {(const uint8_t*)g->d_rk_kind.ptr, (const double*)g->d_rk_delta.ptr, nullptr, 1.0, CGMR_RK_NONE};
  }
  if (B.use_w) {                      // the own edges' stored weights (cond_queue binds the staged snapshot)
    Ed.robust = false;
    Ed.gnc = true; Ed.gnc_own_only = true; Ed.ga.mode = kGncReuse;
  }
  return 0;
}

// The pinned staging block: the context's (the solver's mask staging -- nothing of it is in flight now) or, for a batch that is
// not waited for, the graph's own: the next solve stages its mask while this batch's copy may still be queued.
int cond_stage_block(CondBatch& B, bool go_async) {
  cgmr_graph* g = B.g;
  cgmr_ctx* ctx = B.ctx;
  if (!go_async) {
    int rc = pinned_mask_reserve(ctx, B.S.s_end);
    if (rc) return rc;
    B.hstage = ctx->pinned_mask;
    return 0;
  }
  if (B.S.s_end > g->cond_pinned_cap) {
    if (g->cond_pinned) {
      int rc = side_join_host(ctx);
      if (rc) return rc;
      (void)hipHostFree(g->cond_pinned);
      g->cond_pinned = nullptr; g->cond_pinned_cap = 0;
    }
    const size_t want = 2 * B.S.s_end + (64 << 10);              // (page-locking is slow: rarely)
    HIP_TRY(ctx, hipHostMalloc((void**)&g->cond_pinned, want, hipHostMallocDefault));
    g->cond_pinned_cap = want;
  }
  B.hstage = g->cond_pinned;
  return 0;
}

// The host's part of the batch, written straight into the staging block: every job's initial guess, column mask, query lists
// and descriptor.  The guess is GraphManipulator::fixGauge + optimize(1) (graph_manipulator.cpp:62-124): only the gauge is fixed,
// spanning-tree initial guess over my own edges with the gauge as the root (0.15-0.3 ms of host work each: on the helper threads).
void cond_fill_stage(CondBatch& B) {
  const cgmr_graph* g = B.g;
  const Symbolic& S = B.ctx->sym;
  const int nV = B.nV, nA = B.nA, nf = B.nf, maxq = B.maxq;
  char* h = B.hstage;
  const double tg0 = wall_s();
  const bool cached_walk = B.ctx->sw.guess_cached;
  // (the general form walks an edge list: the kept own edges, in their order)
  std::vector<int32_t> kept_ef, kept_et;
  std::vector<double> kept_meas;
  if (B.use_w && !cached_walk)
    for (int k = 0; k < nA; k++)
      if (B.wt[k] != 0.0) {
        kept_ef.push_back(g->ef[k]); kept_et.push_back(g->et[k]);
        kept_meas.insert(kept_meas.end(), g->h_meas.begin() + 3 * (size_t)k, g->h_meas.begin() + 3 * (size_t)k + 3);
      }
  host_run_tasks(B.nj, [&](int i) {
    double* w = (double*)(h + B.S.s_work + (size_t)24 * nV * i);
    memcpy(w, g->h_poses.data(), (size_t)24 * nV);
    if (cached_walk) {
      thread_local std::vector<int32_t> queue;
      thread_local std::vector<double> cs;
      thread_local std::vector<uint8_t> seen;
      initial_guess_own_edges(g, B.jobs[i].gauge, w, queue, cs, seen, B.use_w ? B.wt.data() : nullptr);
    } else {
      std::vector<uint8_t> fx(nV, 0);
      fx[B.jobs[i].gauge] = 1;
      if (B.use_w) initial_guess_host(nV, w, fx.data(), (int)kept_ef.size(), kept_ef.data(), kept_et.data(), kept_meas.data());
      else initial_guess_host(nV, w, fx.data(), nA, g->ef.data(), g->et.data(), g->h_meas.data());
    }
  });
  if (B.use_w && nA > 0) memcpy(h + B.S.s_w, B.wt.data(), 8 * (size_t)nA);
  const double tm0 = wall_s();
  B.t_guess = tm0 - tg0;
  // the column masks: a vertex without an own edge is out of every job's system (the received edges are switched off);
  // the jobs differ in their gauge only
  std::vector<uint8_t> live(nV, 0);
  for (int k = 0; k < nA; k++) { live[B.s_ef[k]] = 1; live[B.s_et[k]] = 1; }
  std::vector<char> base(nf);
  for (int c = 0; c < nf; c++) base[c] = live[S.perm[c]] ? 0 : 1;
  for (int i = 0; i < B.nj; i++) {
    const CondJob& J = B.jobs[i];
    char* pm = h + (size_t)nf * i;
    memcpy(pm, base.data(), (size_t)nf);
    if (S.vperm[J.gauge] >= 0) pm[S.vperm[J.gauge]] = 1;
    const int nq = (int)J.q.size();
    int32_t* qc = (int32_t*)(h + B.S.s_qc) + (size_t)maxq * i;
    int32_t* qv = (int32_t*)(h + B.S.s_qv) + (size_t)maxq * i;
    for (int k = 0; k < nq; k++) { const int q = J.q[k]; qc[k] = (q == J.gauge || !live[q]) ? -1 : S.vperm[q]; qv[k] = q; }
    CondJobDev& jd = ((CondJobDev*)(h + B.S.s_jd))[i];
    jd.nq = nq; jd.gauge = J.gauge; jd.gauge_id = g->ids[J.gauge]; jd.out_slot = B.to_wire ? J.peer : i;
  }
  B.t_mask = wall_s() - tm0;
}

// The device's part, ONE sequence of launches with a job dimension (gn_kernels.hip CGMR_JOB) -- a stream of ~65 launches per
// job side by side had the device dispatch the small kernels of 7 jobs at ~7 us apiece (3.9 ms for the condensed graphs of a
// round with 8 robots): the staging block goes up, one Gauss-Newton pass, the marginals of that pass's Hessian, the labelled
// edges (to_wire: double-precision copy in the peers' slots + 44-byte wire records in the send buffer; else in the jobs' work
// spaces), the status words back into the staging block.
int cond_queue(CondBatch& B) {
  cgmr_graph* g = B.g;
  cgmr_ctx* ctx = B.ctx;
  hipStream_t st = B.st;
  GnDevice& DB = B.DB;
  const MargLayout& M = B.M;
  const CondStage& S = B.S;
  const int nj = B.nj, maxq = B.maxq, cap = g->cap;
  char *d0 = B.d0, *ds = B.ds;
  // the chained backward solve and the merged levels need their workgroups resident together: the batch takes nj times the slots
  // (after a time-out -- two chained solves per context on eight contexts of one device make them likelier -- the batches of
  // this graph solve level by level: no in-kernel waits, like gn_run's retry)
  choose_bwd_chain(DB, (ctx->side_used ? 2 : 1) * nj, g->cond_levelwise);
  choose_fwd_merge(DB, (ctx->side_used ? 2 : 1) * nj, g->cond_levelwise, ctx->fwd_merge_any);
  const double tu0 = wall_s();
  double* d_work0 = (double*)(ds + S.s_work);                    // the passes work on the poses where they landed
  HIP_TRY(ctx, hipMemcpyAsync(ds, B.hstage, S.s_st, hipMemcpyHostToDevice, st));
  CondPrepare P;
  P.njobs = nj; P.nf = B.nf; P.maxq = maxq;
  P.stage_mask = (const uint8_t*)ds; P.stage_qc = (const int32_t*)(ds + S.s_qc); P.stage_qv = (const int32_t*)(ds + S.s_qv);
  P.cmask = DB.cmask; P.qc = (int32_t*)(d0 + M.o_qc); P.qv = (int32_t*)(d0 + M.o_qv); P.status = DB.status;
  P.pan = DB.Pan; P.pan_doubles = DB.pan_doubles; P.Y = (double*)(d0 + M.o_Y); P.y_doubles = (long long)M.n * M.m;
  P.rep_stride = DB.job_stride; P.marg_stride = (long long)B.per_job;
  launch_cond_prepare(st, P);
  DB.pan_clean = DB.pan_doubles > 0;                             // (gn_pass_on: no memset in front of the assembly)
  B.t_up = wall_s() - tu0;
  if (B.trace) for (auto& e : B.evs) (void)hipEventCreate(&e);
  B.mark(0);
  const double tp0 = wall_s();
  GnPassOpts pass;
  pass.write_l11c = true;
  if (B.use_w) B.Ed.ga.weight = (double*)(ds + S.s_w);          // (went up with the staging block above)
  gn_pass_on(ctx, DB, st, d_work0, B.Ed, pass);
  const double tp1 = wall_s();
  B.t_gn = tp1 - tp0;
  B.mark(1);
  MargBatch MBt;
  MBt.jobs = (const CondJobDev*)(ds + S.s_jd);
  MBt.marg_stride = (long long)B.per_job;
  double *est0, *info0;
  if (B.to_wire) { est0 = g->d_est64; info0 = g->d_info64; MBt.est_stride = 24LL * cap; MBt.info_stride = 48LL * cap; MBt.wire_stride = (long long)sizeof(WireEdge) * cap; }
  else { est0 = (double*)(d0 + M.o_est); info0 = (double*)(d0 + M.o_info); MBt.est_stride = MBt.info_stride = (long long)B.per_job; }
  launch_marginals(st, DB, maxq, (const int32_t*)(d0 + M.o_qc), M.m, (double*)(d0 + M.o_Y), (double*)(d0 + M.o_U), (double*)(d0 + M.o_part),
                   (double*)(d0 + M.o_G), (double*)(d0 + M.o_cov), M.chunk, M.nchunk, (uint8_t*)(d0 + M.o_live), &MBt, /*y_is_zero=*/true);
  B.mark(2);
  launch_label(st, maxq, (const int32_t*)(d0 + M.o_qv), 0, d_work0, (const double*)(d0 + M.o_cov), est0, info0, (int*)(d0 + M.o_fl), &DB, &MBt);
  if (B.to_wire) {
    WireEdge* send_edges = reinterpret_cast<WireEdge*>(g->d_send + wire_edges_off(g->n_robots));
    launch_wire_write_edges(st, maxq, 0, (const int32_t*)(d0 + M.o_qv), (const int32_t*)g->d_vids.ptr, est0, info0, send_edges, nj, &MBt);
  }
  B.mark(3);
  HIP_TRY(ctx, hipMemcpy2DAsync(B.hstage + S.s_st, 16, DB.status, (size_t)DB.job_stride, 16, (size_t)nj, hipMemcpyDeviceToHost, st));
  B.t_marg = wall_s() - tp1;
  return 0;
}

// Ending of a batch that is not waited for (ev_cond_done is recorded behind it): the status words are looked at by
// cond_finish(); a message packed before that gets its counts corrected on the device (cgmr_graph_pack).
void cond_hand_over(CondBatch& B) {
  cgmr_graph* g = B.g;
  g->cond_pending = true;
  g->cond_last_rc = 0;
  g->cond_peers.clear();
  for (CondJob& J : B.jobs) g->cond_peers.push_back(J.peer);
  g->cond_status = (const int32_t*)(B.hstage + B.S.s_st);
  g->cond_jobs_dev = (const CondJobDev*)(B.ds + B.S.s_jd);
  g->cond_status_dev = B.DB.status;
  g->cond_status_stride = B.DB.job_stride;
  if (B.trace)
    fprintf(stderr, "[cond] %d jobs queued on the side stream, nV %d nE %d: structure %.0f us, queueing %.0f us (work space %.0f, initial guesses %.0f, masks %.0f, uploads %.0f, GN pass %.0f, marginals + labels %.0f)\n",
            B.nj, B.nV, B.nE, 1e6 * B.t_structure, 1e6 * (wall_s() - B.t0 - B.t_structure), 1e6 * B.t_space, 1e6 * B.t_guess, 1e6 * B.t_mask, 1e6 * B.t_up, 1e6 * B.t_gn, 1e6 * B.t_marg);
}

// Ending of a waited batch: the information matrices of a gauge search (info_out[i], 6 doubles per edge) come back with the
// status words.
int cond_wait(CondBatch& B, std::vector<std::vector<double>>* info_out) {
  cgmr_graph* g = B.g;
  cgmr_ctx* ctx = B.ctx;
  const int nj = B.nj;
  if (info_out) info_out->assign(nj, {});
  for (int i = 0; i < nj && info_out && !B.to_wire; i++) {
    (*info_out)[i].resize(6 * B.jobs[i].q.size());
    HIP_TRY(ctx, hipMemcpyAsync((*info_out)[i].data(), B.d0 + B.per_job * (size_t)i + B.M.o_info, 48 * B.jobs[i].q.size(), hipMemcpyDeviceToHost, B.st));
  }
  const double t2 = wall_s();
  HIP_TRY(ctx, hipStreamSynchronize(B.st));
  HIP_TRY(ctx, hipGetLastError());
  const BatchStatus s = batch_status((const int32_t*)(B.hstage + B.S.s_st), (size_t)nj);
  if (B.trace) {
    float a = 0, b = 0, c = 0;
    (void)hipEventElapsedTime(&a, B.evs[0], B.evs[1]); (void)hipEventElapsedTime(&b, B.evs[1], B.evs[2]); (void)hipEventElapsedTime(&c, B.evs[2], B.evs[3]);
    fprintf(stderr, "[cond]   device: GN pass %.0f us, marginals %.0f us (m %d, %d levels), labels + wire %.0f us\n", 1e3 * a, 1e3 * b, B.M.m, B.DB.nlevels_full, 1e3 * c);
    fprintf(stderr, "[cond] %d jobs in one batch, nV %d nE %d: structure %.0f us, queueing %.0f us (initial guesses %.0f, masks %.0f, uploads %.0f, GN pass %.0f, marginals + labels %.0f), waiting %.0f us\n",
            nj, B.nV, B.nE, 1e6 * B.t_structure, 1e6 * (t2 - B.t0 - B.t_structure), 1e6 * B.t_guess, 1e6 * B.t_mask, 1e6 * B.t_up, 1e6 * B.t_gn, 1e6 * B.t_marg, 1e6 * (wall_s() - t2));
  }
  if (s.timed_out) count_timeout(ctx);
  return batch_outcome(g, s.timed_out ? CGMR_E_TIMEOUT : s.failed ? CGMR_E_CHOLESKY_BASE : 0);
}

// CondensedGraphCreator::compute (condensed_graph_creator.cpp:33-66) for a batch of (gauge, vertex set) jobs on the
// robot's own edges: ONE sequence of launches with a job dimension (a single job is a batch of one).
// to_wire: the labelled edges go to the peer's slots (double-precision copy + 44-byte wire records in the send
// buffer); otherwise only the information matrices come back (info_out[i], 6 doubles per edge: gauge search).
// async_out (nullable): on entry true = queue the batch on the context's side stream and return without waiting (the
// caller finishes it later: cond_finish); set to false when the batch could not be queued that way and was waited for.
int run_cond_jobs(cgmr_graph* g, std::vector<CondJob>& jobs, bool to_wire, std::vector<std::vector<double>>* info_out,
                  bool* async_out = nullptr) {
  cgmr_ctx* ctx = g->ctx;
  bool go_async = async_out && *async_out && to_wire && !info_out;
  if (async_out) *async_out = false;
  if (jobs.empty()) return 0;
  CondBatch B(g, jobs, to_wire);
  B.trace = ctx->sw.cond_trace;
  B.t0 = wall_s();
  int rc = cond_setup(B);
  if (rc) return rc;
  // (the callers come with own edges only, and analyze() gives every vertex with an edge a column: never without a free one)
  if (B.nf == 0) return gerr(g, CGMR_E_INVALID, "condensed graphs: the structure has no free column");
  // whatever ran on the side stream before (another graph of this context, this graph's previous batch) used the work spaces
  // this batch is about to fill
  // (work queued on the side stream behind the fork is marked -- side_busy, side_tail -- even when this function leaves on an error:
  // the next join then waits for it instead of skipping it)
  struct SideGuard {
    cgmr_ctx* c; bool armed;
    ~SideGuard() { if (armed) (void)side_mark(c); }
  } side_guard{ctx, false};
  B.st = ctx->stream;
  if (go_async) {
    rc = side_fork(ctx);
    if (rc) return rc;
    side_guard.armed = true;
    B.st = ctx->side;
    rc = wait_consumers(g, B.st);
    if (rc) return rc;
  } else {
    rc = side_join_stream(ctx, B.st);
    if (rc) return rc;
    rc = wait_consumers(g, B.st);
    if (rc) return rc;
  }
  rc = cond_stage_block(B, go_async);
  if (rc) return rc;
  cond_fill_stage(B);
  rc = cond_queue(B);
  if (rc) return rc;
  if (!go_async) return cond_wait(B, info_out);
  HIP_TRY(ctx, hipEventRecord(g->ev_cond_done, B.st));
  side_guard.armed = false;
  rc = side_mark(ctx);
  if (rc) return rc;
  cond_hand_over(B);
  *async_out = true;
  return 0;
}

// computeOverallUncertainty (condensed_graph_buffer.cpp:172-180): sum over the star's edges of det(information^-1)
double overall_uncertainty(const std::vector<double>& info_upper) {
  double total = 0;
  for (size_t k = 0; k + 5 < info_upper.size(); k += 6) {
    const double* u = &info_upper[k];
    const double a = u[0], b = u[1], c = u[2], d = u[3], e = u[4], f = u[5];
    const double det = a * (d * f - e * e) - b * (b * f - e * c) + c * (b * e - d * c);
    total += 1.0 / det;                                          // det(A^-1) = 1 / det(A)
  }
  return total;
}

// CondensedGraphBuffer::computeCondensedGraph(robot, optimal) (condensed_graph_buffer.cpp:437-485) for one peer or, with
// peer < 0, for every peer that has asked for vertices: gauge = selectGaugeCentroid (:318-345) -- or, after
// cgmr_graph_set_optimal_gauge(g, 1), selectOptimalGauge (:252-288: the candidate whose star has the smallest overall
// uncertainty, every candidate's condensed graph being built for that) --, edges = getMyEdges (own edges only),
// CondensedGraphCreator::compute per peer.  The passes of all peers (and of eight gauge candidates at a time) run as
// one batch; the labelled edges land in the send buffer as wire records.  Returns the number of peers built.
int compute_condensed_impl(cgmr_graph* g, int peer, bool go_async) {
  if (!g || peer >= g->n_robots) return CGMR_E_INVALID;
  if (!g->ctx) return gerr(g, CGMR_E_NO_DEVICE, "cgmr_graph_compute_condensed: the graph was created without a device context");
  cgmr_ctx* ctx = g->ctx;
  if (int rc = graph_device(g)) return rc;
  hipStream_t st = ctx->stream;
  {
    // the previous batch, if it was not waited for.  Its failure (Cholesky, time-out) cost its peers that round's edges and is
    // on record (cond_last_rc until the next batch is queued, cgmr_graph_failed_batches); it must not cost them this round's
    // as well: the current batch is built regardless (round 4 returned the old error here and the run stopped)
    const int rc = finish_pending(g, /*tolerate_failed_batch=*/true);
    if (rc) return rc;
  }
  const double t0 = wall_s();
  const int nV = (int)g->ids.size(), nA = (int)g->ef.size(), cap = g->cap;
  struct Want { int peer; std::vector<int32_t> idx; };
  std::vector<Want> wants;
  for (int p = 0; p < g->n_robots; p++) {
    if (p == g->robot || (peer >= 0 && p != peer)) continue;
    Want W;
    W.peer = p;
    for (int32_t id : g->out_closures[p]) W.idx.push_back(g->index[id]);       // id order (VertexIDMap)
    if (W.idx.size() < 2) { g->out[p].n = 0; g->out[p].host.clear(); g->out[p].host_valid = true; continue; }
    if (slice_not_sent((int)W.idx.size() - 1, 0, cap)) {           // more edges than a message holds: nothing would be sent
      g->out[p].n = 0; g->out[p].host.clear(); g->out[p].host_valid = true;
      g->skipped_messages++;
      continue;
    }
    wants.push_back(std::move(W));
  }
  if (wants.empty() || nA == 0) return 0;
  // current estimates -> host (gauge selection, spanning-tree initial guess); the last optimize() brought them along when
  // it knew that condensed graphs would follow
  if (!g->h_poses_fresh) {
    HIP_TRY(ctx, hipMemcpyAsync(g->h_poses.data(), g->d_poses.ptr, 24 * (size_t)nV, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  std::vector<CondJob> jobs;
  for (Want& W : wants) {
    CondJob J;
    J.peer = W.peer;
    J.gauge = select_gauge_centroid(W.idx, g->h_poses.data());
    if (g->optimal_gauge) {
      // selectOptimalGauge: every requested vertex in turn as the gauge, eight candidates' passes in flight
      double best = 1.79769313486231570815e308;
      for (size_t c0 = 0; c0 < W.idx.size(); c0 += 8) {
        std::vector<CondJob> cand;
        for (size_t c = c0; c < std::min(W.idx.size(), c0 + 8); c++) {
          CondJob C;
          C.peer = W.peer; C.gauge = W.idx[c];
          for (int v : W.idx) if (v != C.gauge) C.q.push_back(v);
          cand.push_back(std::move(C));
        }
        std::vector<std::vector<double>> info;
        int rc = run_cond_jobs(g, cand, /*to_wire=*/false, &info);
        if (rc) return rc;
        for (size_t c = 0; c < cand.size(); c++) {
          const double u = overall_uncertainty(info[c]);
          if (u < best) { best = u; J.gauge = cand[c].gauge; }
        }
      }
      g->out[W.peer].uncertainty = best;
    }
    for (int v : W.idx) if (v != J.gauge) J.q.push_back(v);
    jobs.push_back(std::move(J));
  }
  bool queued = go_async;
  int rc = run_cond_jobs(g, jobs, /*to_wire=*/true, nullptr, &queued);
  if (rc == CGMR_E_TIMEOUT && !g->cond_levelwise) {
    // a bounded wait of the chained backward solve ran out: once more with one launch per tree level (gn_run does the same)
    g->cond_levelwise = true;
    queued = go_async;
    rc = run_cond_jobs(g, jobs, /*to_wire=*/true, nullptr, &queued);
  }
  if (rc) { for (CondJob& J : jobs) { g->out[J.peer].n = 0; g->out[J.peer].host_valid = false; } return rc; }
  for (CondJob& J : jobs) {
    PeerOut& O = g->out[J.peer];
    O.n = (int)J.q.size();
    O.gauge_id = g->ids[J.gauge];
    O.to_idx = J.q;
    O.host_valid = false;
  }
  g->last_condense_seconds = wall_s() - t0;
  return (int)jobs.size();
}

}  // namespace

extern "C" {

int cgmr_graph_compute_condensed(cgmr_graph* g, int peer) { return compute_condensed_impl(g, peer, false); }

// The same, queued on the context's side stream and NOT waited for: the call returns once the passes are queued (the host
// part -- gauges, spanning-tree guesses, masks -- is done), the device part runs beside whatever the caller does next on the
// context's stream (the reference builds its condensed graphs on the communication thread, src/mrslam/graph_comm.cpp:195-207,
// beside the main loop).  The batch reads a snapshot: the estimates and own edges as they are now; vertices / edges added and
// solves run afterwards do not touch it.  cgmr_graph_pack / cgmr_allgather_condensed / cgmr_graph_deliver order themselves
// behind it on the device; every entry point that hands results to the HOST (cgmr_graph_get_condensed, _pack_host,
// _message_for, the next _compute_condensed*) waits for it first.  A failed pass (Cholesky, time-out) is reported by
// cgmr_graph_condensed_wait or by the next call that waits; the message packed meanwhile carries no edges for the batch's peers.
// Returns the number of peers whose condensed graph is being built.
int cgmr_graph_compute_condensed_async(cgmr_graph* g, int peer) {
  if (g) use_side_stream(g->ctx);
  return compute_condensed_impl(g, peer, true);
}

// Wait for the batch queued by cgmr_graph_compute_condensed_async (nothing to wait for: CGMR_OK) and report how it ended.
int cgmr_graph_condensed_wait(cgmr_graph* g) {
  if (!g) return CGMR_E_INVALID;
  if (!g->ctx) return CGMR_OK;
  if (int rc = graph_device(g)) return rc;
  if (g->cond_pending) return cond_finish(g);
  return batch_outcome(g, g->cond_last_rc);     // (another call has waited for the batch already: its outcome is kept)
}

// Announce that this graph will use cgmr_graph_compute_condensed_async (call before the first solve: the chained backward
// solves of the context's stream and of the side stream then share the resident workgroups from the start).
int cgmr_graph_set_async(cgmr_graph* g, int on) {
  if (!g) return CGMR_E_INVALID;
  if (on) use_side_stream(g->ctx);
  return CGMR_OK;
}

// optimal = 1: computeCondensedGraph picks the gauge with selectOptimalGauge instead of selectGaugeCentroid (the
// reference's default is the centroid: condensed_graph_buffer.h:55, mr_graph_slam.cpp:347)
int cgmr_graph_set_optimal_gauge(cgmr_graph* g, int optimal) {
  if (!g) return CGMR_E_INVALID;
  g->optimal_gauge = optimal != 0;
  return CGMR_OK;
}

// The condensed graph built for `peer`, in double precision (before the wire narrows it): returns the number of edges;
// from_id_out = the gauge, to_ids_out [n], est_out [n*3], info_upper_out [n*6] (all nullable)
int cgmr_graph_get_condensed(cgmr_graph* g, int peer, int cap, int32_t* from_id_out, int32_t* to_ids_out, double* est_out,
                             double* info_upper_out) {
  if (!g || peer < 0 || peer >= g->n_robots || cap < 0) return CGMR_E_INVALID;
  if (int rc = finish_pending(g, false)) return rc;
  PeerOut& O = g->out[peer];
  const int n = std::min(O.n, cap);
  if (from_id_out) *from_id_out = O.gauge_id;
  if (O.host_valid) {               // set from the host (cgmr_graph_set_condensed): float32 is all there is
    for (int k = 0; k < n; k++) {
      double est[3], info[6];
      widen(O.host[k], est, info);
      if (to_ids_out) to_ids_out[k] = O.host[k].to;
      if (est_out) memcpy(est_out + 3 * k, est, sizeof est);
      if (info_upper_out) memcpy(info_upper_out + 6 * k, info, sizeof info);
    }
    return O.n;
  }
  if (!g->ctx) return O.n;
  cgmr_ctx* ctx = g->ctx;
  if (int rc = graph_device(g)) return rc;
  if (to_ids_out) for (int k = 0; k < n; k++) to_ids_out[k] = g->ids[O.to_idx[k]];
  if (est_out && n) HIP_TRY(ctx, hipMemcpyAsync(est_out, g->d_est64 + 3 * (size_t)g->cap * peer, 24 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (info_upper_out && n) HIP_TRY(ctx, hipMemcpyAsync(info_upper_out, g->d_info64 + 6 * (size_t)g->cap * peer, 48 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return O.n;
}

// Test / integration hook: install a condensed graph for `peer` from host data (what computeCondensedGraph would have
// produced), in wire precision.
int cgmr_graph_set_condensed(cgmr_graph* g, int peer, int n, int32_t from_id, const int32_t* to_ids, const float* est,
                             const float* info_upper) {
  if (!g || peer < 0 || peer >= g->n_robots || n < 0 || n > g->cap || (n > 0 && (!to_ids || !est || !info_upper))) return CGMR_E_INVALID;
  if (int rc = finish_pending(g, false)) return rc;
  PeerOut& O = g->out[peer];
  O.n = n; O.gauge_id = from_id; O.host.resize(n); O.host_valid = true; O.to_idx.clear();
  for (int k = 0; k < n; k++) {
    O.host[k].from = from_id; O.host[k].to = to_ids[k];
    memcpy(O.host[k].est, est + 3 * k, 12);
    memcpy(O.host[k].info, info_upper + 6 * k, 24);
  }
  if (g->ctx && n > 0) {
    cgmr_ctx* ctx = g->ctx;
    if (int rc = graph_device(g)) return rc;
    WireEdge* dst = reinterpret_cast<WireEdge*>(g->d_send + wire_edges_off(g->n_robots)) + (size_t)g->cap * peer;
    int rcw = wait_consumers(g, ctx->stream);
    if (rcw) return rcw;
    HIP_TRY(ctx, hipMemcpyAsync(dst, O.host.data(), sizeof(WireEdge) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return CGMR_OK;
}

}  // extern "C"
