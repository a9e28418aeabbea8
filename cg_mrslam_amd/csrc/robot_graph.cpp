// C ABI of the multi-robot path (include/cgmr.h, "robot graph"): one robot's pose graph resident in HBM, grown
// incrementally, optimised in place, condensed for every peer that asked, exchanged as 44-byte wire edges.
// This file: the graph itself -- create / destroy, growth, poses, closure lists, robust and GNC settings, the optimisers.
// The condensed graphs are in condensed_host.cpp, the exchange in exchange_host.cpp (robot_graph.h: which file holds what).
//
// Reference behaviour being replaced (each file names the lines of what it holds):
//   GraphSLAM::optimize                       src/slam/graph_slam.cpp:561-575
//   CondensedGraphBuffer                      src/mrslam/condensed_graph/condensed_graph_buffer.cpp
//     insertInClosure / insertOutClosure      :131-170      getMyEdges            :347-366
//   wire structs (wire_format.h)              src/mrslam/msg_factory.h:78-112,200-238
// The graph *structure* (ids, edge end points, closure lists) lives on the host, as g2o's does; everything numeric
// (poses, measurements, information matrices, received edges, the wire buffers) lives in HBM.
#include "robot_graph.h"

using namespace cgmr;

namespace cgmr {

int gerr(cgmr_graph* g, int code, const char* msg) {
  g->err = msg;
  if (g->ctx) set_err(g->ctx, code, "%s", msg);
  return code;
}

int dev_grow(cgmr_graph* g, DevBuf& B, size_t used_bytes, size_t need_bytes) {
  if (need_bytes <= B.cap) return 0;
  cgmr_ctx* ctx = g->ctx;
  size_t want = std::max(std::max(need_bytes + need_bytes / 2, 2 * B.cap), (size_t)1 << 16);
  char* p = nullptr;
  hipError_t e = hipMalloc((void**)&p, want);
  if (e != hipSuccess) return set_err(ctx, CGMR_E_ALLOC, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
  if (B.ptr) {
    // the contents move on the context's stream (whatever is appended next follows on the same stream); the old block is
    // not freed here -- a batch on the side stream may still read it, and hipFree waits for the whole device -- but with
    // the context (cgmr_ctx.h: graveyard)
    if (used_bytes) HIP_TRY(ctx, hipMemcpyAsync(p, B.ptr, used_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->graveyard.push_back({B.ptr, g});
  }
  B.ptr = p;
  B.cap = want;
  return 0;
}

void rebuild_all_edges(cgmr_graph* g) {
  g->all_ef = g->ef;
  g->all_et = g->et;
  g->nB = 0;
  for (int p = 0; p < g->n_robots; p++) {
    g->all_ef.insert(g->all_ef.end(), g->in[p].from_idx.begin(), g->in[p].from_idx.end());
    g->all_et.insert(g->all_et.end(), g->in[p].to_idx.begin(), g->in[p].to_idx.end());
    g->nB += (int)g->in[p].slot.size();
  }
}

void insert_sorted_unique(std::vector<int32_t>& v, const int32_t* ids, int n) {
  v.insert(v.end(), ids, ids + n);
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
}

GnEdges graph_edges(const cgmr_graph* g, int n_active) {
  GnEdges Ed;
  Ed.meas_a = (const double*)g->d_meas_a.ptr; Ed.info_a = (const double*)g->d_info_a.ptr;
  Ed.meas_b = g->d_meas_b; Ed.info_b = g->d_info_b;
  Ed.nA = (int)g->ef.size(); Ed.n_active = n_active;
  return Ed;
}

}  // namespace cgmr

namespace {

// the gauge vertices of the stars received from the peers (every received edge starts at one), in order of first appearance
std::vector<int32_t> received_hubs(const cgmr_graph* g) {
  std::vector<int32_t> hubs;
  for (int p = 0; p < g->n_robots; p++)
    for (int32_t v : g->in[p].from_idx) if (std::find(hubs.begin(), hubs.end(), v) == hubs.end()) hubs.push_back(v);
  return hubs;
}

// the page-locked landing zone of a solve's pose read-back, for nV poses
int pinned_poses_reserve(cgmr_graph* g, int nV) {
  if ((size_t)nV <= g->pinned_poses_cap) return 0;
  cgmr_ctx* ctx = g->ctx;
  if (g->pinned_poses) (void)hipHostFree(g->pinned_poses);
  g->pinned_poses = nullptr;
  g->pinned_poses_cap = (size_t)nV + (size_t)nV / 2 + 1024;
  HIP_TRY(ctx, hipHostMalloc((void**)&g->pinned_poses, 24 * g->pinned_poses_cap, hipHostMallocDefault));
  return 0;
}

// What cgmr_graph_optimize and cgmr_graph_optimize_gnc share around their *_run.  The system the graph solves now: the level-0
// edges from its device arrays (own edges, then the received ones), the received stars' gauge vertices as hubs of the ordering.
// begin(): the clock, the hubs, the landing zone of the estimates -- they come back in the solve's own final wait: the
// condensed graphs that follow pick their gauges from the host copy, the caller's next key frame dead-reckons from it
// (cgmr_graph_get_poses: no device round trip then) --, the LM / dogleg records cleared.  end(): the host copy and what was solved.
struct GraphSolve {
  cgmr_graph* g;
  const int nV, nE, nA;
  GnEdges Ed;
  std::vector<int32_t> hubs;
  GnSystem sys;
  double t0 = 0;
  explicit GraphSolve(cgmr_graph* graph)
      : g(graph), nV((int)g->ids.size()), nE((int)g->all_ef.size()), nA((int)g->ef.size()), Ed(graph_edges(g, nE)),
        sys{nV, (double*)g->d_poses.ptr, g->fixed.data(), nE, g->all_ef.data(), g->all_et.data()} {
    g->rk_stats.clear();
  }
  int begin() {
    t0 = wall_s();
    hubs = received_hubs(g);
    sys.hub_vertices = hubs.data(); sys.n_hub_vertices = (int)hubs.size();
    const int rc = pinned_poses_reserve(g, nV);
    if (rc) return rc;
    g->ctx->poses_out_host = g->pinned_poses;                    // (the estimates ride in every wait of the driver: the last one counts)
    g->lm_lambda.clear(); g->lm_trials.clear(); g->dl_delta.clear(); g->dl_trials.clear(); g->dl_step.clear();
    return 0;
  }
  static bool ended(int rc) { return rc == CGMR_OK || rc <= CGMR_E_CHOLESKY_BASE; }
  int end(int rc) {
    g->ctx->poses_out_host = nullptr;
    g->h_poses_fresh = ended(rc);
    if (g->h_poses_fresh) memcpy(g->h_poses.data(), g->pinned_poses, 24 * (size_t)nV);
    g->last_optimize_seconds = wall_s() - t0;
    g->solved_ef = g->all_ef; g->solved_et = g->all_et;
    g->solved_nV = nV; g->solved_nA = nA;
    return rc;
  }
};

// some own edge, or the received class, carries a robust kernel other than none
bool any_robust_kernel(const cgmr_graph* g) {
  if (g->rk_recv_kind != CGMR_RK_NONE) return true;
  for (uint8_t k : g->rk_kind) if (k != CGMR_RK_NONE) return true;
  return false;
}

// the robust kinds / deltas of own edges [first, first + n) to the device arrays (grown to every own edge)
int rk_upload(cgmr_graph* g, int first, int n) {
  cgmr_ctx* ctx = g->ctx;
  if (!ctx) return 0;
  const size_t nA = g->ef.size(), used = g->rk_dev ? std::min(nA, (size_t)first) : 0;
  if (int rc = graph_device(g)) return rc;
  int rc = dev_grow(g, g->d_rk_kind, used, nA);
  if (!rc) rc = dev_grow(g, g->d_rk_delta, 8 * used, 8 * nA);
  if (rc) return rc;
  if (!g->rk_dev) { first = 0; n = (int)nA; }
  if (n > 0 && g->cond_pending) {     // (a condensed batch not waited for may still read the entries rewritten in place)
    int rj = side_join_stream(ctx, ctx->stream);
    if (rj) return rj;
  }
  if (n > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(g->d_rk_kind.ptr + first, g->rk_kind.data() + first, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(g->d_rk_delta.ptr + 8 * (size_t)first, g->rk_delta.data() + first, 8 * (size_t)n, hipMemcpyHostToDevice,
                                ctx->stream));
  }
  g->rk_dev = true;
  return 0;
}

int alloc_fixed(cgmr_graph* g) {
  cgmr_ctx* ctx = g->ctx;
  const size_t R = g->n_robots, cap = g->cap, slots = R * cap, wb = wire_bytes(g->n_robots, g->cap);
  const size_t ids_bytes = IdsLayout{g->cap}.bytes(g->n_robots);
  size_t off = 0;
  auto add = [&](size_t bytes) { size_t o = off; off = round256(off + bytes); return o; };
  const size_t o_sm = add(24 * slots), o_si = add(48 * slots), o_tm = add(24 * slots), o_ti = add(48 * slots),
               o_mb = add(24 * slots), o_ib = add(48 * slots), o_e64 = add(24 * slots), o_i64 = add(48 * slots),
               o_qp = add(24 * slots), o_ids = add(ids_bytes), o_slot = add(4 * slots), o_qi = add(4 * slots),
               o_st = add(4 * R * 4), o_send = add(wb), o_recv = add(R * wb), o_recv2 = add(R * wb);
  HIP_TRY(ctx, hipMalloc((void**)&g->d_fixed_block, off));
  HIP_TRY(ctx, hipMemsetAsync(g->d_fixed_block, 0, off, ctx->stream));
  char* d = g->d_fixed_block;
  g->d_stage_meas = (double*)(d + o_sm); g->d_stage_info = (double*)(d + o_si);
  g->d_tmp_meas = (double*)(d + o_tm); g->d_tmp_info = (double*)(d + o_ti);
  g->d_meas_b = (double*)(d + o_mb); g->d_info_b = (double*)(d + o_ib);
  g->d_est64 = (double*)(d + o_e64); g->d_info64 = (double*)(d + o_i64); g->d_qposes = (double*)(d + o_qp);
  g->d_ids_out = (int32_t*)(d + o_ids); g->d_slot = (int32_t*)(d + o_slot); g->d_qidx = (int32_t*)(d + o_qi);
  g->d_status_all = (int32_t*)(d + o_st);
  g->d_send = (unsigned char*)(d + o_send); g->d_recv = (unsigned char*)(d + o_recv); g->d_recv2 = (unsigned char*)(d + o_recv2);
  g->n_delivered.assign(R, 0);
  g->recv_round[0].assign(R, -1);
  g->recv_round[1].assign(R, -1);
  Layout256 P;                        // the pinned block (robot_graph.h: PinnedLayout)
  g->pin.wire = P.add(wb); g->pin.ids = P.add(ids_bytes); g->pin.slot = P.add(4 * slots); g->pin.msg = P.add(72 * cap);
  g->pin.bytes = round256(P.off);
  HIP_TRY(ctx, hipHostMalloc((void**)&g->pinned, g->pin.bytes, hipHostMallocDefault));
  HIP_TRY(ctx, hipEventCreateWithFlags(&g->ev_msg, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&g->ev_cond_done, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&g->ev_pack, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&g->ev_packed, hipEventDisableTiming));
  g->ev_consumed.assign(g->n_robots, nullptr);
  g->consumed_pending.assign(g->n_robots, 0);
  for (hipEvent_t& e : g->ev_consumed) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return 0;
}

}  // namespace

extern "C" {

int cgmr_graph_create(cgmr_ctx* ctx, int robot_id, int n_robots, int base_id, int cap_edges_per_peer, cgmr_graph** out) {
  if (!out) return CGMR_E_INVALID;
  *out = nullptr;
  if (robot_id < 0 || n_robots < 1 || robot_id >= n_robots || n_robots > 64 || base_id < 1 || cap_edges_per_peer < 1 ||
      cap_edges_per_peer > 2270)      // MAX_LENGTH_MSG = 100000 bytes holds about 2270 edges of 44 bytes (graph_comm.h)
    return ctx ? set_err(ctx, CGMR_E_INVALID, "cgmr_graph_create: bad argument") : CGMR_E_INVALID;
  cgmr_graph* g = new cgmr_graph();
  g->ctx = ctx; g->robot = robot_id; g->n_robots = n_robots; g->base_id = base_id; g->cap = cap_edges_per_peer;
  g->in.resize(n_robots); g->out.resize(n_robots);
  g->out_closures.resize(n_robots); g->in_closures.resize(n_robots);
  g->hs_meas.assign(3 * (size_t)n_robots * g->cap, 0.0);
  g->hs_info.assign(6 * (size_t)n_robots * g->cap, 0.0);
  g->hs_fresh.assign(n_robots, 1);
  if (ctx) {
    if (hipSetDevice(ctx->device) != hipSuccess) { delete g; return CGMR_E_NO_DEVICE; }
    int rc = alloc_fixed(g);
    if (rc) { cgmr_graph_destroy(g); return rc; }
  }
  *out = g;
  return CGMR_OK;
}

void cgmr_graph_destroy(cgmr_graph* g) {
  if (!g) return;
  // (a binding's garbage collector may get here at interpreter exit, after the HIP runtime has begun to take itself apart:
  // its calls then throw -- std::bad_variant_access was seen -- and a destructor must not end the process for that)
  try {
  if (g->ctx) {
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    (void)side_join_host(g->ctx);
    for (DevBuf* b : {&g->d_poses, &g->d_meas_a, &g->d_info_a, &g->d_vids, &g->d_rk_kind, &g->d_rk_delta, &g->d_gnc_w})
      if (b->ptr) (void)hipFree(b->ptr);
    // the blocks this graph's arrays have outgrown (nothing of it is in flight any more: both streams were waited for above)
    auto& gy = g->ctx->graveyard;
    for (auto& q : gy) if (q.second == g) (void)hipFree(q.first);
    gy.erase(std::remove_if(gy.begin(), gy.end(), [g](const std::pair<void*, const void*>& q) { return q.second == g; }), gy.end());
    if (g->d_fixed_block) (void)hipFree(g->d_fixed_block);
    if (g->pinned) (void)hipHostFree(g->pinned);
    if (g->cond_pinned) (void)hipHostFree(g->cond_pinned);
    if (g->pinned_poses) (void)hipHostFree(g->pinned_poses);
    for (hipEvent_t e : {g->ev_msg, g->ev_cond_done, g->ev_pack, g->ev_packed}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->ev_consumed) if (e) (void)hipEventDestroy(e);
  }
  } catch (...) {
  }
  delete g;
}

const char* cgmr_graph_last_error(const cgmr_graph* g) { return g ? g->err.c_str() : "null graph"; }

int cgmr_graph_add_vertices(cgmr_graph* g, int n, const int32_t* ids, const double* poses_xyt, const uint8_t* fixed) {
  if (!g || n < 0 || (n > 0 && (!ids || !poses_xyt))) return CGMR_E_INVALID;
  for (int k = 0; k < n; k++)
    if (g->index.count(ids[k])) return gerr(g, CGMR_E_INVALID, "cgmr_graph_add_vertices: duplicate vertex id");
  const size_t v0 = g->ids.size();
  for (int k = 0; k < n; k++) {
    g->index[ids[k]] = (int32_t)g->ids.size();
    g->ids.push_back(ids[k]);
    g->fixed.push_back(fixed ? fixed[k] : 0);
  }
  g->adj_head.resize(g->ids.size(), -1);
  g->adj_tail.resize(g->ids.size(), -1);
  g->h_poses.insert(g->h_poses.end(), poses_xyt, poses_xyt + 3 * (size_t)n);
  if (g->ctx && n > 0) {
    cgmr_ctx* ctx = g->ctx;
    if (int rc = graph_device(g)) return rc;
    int rc = dev_grow(g, g->d_poses, 24 * v0, 24 * (v0 + n));
    if (!rc) rc = dev_grow(g, g->d_vids, 4 * v0, 4 * (v0 + n));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(g->d_poses.ptr + 24 * v0, poses_xyt, 24 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(g->d_vids.ptr + 4 * v0, ids, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  }
  return CGMR_OK;
}

int cgmr_graph_add_edges(cgmr_graph* g, int n, const int32_t* from_ids, const int32_t* to_ids, const double* meas_xyt,
                         const double* info_upper) {
  if (!g || n < 0 || (n > 0 && (!from_ids || !to_ids || !meas_xyt || !info_upper))) return CGMR_E_INVALID;
  const size_t e0 = g->ef.size();
  for (int k = 0; k < n; k++) {
    auto a = g->index.find(from_ids[k]), b = g->index.find(to_ids[k]);
    if (a == g->index.end() || b == g->index.end()) {
      g->ef.resize(e0); g->et.resize(e0);
      return gerr(g, CGMR_E_INVALID, "cgmr_graph_add_edges: unknown vertex id");
    }
    g->ef.push_back(a->second);
    g->et.push_back(b->second);
  }
  g->h_meas.insert(g->h_meas.end(), meas_xyt, meas_xyt + 3 * (size_t)n);
  g->h_info.insert(g->h_info.end(), info_upper, info_upper + 6 * (size_t)n);
  g->adj_next.resize(2 * g->ef.size(), -1);
  g->e_cs.resize(2 * g->ef.size());
  for (size_t k = e0; k < g->ef.size(); k++) {
    for (int side = 0; side < 2; side++) {
      const int v = side ? g->et[k] : g->ef[k];
      const int32_t item = (int32_t)(2 * k + side);
      if (g->adj_tail[v] < 0) g->adj_head[v] = item; else g->adj_next[g->adj_tail[v]] = item;
      g->adj_tail[v] = item;
    }
    g->e_cs[2 * k] = std::cos(g->h_meas[3 * k + 2]);
    g->e_cs[2 * k + 1] = std::sin(g->h_meas[3 * k + 2]);
  }
  if (g->ctx && n > 0) {
    cgmr_ctx* ctx = g->ctx;
    if (int rc = graph_device(g)) return rc;
    int rc = dev_grow(g, g->d_meas_a, 24 * e0, 24 * (e0 + n));
    if (!rc) rc = dev_grow(g, g->d_info_a, 48 * e0, 48 * (e0 + n));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(g->d_meas_a.ptr + 24 * e0, meas_xyt, 24 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(g->d_info_a.ptr + 48 * e0, info_upper, 48 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  }
  g->rk_kind.resize(g->ef.size(), CGMR_RK_NONE);
  g->rk_delta.resize(g->ef.size(), 1.0);
  g->gnc_c.resize(g->ef.size(), 0.0);
  g->gnc_known.resize(g->ef.size(), 0);
  g->gnc_w.resize(g->ef.size(), 1.0);
  if (g->rk_dev && n > 0) {
    int rc = rk_upload(g, (int)e0, n);
    if (rc) return rc;
  }
  rebuild_all_edges(g);
  return CGMR_OK;
}

int cgmr_graph_counts(const cgmr_graph* g, int32_t out[4]) {
  if (!g || !out) return CGMR_E_INVALID;
  out[0] = (int32_t)g->ids.size(); out[1] = (int32_t)g->ef.size(); out[2] = g->nB;
  int np = 0;
  for (int p = 0; p < g->n_robots; p++) np += g->out_closures[p].empty() ? 0 : 1;
  out[3] = np;
  return CGMR_OK;
}

// void GraphSLAM::optimize(int nrunnings) (src/slam/graph_slam.cpp:561-575) on the level-0 edges: own + received
int cgmr_graph_optimize(cgmr_graph* g, int iters, double* chi2_out) {
  if (!g || iters < 0) return CGMR_E_INVALID;
  if (!g->ctx) return gerr(g, CGMR_E_NO_DEVICE, "cgmr_graph_optimize: the graph was created without a device context");
  cgmr_ctx* ctx = g->ctx;
  if (int rc = graph_device(g)) return rc;
  if (g->ids.empty()) return CGMR_OK;
  GraphSolve S(g);
  GnEdges& Ed = S.Ed;
  const int nE = S.nE;
  if (g->rk_dev) {                    // (set once any kernel is: own edges from the device arrays, received ones from the class)
    Ed.robust = true;
    Ed.rk = {(const uint8_t*)g->d_rk_kind.ptr, (const double*)g->d_rk_delta.ptr, nullptr, g->rk_recv_delta, g->rk_recv_kind};
    if (nE > 0) {
      int rc = arena_reserve(ctx, ctx->rk_arena, 16 * (size_t)nE + 256);
      if (rc) return rc;
      Ed.rk.stats = (double*)ctx->rk_arena.ptr;
    }
  }
  if (g->gnc_keep) {                  // cgmr_graph_keep_gnc_weights: every own edge scaled by its stored weight (kGncReuse)
    if (g->algorithm != CGMR_ALG_GAUSS_NEWTON)
      return gerr(g, CGMR_E_INVALID, "cgmr_graph_optimize: the stored GNC weights (cgmr_graph_keep_gnc_weights) go with Gauss-Newton only");
    if (any_robust_kernel(g))
      return gerr(g, CGMR_E_INVALID, "cgmr_graph_optimize: the stored GNC weights (cgmr_graph_keep_gnc_weights) are not combined with robust kernels");
    Ed.robust = false;
    Ed.rk = RobustArgs();
    if (nE > 0) {
      int rc = dev_grow(g, g->d_gnc_w, 0, 8 * (size_t)nE);
      if (rc) return rc;
      g->gnc_w_up = g->gnc_w;         // (a member: it outlives the copy, and the solve's final wait comes before the next one)
      g->gnc_w_up.resize((size_t)nE, 1.0);
      HIP_TRY(ctx, hipMemcpyAsync(g->d_gnc_w.ptr, g->gnc_w_up.data(), 8 * (size_t)nE, hipMemcpyHostToDevice, ctx->stream));
      Ed.gnc = true; Ed.ga.mode = kGncReuse; Ed.ga.weight = (double*)g->d_gnc_w.ptr;
    }
  }
  int rc = S.begin();
  if (rc) return rc;
  if (g->algorithm == CGMR_ALG_LEVENBERG) {
    std::vector<double> lam(iters);
    std::vector<int32_t> tri(iters);
    int32_t done = 0;
    rc = lm_run(ctx, S.sys, Ed, iters, g->lm_params_set ? &g->lm_params : nullptr, {chi2_out, lam.data(), tri.data(), &done});
    if (rc == CGMR_OK) { g->lm_lambda.assign(lam.begin(), lam.begin() + done); g->lm_trials.assign(tri.begin(), tri.begin() + done); }
  } else if (g->algorithm == CGMR_ALG_DOGLEG) {
    std::vector<double> del(iters);
    std::vector<int32_t> tri(iters), stp(iters);
    int32_t done = 0;
    rc = dl_run(ctx, S.sys, Ed, iters, g->dl_params_set ? &g->dl_params : nullptr, {chi2_out, del.data(), tri.data(), stp.data(), &done});
    if (S.ended(rc)) {
      g->dl_delta.assign(del.begin(), del.begin() + done);
      g->dl_trials.assign(tri.begin(), tri.begin() + done);
      g->dl_step.assign(stp.begin(), stp.begin() + done);
    }
  } else {
    rc = gn_run(ctx, S.sys, Ed, iters, chi2_out);
  }
  if (Ed.rk.stats && S.ended(rc)) {
    ctx->poses_out_host = nullptr; g->h_poses_fresh = true;   // (what end() does first: a failed read-back leaves the graph as it always has)
    g->rk_stats.resize(2 * (size_t)nE);
    HIP_TRY(ctx, hipMemcpyAsync(g->rk_stats.data(), Ed.rk.stats, 16 * (size_t)nE, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return S.end(rc);
}

int cgmr_graph_set_algorithm(cgmr_graph* g, int algorithm, const cgmr_lm_params* params) {
  if (!g || (algorithm != CGMR_ALG_GAUSS_NEWTON && algorithm != CGMR_ALG_LEVENBERG && algorithm != CGMR_ALG_DOGLEG))
    return CGMR_E_INVALID;
  if (algorithm == CGMR_ALG_DOGLEG) {
    if (params) return gerr(g, CGMR_E_INVALID, "cgmr_graph_set_algorithm: dogleg takes its parameters from cgmr_graph_set_dogleg_params");
    g->algorithm = algorithm;
    return CGMR_OK;
  }
  g->algorithm = algorithm;
  g->lm_params_set = params != nullptr;
  if (params) g->lm_params = *params;
  return CGMR_OK;
}

int cgmr_graph_set_dogleg_params(cgmr_graph* g, const cgmr_dl_params* params) {
  if (!g) return CGMR_E_INVALID;
  if (!dl_params_ok(params))
    return gerr(g, CGMR_E_INVALID,
                "cgmr_graph_set_dogleg_params: max_trials must be >= 1, initial_delta / initial_lambda > 0, lambda_factor > 1, all finite");
  g->dl_params_set = params != nullptr;
  if (params) g->dl_params = *params;
  return CGMR_OK;
}

int cgmr_graph_set_edge_robust(cgmr_graph* g, int first, int n, const uint8_t* kind, const double* delta) {
  if (!g || first < 0 || n < 0 || first + n > (int)g->ef.size() || (n > 0 && !kind)) return CGMR_E_INVALID;
  for (int k = 0; k < n; k++)
    if (!robust_valid(kind[k], delta ? delta[k] : 1.0))
      return gerr(g, CGMR_E_INVALID, "cgmr_graph_set_edge_robust: a kind must be 0..7, its delta finite and > 0 (kind 0 excepted)");
  for (int k = 0; k < n; k++) { g->rk_kind[first + k] = kind[k]; g->rk_delta[first + k] = delta ? delta[k] : 1.0; }
  return rk_upload(g, first, n);
}

int cgmr_graph_set_received_robust(cgmr_graph* g, int kind, double delta) {
  if (!g) return CGMR_E_INVALID;
  if (!robust_valid(kind, delta))
    return gerr(g, CGMR_E_INVALID, "cgmr_graph_set_received_robust: the kind must be 0..7, its delta finite and > 0 (kind 0 excepted)");
  g->rk_recv_kind = kind;
  g->rk_recv_delta = kind == CGMR_RK_NONE ? 1.0 : delta;
  return g->rk_dev ? 0 : rk_upload(g, 0, (int)g->ef.size());
}

int cgmr_graph_set_condensed_robust(cgmr_graph* g, int on) {
  if (!g) return CGMR_E_INVALID;
  if (on && g->cond_gnc)
    return gerr(g, CGMR_E_INVALID, "cgmr_graph_set_condensed_robust: refused while cgmr_graph_set_condensed_gnc is on (the GNC instances take no robust kernel)");
  g->cond_robust = on != 0;
  return CGMR_OK;
}

int cgmr_graph_set_edge_gnc(cgmr_graph* g, int first, int n, const double* barc_sq, const uint8_t* known_inlier) {
  if (!g || first < 0 || n < 0 || (size_t)first + (size_t)n > g->ef.size()) return CGMR_E_INVALID;
  for (int k = 0; barc_sq && k < n; k++)
    if (!std::isfinite(barc_sq[k]) || !(barc_sq[k] > 0))
      return gerr(g, CGMR_E_INVALID, "cgmr_graph_set_edge_gnc: barc_sq must be finite and > 0");
  for (int k = 0; k < n; k++) {
    g->gnc_c[first + k] = barc_sq ? barc_sq[k] : 0.0;
    g->gnc_known[first + k] = known_inlier && known_inlier[k] ? 1 : 0;
  }
  return CGMR_OK;
}

int cgmr_graph_set_received_gnc(cgmr_graph* g, double barc_sq, int known_inlier) {
  if (!g) return CGMR_E_INVALID;
  if (!std::isfinite(barc_sq) || barc_sq < 0)
    return gerr(g, CGMR_E_INVALID, "cgmr_graph_set_received_gnc: barc_sq must be finite and > 0, or 0 for the default");
  g->gnc_recv_c = barc_sq;
  g->gnc_recv_known = known_inlier != 0;
  return CGMR_OK;
}

int cgmr_graph_gnc_weights(const cgmr_graph* g, int cap, double* weight_out) {
  if (!g || cap < 0 || (cap > 0 && !weight_out)) return CGMR_E_INVALID;
  const int n = (int)g->gnc_w.size();
  for (int k = 0; k < std::min(n, cap); k++) weight_out[k] = g->gnc_w[k];
  return n;
}

int cgmr_graph_keep_gnc_weights(cgmr_graph* g, int on) {
  if (!g) return CGMR_E_INVALID;
  g->gnc_keep = on != 0;
  return CGMR_OK;
}

int cgmr_graph_set_condensed_gnc(cgmr_graph* g, int on, double drop_below) {
  if (!g) return CGMR_E_INVALID;
  if (on && g->cond_robust)
    return gerr(g, CGMR_E_INVALID, "cgmr_graph_set_condensed_gnc: refused while cgmr_graph_set_condensed_robust is on (the GNC instances take no robust kernel)");
  if (on && (!std::isfinite(drop_below) || drop_below < 0 || drop_below > 1))
    return gerr(g, CGMR_E_INVALID, "cgmr_graph_set_condensed_gnc: drop_below must lie in [0, 1]");
  g->cond_gnc = on != 0;
  g->cond_drop_below = on ? drop_below : 0.0;
  return CGMR_OK;
}

// cgmr_gnc_optimize (include/cgmr.h; the contract: tests/ref_gnc.py) on the system cgmr_graph_optimize would solve now: own
// edges, then the received ones; Gauss-Newton inside; the received stars' gauge vertices are hubs of the ordering.
int cgmr_graph_optimize_gnc(cgmr_graph* g, const cgmr_gnc_params* params, double* mu_out, double* cost_out, int32_t* partial_out,
                            int32_t* outer_done) {
  if (!g) return CGMR_E_INVALID;
  if (!g->ctx) return gerr(g, CGMR_E_NO_DEVICE, "cgmr_graph_optimize_gnc: the graph was created without a device context");
  cgmr_ctx* ctx = g->ctx;
  const cgmr_gnc_params P = params ? *params : gnc_params_default();
  if (!gnc_params_ok(&P))
    return gerr(g, CGMR_E_INVALID, "cgmr_graph_optimize_gnc: loss must be CGMR_GNC_TLS or CGMR_GNC_GM, mu_factor finite and > 1, max_outer / inner_iters / outer_per_wait >= 1, default_barc_sq finite");
  if (P.barc_sq || P.known_inlier || P.weight_out || P.edge_chi2_out)
    return gerr(g, CGMR_E_INVALID, "cgmr_graph_optimize_gnc: the per-edge pointers of the parameters must be null (the graph holds them: cgmr_graph_set_edge_gnc, cgmr_graph_edge_stats, cgmr_graph_gnc_weights)");
  if (any_robust_kernel(g))
    return gerr(g, CGMR_E_INVALID, "cgmr_graph_optimize_gnc: not combined with robust kernels (cgmr_graph_set_edge_robust / _set_received_robust)");
  if (int rc = graph_device(g)) return rc;
  if (outer_done) *outer_done = 0;
  for (int k = 0; k < P.max_outer; k++) { if (mu_out) mu_out[k] = 0.0; if (partial_out) partial_out[k] = 0; }
  for (int k = 0; cost_out && k <= P.max_outer; k++) cost_out[k] = 0.0;
  if (g->ids.empty()) return CGMR_OK;
  GraphSolve S(g);
  const int nE = S.nE, nA = S.nA;
  const double c0 = P.default_barc_sq > 0 ? P.default_barc_sq : gnc_default_barc_sq(3);
  std::vector<double> hc((size_t)nE), hw((size_t)nE, 1.0), hr((size_t)nE, 0.0);
  std::vector<uint8_t> hk((size_t)nE);
  for (int k = 0; k < nE; k++) {
    const double c = k < nA ? g->gnc_c[k] : g->gnc_recv_c;
    hc[k] = c > 0 ? c : c0;
    hk[k] = k < nA ? g->gnc_known[k] : (g->gnc_recv_known ? 1 : 0);
  }
  int rc = S.begin();
  if (rc) return rc;
  rc = gnc_run(ctx, S.sys, S.Ed, P, hc.data(), hk.data(), {mu_out, cost_out, partial_out, outer_done, hw.data(), hr.data()});
  if (S.ended(rc)) {
    g->rk_stats.assign(hr.begin(), hr.end());                     // cgmr_graph_edge_stats: r of every edge, then its weight
    g->rk_stats.insert(g->rk_stats.end(), hw.begin(), hw.end());
  }
  if (rc == CGMR_OK) std::copy(hw.begin(), hw.begin() + nA, g->gnc_w.begin());   // (a Cholesky code leaves the stored weights alone)
  return S.end(rc);
}

int cgmr_graph_edge_stats(const cgmr_graph* g, int cap, double* edge_chi2_out, double* weight_out) {
  if (!g || cap < 0) return CGMR_E_INVALID;
  const int n = (int)(g->rk_stats.size() / 2);
  for (int k = 0; k < std::min(n, cap); k++) {
    if (edge_chi2_out) edge_chi2_out[k] = g->rk_stats[k];
    if (weight_out) weight_out[k] = g->rk_stats[n + k];
  }
  return n;
}

int cgmr_graph_lm_last(const cgmr_graph* g, int cap, double* lambda_out, int32_t* trials_out) {
  if (!g || cap < 0) return CGMR_E_INVALID;
  const int n = (int)g->lm_lambda.size();
  for (int k = 0; k < std::min(n, cap); k++) {
    if (lambda_out) lambda_out[k] = g->lm_lambda[k];
    if (trials_out) trials_out[k] = g->lm_trials[k];
  }
  return n;
}

int cgmr_graph_dl_last(const cgmr_graph* g, int cap, double* delta_out, int32_t* trials_out, int32_t* step_out) {
  if (!g || cap < 0) return CGMR_E_INVALID;
  const int n = (int)g->dl_delta.size();
  for (int k = 0; k < std::min(n, cap); k++) {
    if (delta_out) delta_out[k] = g->dl_delta[k];
    if (trials_out) trials_out[k] = g->dl_trials[k];
    if (step_out) step_out[k] = g->dl_step[k];
  }
  return n;
}

int cgmr_graph_get_poses(cgmr_graph* g, int first, int n, double* poses_out) {
  if (!g || first < 0 || n < 0 || first + n > (int)g->ids.size() || (n > 0 && !poses_out)) return CGMR_E_INVALID;
  if (g->ctx && n > 0 && !g->h_poses_fresh) {          // (fresh: the last optimize() left them on the host as well)
    cgmr_ctx* ctx = g->ctx;
    if (int rc = graph_device(g)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(g->h_poses.data() + 3 * (size_t)first, g->d_poses.ptr + 24 * (size_t)first, 24 * (size_t)n,
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (n) memcpy(poses_out, g->h_poses.data() + 3 * (size_t)first, 24 * (size_t)n);
  return CGMR_OK;
}

int cgmr_graph_set_poses(cgmr_graph* g, int first, int n, const double* poses_xyt) {
  if (!g || first < 0 || n < 0 || first + n > (int)g->ids.size() || (n > 0 && !poses_xyt)) return CGMR_E_INVALID;
  if (n) memcpy(g->h_poses.data() + 3 * (size_t)first, poses_xyt, 24 * (size_t)n);
  if (g->ctx && n > 0) {
    cgmr_ctx* ctx = g->ctx;
    if (int rc = graph_device(g)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(g->d_poses.ptr + 24 * (size_t)first, poses_xyt, 24 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return CGMR_OK;
}

// CondensedGraphBuffer::insertInClosure (condensed_graph_buffer.cpp:131-150): ids of `peer`'s vertices I ask for
int cgmr_graph_insert_in_closure(cgmr_graph* g, int peer, int n, const int32_t* vertex_ids) {
  if (!g || peer < 0 || peer >= g->n_robots || n < 0 || (n > 0 && !vertex_ids)) return CGMR_E_INVALID;
  insert_sorted_unique(g->in_closures[peer], vertex_ids, n);
  return CGMR_OK;
}

// CondensedGraphBuffer::insertOutClosure (:152-170): ids of MY vertices `peer` asked for (unknown ids are dropped, as
// MRGraphSLAM::addInterRobotData does before inserting, mr_graph_slam.cpp:336-343)
int cgmr_graph_insert_out_closure(cgmr_graph* g, int peer, int n, const int32_t* vertex_ids) {
  if (!g || peer < 0 || peer >= g->n_robots || n < 0 || (n > 0 && !vertex_ids)) return CGMR_E_INVALID;
  std::vector<int32_t> known;
  for (int k = 0; k < n; k++) if (g->index.count(vertex_ids[k])) known.push_back(vertex_ids[k]);
  insert_sorted_unique(g->out_closures[peer], known.data(), (int)known.size());
  return CGMR_OK;
}

int cgmr_graph_closures(const cgmr_graph* g, int peer, int which, int cap, int32_t* ids_out) {
  if (!g || peer < 0 || peer >= g->n_robots || cap < 0 || (cap > 0 && !ids_out)) return CGMR_E_INVALID;
  const std::vector<int32_t>& v = which ? g->in_closures[peer] : g->out_closures[peer];
  for (int k = 0; k < (int)v.size() && k < cap; k++) ids_out[k] = v[k];
  return (int)v.size();
}

int cgmr_graph_last_seconds(const cgmr_graph* g, double out[2]) {
  if (!g || !out) return CGMR_E_INVALID;
  out[0] = g->last_optimize_seconds; out[1] = g->last_condense_seconds;
  return CGMR_OK;
}

}  // extern "C"
