// C ABI of the multi-robot path (include/cgmr.h, "robot graph"): one robot's pose graph resident in HBM, grown
// incrementally, optimised in place, condensed for every peer that asked, exchanged as 44-byte wire edges.
//
// Reference behaviour being replaced:
//   MRGraphSLAM::addInterRobotData            src/mrslam/mr_graph_slam.cpp:331-395  (closure requests in, edges in)
//   CondensedGraphBuffer                      src/mrslam/condensed_graph/condensed_graph_buffer.cpp
//     insertInClosure / insertOutClosure      :131-170      getMyEdges            :347-366
//     selectGaugeCentroid                     :318-345      computeCondensedGraph :437-485
//     insertEdgesFromRobot                    :487-510  (the newest set from a robot replaces the previous one)
//   CondensedGraphCreator::compute            src/mrslam/condensed_graph/condensed_graph_creator.cpp:33-66
//   wire structs                              src/mrslam/msg_factory.h:78-112,200-238
// The graph *structure* (ids, edge end points, closure lists) lives on the host, as g2o's does; everything numeric
// (poses, measurements, information matrices, received edges, the wire buffers) lives in HBM.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <unordered_map>
#include <mutex>
#include <vector>

#include "cgmr_ctx.h"
#include "gn_host.h"
#include "gnc_device.h"
#include "mrslam_device.h"

using namespace cgmr;

namespace {

struct DevBuf {                       // growable device array; contents survive growth
  char* ptr = nullptr;
  size_t cap = 0;
};

struct PeerOut {                      // condensed graph built for one peer
  int n = 0;                          // edges
  int32_t gauge_id = -1;
  std::vector<WireEdge> host;         // host copy (set by cgmr_graph_set_condensed or downloaded on demand)
  bool host_valid = false;
  std::vector<int32_t> to_idx;        // vertex index of every edge's far end
  double uncertainty = 0;             // selectOptimalGauge: overall uncertainty of the chosen star
};

struct PeerIn {                       // edges received from one peer (the accepted, newest set)
  std::vector<int32_t> slot, from_idx, to_idx;     // staging slot (peer * cap + k), end points (vertex indices)
};

}  // namespace

struct cgmr_graph {
  cgmr_ctx* ctx = nullptr;            // null: host-only bookkeeping (no numeric entry point works)
  int robot = 0, n_robots = 1, base_id = 10000, cap = 128;
  int64_t skipped_messages = 0;                   // messages left out / dropped because they exceed the wire capacity
  std::string err;
  // vertices
  std::vector<int32_t> ids;
  std::unordered_map<int32_t, int32_t> index;
  std::vector<uint8_t> fixed;
  std::vector<double> h_poses;        // estimates as added / as of the last download
  // own edges (segment A) and received edges (segment B, compact, peer order)
  std::vector<int32_t> ef, et;
  std::vector<double> h_meas, h_info;
  // incidence lists of the own edges, kept as they are appended (item = 2 * edge + side, per vertex in edge order: what a
  // counting sort of the edge list gives), and cos / sin of every own measurement's angle: the spanning-tree initial guesses of
  // a round's condensed graphs walk them instead of rebuilding both per gauge
  std::vector<int32_t> adj_head, adj_tail, adj_next;
  std::vector<double> e_cs;
  std::vector<PeerIn> in;             // per peer
  std::vector<PeerOut> out;           // per peer
  std::vector<std::vector<int32_t>> out_closures, in_closures;   // sorted unique ids
  std::vector<int32_t> all_ef, all_et;                           // A then B
  int nB = 0;
  // the edge list of the last optimize(): the condensed graphs that follow use the own edges only, so the structure analysed
  // for that solve serves them as long as no vertex or own edge has been added since -- whatever the exchange has done to
  // the received edges in between (they are switched off in those passes)
  std::vector<int32_t> solved_ef, solved_et;
  int solved_nV = -1, solved_nA = -1;
  // host staging of received numeric data (host-only mode and getters): slot-indexed like the device staging
  std::vector<double> hs_meas, hs_info;
  // device
  DevBuf d_poses, d_meas_a, d_info_a, d_vids;
  char* d_fixed_block = nullptr;      // one allocation for the fixed-size buffers below
  double *d_stage_meas = nullptr, *d_stage_info = nullptr, *d_tmp_meas = nullptr, *d_tmp_info = nullptr;
  double *d_meas_b = nullptr, *d_info_b = nullptr, *d_est64 = nullptr, *d_info64 = nullptr, *d_qposes = nullptr;
  int32_t *d_ids_out = nullptr, *d_slot = nullptr, *d_qidx = nullptr, *d_status_all = nullptr;
  unsigned char *d_send = nullptr, *d_recv = nullptr;
  unsigned char* d_recv2 = nullptr;   // second receive buffer of the in-process transport (cgmr_graph_deliver): round t's messages land
                                      // in buffer t & 1 while round t - 1's may not have been ingested yet
  std::vector<int64_t> n_delivered;   // per destination robot: messages delivered to it so far
  std::vector<int64_t> recv_round[2]; // per receive buffer and sender: which of the sender's deliveries lies there (-1: none)
  int64_t n_packed = 0;               // messages packed on the device so far (cgmr_graph_deliver needs one)
  int64_t n_ingested_delivered = 0;
  char* pinned = nullptr;             // header + closures staging, ids read-back, slot lists, one message's numbers
  size_t pinned_bytes = 0, pinned_msg_off = 0;
  hipEvent_t ev_msg = nullptr;        // the uploads of the last cgmr_graph_message_from have left the pinned block
  bool msg_in_flight = false;
  std::vector<uint8_t> hs_fresh;      // per peer: hs_meas / hs_info hold what the device staging holds
  double last_condense_seconds = 0, last_optimize_seconds = 0;
  bool optimal_gauge = false;         // computeCondensedGraph(robot, optimal)
  int algorithm = CGMR_ALG_GAUSS_NEWTON;   // cgmr_graph_set_algorithm: the optimiser of cgmr_graph_optimize
  bool lm_params_set = false;
  cgmr_lm_params lm_params{};
  bool dl_params_set = false;          // cgmr_graph_set_dogleg_params (else g2o's defaults)
  cgmr_dl_params dl_params{};
  // robust kernels (cgmr_graph_set_edge_robust): kind / delta of every own edge on the host and, from the first setting on, on
  // the device (rk_dev; grown with d_meas_a); the received edges' class; the per-edge statistics of the last optimize (e2 of
  // every level-0 edge, then rho1; empty when it ran plain)
  std::vector<uint8_t> rk_kind;
  std::vector<double> rk_delta;
  DevBuf d_rk_kind, d_rk_delta;
  bool rk_dev = false;
  int rk_recv_kind = CGMR_RK_NONE;
  double rk_recv_delta = 1.0;
  std::vector<double> rk_stats;
  bool cond_robust = false;           // cgmr_graph_set_condensed_robust: the condensed graphs take the own edges' kernels
  // graduated non-convexity (cgmr_graph_optimize_gnc): per own edge barc^2 (0: the call's default), the known-inlier flag and
  // the stored weight (1 until a GNC solve ends well; the last outer iteration's then); the received edges' class.  The weights
  // live on the host: cgmr_graph_optimize (keep_gnc_weights) and every condensed batch (cond_gnc) send up a copy of their own
  std::vector<double> gnc_c, gnc_w, gnc_w_up;
  std::vector<uint8_t> gnc_known;
  double gnc_recv_c = 0.0;
  bool gnc_recv_known = false;
  bool gnc_keep = false;              // cgmr_graph_keep_gnc_weights
  bool cond_gnc = false;              // cgmr_graph_set_condensed_gnc: the condensed graphs leave the rejected own edges out
  double cond_drop_below = 0.0;
  DevBuf d_gnc_w;                     // the weights of a keep_gnc_weights solve: own edges, then ones for the received
  std::vector<double> lm_lambda;      // records of the last Levenberg solve (cgmr_graph_lm_last)
  std::vector<int32_t> lm_trials;
  std::vector<double> dl_delta;       // records of the last dogleg solve (cgmr_graph_dl_last)
  std::vector<int32_t> dl_trials, dl_step;
  bool h_poses_fresh = false;         // h_poses holds the estimates as the last optimize() left them
  double* pinned_poses = nullptr;     // landing zone of that read-back (page-locked: a copy into the pageable h_poses goes through the runtime's staging path)
  size_t pinned_poses_cap = 0;        // in poses
  // a batch of condensed-graph passes queued on the context's side stream and not waited for yet
  // (cgmr_graph_compute_condensed_async): what is needed to finish it
  bool cond_pending = false;
  int cond_last_rc = 0;               // how the most recent asynchronous batch ended (kept for cgmr_graph_condensed_wait)
  int64_t cond_failed_batches = 0;    // asynchronous batches that failed (Cholesky / time-out): their peers got no edges that round
  bool cond_levelwise = false;        // a batch's chained backward solve has timed out once: the batches solve level by level from now on
  std::vector<int32_t> cond_peers;    // peer of every job of the batch
  const int32_t* cond_status = nullptr;   // pinned: 4 status words per job, valid after ev_cond_done
  const CondJobDev* cond_jobs_dev = nullptr;    // the batch's job table on the device (peer of job j = out_slot)
  const int* cond_status_dev = nullptr;         // first job's status words on the device; cond_status_stride bytes to the next
  long long cond_status_stride = 0;
  char* cond_pinned = nullptr;        // staging block of an asynchronous batch (the context's is the solver's)
  size_t cond_pinned_cap = 0;
  hipEvent_t ev_cond_done = nullptr, ev_pack = nullptr, ev_packed = nullptr;
  bool pack_in_flight = false;        // the uploads of the last cgmr_graph_pack may not have left the pinned block yet
  std::vector<hipEvent_t> ev_consumed;          // per destination robot: its copy of my send buffer is done (cgmr_graph_deliver)
  std::vector<uint8_t> consumed_pending;
};

namespace {

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

size_t round256(size_t v) { return (v + 255) & ~size_t(255); }

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
      : g(graph), nV((int)g->ids.size()), nE((int)g->all_ef.size()), nA((int)g->ef.size()),
        sys{nV, (double*)g->d_poses.ptr, g->fixed.data(), nE, g->all_ef.data(), g->all_et.data()} {
    Ed.meas_a = (const double*)g->d_meas_a.ptr; Ed.info_a = (const double*)g->d_info_a.ptr;
    Ed.meas_b = g->d_meas_b; Ed.info_b = g->d_info_b;
    Ed.nA = nA; Ed.n_active = nE;
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

// The stored GNC weights as a condensed pass takes them (cgmr_graph_set_condensed_gnc): below drop_below, or zero, the edge is
// removed (0); the others keep their weight.
std::vector<double> cond_gnc_weights(const cgmr_graph* g) {
  std::vector<double> w(g->gnc_w);
  for (double& x : w) if (x < g->cond_drop_below || x == 0.0) x = 0.0;
  return w;
}

// the robust kinds / deltas of own edges [first, first + n) to the device arrays (grown to every own edge)
int rk_upload(cgmr_graph* g, int first, int n) {
  cgmr_ctx* ctx = g->ctx;
  if (!ctx) return 0;
  const size_t nA = g->ef.size(), used = g->rk_dev ? std::min(nA, (size_t)first) : 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
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
  size_t off = 0;
  auto add = [&](size_t bytes) { size_t o = off; off = round256(off + bytes); return o; };
  const size_t o_sm = add(24 * slots), o_si = add(48 * slots), o_tm = add(24 * slots), o_ti = add(48 * slots),
               o_mb = add(24 * slots), o_ib = add(48 * slots), o_e64 = add(24 * slots), o_i64 = add(48 * slots),
               o_qp = add(24 * slots), o_ids = add(4 * R * (2 + 3 * cap)), o_slot = add(4 * slots), o_qi = add(4 * slots),
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
  g->pinned_bytes = round256(wb) + round256(4 * R * (2 + 3 * cap)) + round256(4 * slots) + round256(24 * slots) + 4096;
  g->pinned_msg_off = g->pinned_bytes;
  g->pinned_bytes += round256(72 * cap);
  HIP_TRY(ctx, hipHostMalloc((void**)&g->pinned, g->pinned_bytes, hipHostMallocDefault));
  HIP_TRY(ctx, hipEventCreateWithFlags(&g->ev_msg, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&g->ev_cond_done, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&g->ev_pack, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&g->ev_packed, hipEventDisableTiming));
  g->ev_consumed.assign(g->n_robots, nullptr);
  g->consumed_pending.assign(g->n_robots, 0);
  for (hipEvent_t& e : g->ev_consumed) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return 0;
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

// Finish the pending asynchronous batch: wait for it, look at the status words.  A failed pass leaves nothing to send to any
// peer of the batch (as the synchronous call does); the header of a message packed meanwhile was corrected on the device.
int cond_finish(cgmr_graph* g) {
  if (!g->cond_pending) return 0;
  cgmr_ctx* ctx = g->ctx;
  g->cond_pending = false;
  HIP_TRY(ctx, hipEventSynchronize(g->ev_cond_done));
  bool failed = false, timed_out = false;
  for (size_t j = 0; j < g->cond_peers.size(); j++) {
    if (g->cond_status[4 * j] != 0) failed = true;
    if (g->cond_status[4 * j + 2] != 0) timed_out = true;
  }
  g->cond_last_rc = 0;
  if (!failed) return 0;
  for (int32_t p : g->cond_peers) { g->out[p].n = 0; g->out[p].host_valid = false; }
  g->cond_failed_batches++;
  if (timed_out) { g->cond_levelwise = true; count_timeout(ctx); return g->cond_last_rc = gerr(g, CGMR_E_TIMEOUT, "a bounded device-side wait ran out while building a condensed graph"); }
  return g->cond_last_rc = gerr(g, CGMR_E_CHOLESKY_BASE, "Cholesky failed while building a condensed graph");
}

// whatever is about to overwrite my send buffer waits for the robots that are still copying it (cgmr_graph_deliver)
// (a flag per stream that may write the buffer: bit 0 = the context's stream, bit 1 = its side stream; an event wait queued on one
// of them orders nothing on the other)
int wait_consumers(cgmr_graph* g, hipStream_t st) {
  const uint8_t bit = st == g->ctx->stream ? 1 : 2;
  for (size_t d = 0; d < g->consumed_pending.size(); d++)
    if (g->consumed_pending[d] & bit) { HIP_TRY(g->ctx, hipStreamWaitEvent(st, g->ev_consumed[d], 0)); g->consumed_pending[d] &= (uint8_t)~bit; }
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

// Shared tail of the two ingest paths.  per sender s: n_e / n_c and the ids as read from its buffer (ids layout of
// k_wire_read).  Decides what is accepted (mr_graph_slam.cpp:331-395), refreshes the host structure and returns the
// staging slots of the compact second edge segment.
// one sender's part: (from, to) id pairs of its n_e edges, its n_c closure requests
bool ingest_decide_sender(cgmr_graph* g, int s, int n_e, const int32_t* from_to, int n_c, const int32_t* closures) {
  const int cap = g->cap;
  // closure requests: only vertices I have (mr_graph_slam.cpp:336-343); an empty set changes nothing (:345)
  std::vector<int32_t> known;
  for (int k = 0; k < n_c; k++) { const int32_t id = closures[k]; if (g->index.count(id)) known.push_back(id); }
  if (!known.empty()) insert_sorted_unique(g->out_closures[s], known.data(), (int)known.size());
  // edges: both end points must exist (:360-363); the set replaces the previous one only if it is not empty (:393-394)
  PeerIn nw;
  for (int k = 0; k < n_e; k++) {
    auto a = g->index.find(from_to[2 * k]), b = g->index.find(from_to[2 * k + 1]);
    if (a == g->index.end() || b == g->index.end()) continue;
    nw.slot.push_back(s * cap + k);
    nw.from_idx.push_back(a->second);
    nw.to_idx.push_back(b->second);
  }
  if (nw.slot.empty()) return false;
  g->in[s] = std::move(nw);
  return true;
}

void ingest_decide(cgmr_graph* g, const int32_t* ids, std::vector<uint8_t>& accepted) {
  const int R = g->n_robots, cap = g->cap;
  accepted.assign(R, 0);
  for (int s = 0; s < R; s++) {
    if (s == g->robot) continue;
    const int32_t* io = ids + (size_t)s * (2 + 3 * (size_t)cap);
    accepted[s] = ingest_decide_sender(g, s, io[0], io + 2, io[1], io + 2 + 2 * cap) ? 1 : 0;
  }
  rebuild_all_edges(g);
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
    HIP_TRY(ctx, hipSetDevice(ctx->device));
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
    HIP_TRY(ctx, hipSetDevice(ctx->device));
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

// Debugging aid: the level-0 edge list (vertex indices) the solver sees: own edges first, then the received ones.
int cgmr_graph_debug_edges(const cgmr_graph* g, int cap, int32_t* from_out, int32_t* to_out, int32_t* n_own_out) {
  if (!g || cap < 0) return CGMR_E_INVALID;
  const int n = (int)g->all_ef.size();
  for (int k = 0; k < n && k < cap; k++) { from_out[k] = g->all_ef[k]; to_out[k] = g->all_et[k]; }
  if (n_own_out) *n_own_out = (int32_t)g->ef.size();
  return n;
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
  HIP_TRY(ctx, hipSetDevice(ctx->device));
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
  HIP_TRY(ctx, hipSetDevice(ctx->device));
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
    HIP_TRY(ctx, hipSetDevice(ctx->device));
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
    HIP_TRY(ctx, hipSetDevice(ctx->device));
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

}  // extern "C"

namespace {

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
  Ed.meas_a = (const double*)g->d_meas_a.ptr; Ed.info_a = (const double*)g->d_info_a.ptr;
  Ed.meas_b = g->d_meas_b; Ed.info_b = g->d_info_b;
  Ed.nA = B.nA; Ed.n_active = B.nA;                              // getMyEdges: the received edges are switched off
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
  const int32_t* status = (const int32_t*)(B.hstage + B.S.s_st);
  bool failed = false, timed_out = false;
  for (int i = 0; i < nj; i++) { failed = failed || status[4 * i] != 0; timed_out = timed_out || status[4 * i + 2] != 0; }
  if (B.trace) {
    float a = 0, b = 0, c = 0;
    (void)hipEventElapsedTime(&a, B.evs[0], B.evs[1]); (void)hipEventElapsedTime(&b, B.evs[1], B.evs[2]); (void)hipEventElapsedTime(&c, B.evs[2], B.evs[3]);
    fprintf(stderr, "[cond]   device: GN pass %.0f us, marginals %.0f us (m %d, %d levels), labels + wire %.0f us\n", 1e3 * a, 1e3 * b, B.M.m, B.DB.nlevels_full, 1e3 * c);
    fprintf(stderr, "[cond] %d jobs in one batch, nV %d nE %d: structure %.0f us, queueing %.0f us (initial guesses %.0f, masks %.0f, uploads %.0f, GN pass %.0f, marginals + labels %.0f), waiting %.0f us\n",
            nj, B.nV, B.nE, 1e6 * B.t_structure, 1e6 * (t2 - B.t0 - B.t_structure), 1e6 * B.t_guess, 1e6 * B.t_mask, 1e6 * B.t_up, 1e6 * B.t_gn, 1e6 * B.t_marg, 1e6 * (wall_s() - t2));
  }
  if (timed_out) { count_timeout(ctx); return gerr(g, CGMR_E_TIMEOUT, "a bounded device-side wait ran out while building a condensed graph"); }
  if (failed) return gerr(g, CGMR_E_CHOLESKY_BASE, "Cholesky failed while building a condensed graph");
  return 0;
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

}  // namespace

extern "C" {

// CondensedGraphBuffer::computeCondensedGraph(robot, optimal) (condensed_graph_buffer.cpp:437-485) for one peer or, with
// peer < 0, for every peer that has asked for vertices: gauge = selectGaugeCentroid (:318-345) -- or, after
// cgmr_graph_set_optimal_gauge(g, 1), selectOptimalGauge (:252-288: the candidate whose star has the smallest overall
// uncertainty, every candidate's condensed graph being built for that) --, edges = getMyEdges (own edges only),
// CondensedGraphCreator::compute per peer.  The passes of all peers (and of eight gauge candidates at a time) run as
// one batch; the labelled edges land in the send buffer as wire records.  Returns the number of peers built.
}  // extern "C"

namespace {
int compute_condensed_impl(cgmr_graph* g, int peer, bool go_async) {
  if (!g || peer >= g->n_robots) return CGMR_E_INVALID;
  if (!g->ctx) return gerr(g, CGMR_E_NO_DEVICE, "cgmr_graph_compute_condensed: the graph was created without a device context");
  cgmr_ctx* ctx = g->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  {
    // the previous batch, if it was not waited for.  Its failure (Cholesky, time-out) cost its peers that round's edges and is
    // on record (cond_last_rc until the next batch is queued, cgmr_graph_failed_batches); it must not cost them this round's
    // as well: the current batch is built regardless (round 4 returned the old error here and the run stopped)
    const int rc = cond_finish(g);
    if (rc != 0 && rc != CGMR_E_TIMEOUT && rc != CGMR_E_CHOLESKY_BASE) return rc;    // (a HIP error still stops)
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
    if ((int)W.idx.size() - 1 > cap) {                 // more edges than a message holds: nothing would be sent (see fill_header)
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
  if (g && g->ctx && !g->ctx->side_used) { g->ctx->side_used = true; g->ctx->sym_valid = false; }   // (the cached structure's chained solve was sized for the whole device)
  return compute_condensed_impl(g, peer, true);
}

// Wait for the batch queued by cgmr_graph_compute_condensed_async (nothing to wait for: CGMR_OK) and report how it ended.
int cgmr_graph_condensed_wait(cgmr_graph* g) {
  if (!g) return CGMR_E_INVALID;
  if (!g->ctx) return CGMR_OK;
  HIP_TRY(g->ctx, hipSetDevice(g->ctx->device));
  if (g->cond_pending) return cond_finish(g);
  if (g->cond_last_rc) gerr(g, g->cond_last_rc, g->cond_last_rc == CGMR_E_TIMEOUT ? "a bounded device-side wait ran out while building a condensed graph"
                                                                                   : "Cholesky failed while building a condensed graph");
  return g->cond_last_rc;                       // (another call has waited for the batch already: its outcome is kept)
}

// Announce that this graph will use cgmr_graph_compute_condensed_async (call before the first solve: the chained backward
// solves of the context's stream and of the side stream then share the resident workgroups from the start).
int cgmr_graph_set_async(cgmr_graph* g, int on) {
  if (!g) return CGMR_E_INVALID;
  if (g->ctx && on && !g->ctx->side_used) { g->ctx->side_used = true; g->ctx->sym_valid = false; }   // (see cgmr_graph_compute_condensed_async)
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
  if (g->ctx && g->cond_pending) {
    HIP_TRY(g->ctx, hipSetDevice(g->ctx->device));
    int rc = cond_finish(g);
    if (rc) return rc;
  }
  PeerOut& O = g->out[peer];
  const int n = std::min(O.n, cap);
  if (from_id_out) *from_id_out = O.gauge_id;
  if (O.host_valid) {               // set from the host (cgmr_graph_set_condensed): float32 is all there is
    for (int k = 0; k < n; k++) {
      if (to_ids_out) to_ids_out[k] = O.host[k].to;
      if (est_out) for (int a = 0; a < 3; a++) est_out[3 * k + a] = O.host[k].est[a];
      if (info_upper_out) for (int a = 0; a < 6; a++) info_upper_out[6 * k + a] = O.host[k].info[a];
    }
    return O.n;
  }
  if (!g->ctx) return O.n;
  cgmr_ctx* ctx = g->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
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
  if (g->ctx && g->cond_pending) {
    HIP_TRY(g->ctx, hipSetDevice(g->ctx->device));
    int rc = cond_finish(g);
    if (rc) return rc;
  }
  PeerOut& O = g->out[peer];
  O.n = n; O.gauge_id = from_id; O.host.resize(n); O.host_valid = true; O.to_idx.clear();
  for (int k = 0; k < n; k++) {
    O.host[k].from = from_id; O.host[k].to = to_ids[k];
    memcpy(O.host[k].est, est + 3 * k, 12);
    memcpy(O.host[k].info, info_upper + 6 * k, 24);
  }
  if (g->ctx && n > 0) {
    cgmr_ctx* ctx = g->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    WireEdge* dst = reinterpret_cast<WireEdge*>(g->d_send + wire_edges_off(g->n_robots)) + (size_t)g->cap * peer;
    int rcw = wait_consumers(g, ctx->stream);
    if (rcw) return rcw;
    HIP_TRY(ctx, hipMemcpyAsync(dst, O.host.data(), sizeof(WireEdge) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return CGMR_OK;
}

int64_t cgmr_graph_wire_bytes(const cgmr_graph* g) { return g ? (int64_t)wire_bytes(g->n_robots, g->cap) : -1; }

namespace {
// header + closure requests of this robot's wire buffer (host side)
void fill_header(const cgmr_graph* g, unsigned char* buf) {
  const int R = g->n_robots, cap = g->cap;
  int32_t* hdr = reinterpret_cast<int32_t*>(buf);
  hdr[0] = g->robot; hdr[1] = R;
  int32_t* clos = reinterpret_cast<int32_t*>(buf + wire_clos_off(R, cap));
  for (int p = 0; p < R; p++) {
    const std::vector<int32_t>& c = g->in_closures[p];
    // A message that does not fit the wire buffer is not sent at all -- the reference's toCharArray() returns 0 for a
    // message beyond MAX_LENGTH_MSG and GraphComm::send skips it (graph_comm.cpp:112-122, msg_factory.h:115) -- instead
    // of failing the round (every rank still contributes its fixed-size buffer to the all-gather).
    if ((int)c.size() > cap || g->out[p].n > cap) { hdr[2 + p] = 0; hdr[2 + R + p] = 0; continue; }
    hdr[2 + p] = g->out[p].n;
    const int n = (int)c.size();
    hdr[2 + R + p] = n;
    for (int k = 0; k < n; k++) clos[(size_t)p * cap + k] = c[k];
  }
}
// counts the messages fill_header() is about to leave out
void count_skipped(cgmr_graph* g) {
  for (int p = 0; p < g->n_robots; p++)
    if (p != g->robot && ((int)g->in_closures[p].size() > g->cap || g->out[p].n > g->cap)) g->skipped_messages++;
}
}  // namespace

// Serialise this robot's round message (ComboMessage of condensed edges + closure requests, mr_graph_slam.cpp:527-562,
// 607-670) into a device buffer of cgmr_graph_wire_bytes() bytes.  The edges are already in the graph's send buffer as
// wire records (cgmr_graph_compute_condensed writes them there); the header and the request lists -- host bookkeeping --
// are staged through pinned memory.  d_send_out may be NULL: the graph's own send buffer is then the message.
int cgmr_graph_pack(cgmr_graph* g, void* d_send_out) {
  if (!g) return CGMR_E_INVALID;
  if (!g->ctx) return gerr(g, CGMR_E_NO_DEVICE, "cgmr_graph_pack: no device context (use cgmr_graph_pack_host)");
  cgmr_ctx* ctx = g->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int R = g->n_robots, cap = g->cap;
  count_skipped(g);
  const size_t wb = wire_bytes(R, cap);
  // the pinned staging may still be in flight from the last round (its own event: no wait for the stream's other work)
  if (g->pack_in_flight) { HIP_TRY(ctx, hipEventSynchronize(g->ev_pack)); g->pack_in_flight = false; }
  // A batch of condensed graphs that has not been waited for is still writing its edges into the send buffer: the message
  // is completed on the side stream, behind it, with the counts the batch WILL produce -- and a kernel that takes them
  // back for the batch's peers should one of its passes have failed (what the synchronous path decides on the host).
  const bool behind_batch = g->cond_pending;
  hipStream_t st = ctx->stream;
  if (behind_batch) {
    int rc = side_stream(ctx);
    if (rc) return rc;
    st = ctx->side;
  }
  {
    int rc = wait_consumers(g, st);
    if (rc) return rc;
  }
  memset(g->pinned, 0, wb);
  fill_header(g, (unsigned char*)g->pinned);
  HIP_TRY(ctx, hipMemcpyAsync(g->d_send, g->pinned, wire_edges_off(R), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(g->d_send + wire_clos_off(R, cap), g->pinned + wire_clos_off(R, cap), (size_t)R * cap * 4,
                              hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(g->ev_pack, st));
  g->pack_in_flight = true;
  if (behind_batch)
    launch_wire_fix_counts(st, (int32_t*)g->d_send, R, (int)g->cond_peers.size(), g->cond_jobs_dev, g->cond_status_dev, g->cond_status_stride);
  if (d_send_out && d_send_out != (void*)g->d_send)
    HIP_TRY(ctx, hipMemcpyAsync(d_send_out, g->d_send, wb, hipMemcpyDeviceToDevice, st));
  HIP_TRY(ctx, hipEventRecord(g->ev_packed, st));
  g->n_packed++;
  if (behind_batch) {
    int rc = side_mark(ctx);
    if (rc) return rc;
  }
  return CGMR_OK;
}

// Peer access from `dev` to `peer`, asked for and switched on ONCE per pair and process (the answer is kept: round 5 asked the
// runtime on every cross-device delivery).  Returns true when dev reads peer's memory directly; false is not an error --
// hipMemcpyPeerAsync then goes through the host.  The caller has made `dev` current.
static bool peer_access_once(int dev, int peer) {
  constexpr int kMaxDev = 64;
  static std::mutex mu;
  static signed char state[kMaxDev][kMaxDev];            // 0: not asked yet, 1: direct, -1: no peer access
  if (dev < 0 || peer < 0 || dev >= kMaxDev || peer >= kMaxDev) return false;
  std::lock_guard<std::mutex> lk(mu);
  if (state[dev][peer] == 0) {
    int can = 0;
    bool ok = hipDeviceCanAccessPeer(&can, dev, peer) == hipSuccess && can;
    if (ok) {
      const hipError_t pe = hipDeviceEnablePeerAccess(peer, 0);
      ok = pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled;
    }
    (void)hipGetLastError();
    state[dev][peer] = ok ? 1 : -1;
  }
  return state[dev][peer] == 1;
}

// In-process transport for robots that share a device (loopback runs, several robots of one node in one process): src's
// packed message (cgmr_graph_pack(src, NULL) before this) goes into slot src->robot of one of dst's two receive buffers
// (the k-th message for dst into buffer k & 1), a device copy on dst's stream behind src's pack -- what the all-gather does
// between ranks.  Nothing waits on the host; dst's k-th cgmr_graph_ingest_delivered is ordered behind the copy, src's next
// write into its send buffer behind it as well.  Every robot delivers to every other once per round.
int cgmr_graph_deliver(cgmr_graph* src, cgmr_graph* dst) {
  if (!src || !dst || !src->ctx || !dst->ctx || src->n_robots != dst->n_robots || src->cap != dst->cap) return CGMR_E_INVALID;
  if (src == dst || src->robot == dst->robot) return gerr(src, CGMR_E_INVALID, "cgmr_graph_deliver: a robot does not deliver to itself");
  if (src->n_packed == 0) return gerr(src, CGMR_E_INVALID, "cgmr_graph_deliver: nothing packed yet (cgmr_graph_pack(src, NULL) first)");
  cgmr_ctx* ctx = dst->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool cross = src->ctx->device != ctx->device;
  if (cross) (void)peer_access_once(ctx->device, src->ctx->device);   // direct when the devices reach each other, staged by the runtime when not
  const size_t wb = wire_bytes(src->n_robots, src->cap);
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, src->ev_packed, 0));
  // two receive buffers taking turns: a robot may deliver its round-t message before the destination has ingested round t - 1's
  // (robots that take turns on one device run their rounds one after the other, not in lock step).  The k-th delivery of src to
  // dst belongs to dst's k-th cgmr_graph_ingest_delivered; which delivery lies in which buffer is kept on the host, and a
  // buffer whose slice is not the expected one (a robot skipped a round, delivered twice, ..) is ingested as "no message"
  const int64_t k = src->n_delivered[dst->robot];
  unsigned char* recv = (k & 1) ? dst->d_recv2 : dst->d_recv;
  if (cross)
    HIP_TRY(ctx, hipMemcpyPeerAsync(recv + (size_t)src->robot * wb, ctx->device, src->d_send, src->ctx->device, wb, ctx->stream));
  else
    HIP_TRY(ctx, hipMemcpyAsync(recv + (size_t)src->robot * wb, src->d_send, wb, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(src->ev_consumed[dst->robot], ctx->stream));
  src->n_delivered[dst->robot] = k + 1;                      // (only now: the copy is queued)
  dst->recv_round[k & 1][src->robot] = k;
  src->consumed_pending[dst->robot] = 3;                     // both of src's streams wait before they write the buffer again
  return CGMR_OK;
}

int64_t cgmr_graph_skipped_messages(const cgmr_graph* g) { return g ? g->skipped_messages : -1; }
int64_t cgmr_graph_failed_batches(const cgmr_graph* g) { return g ? g->cond_failed_batches : -1; }

void* cgmr_graph_send_buffer(cgmr_graph* g) { return g ? (void*)g->d_send : nullptr; }
void* cgmr_graph_recv_buffer(cgmr_graph* g) { return g ? (void*)g->d_recv : nullptr; }

// Host-memory variant (gloo / CPU tests): with a device context the device message is copied out, without one the
// message is built from the host copies of the condensed graphs (cgmr_graph_set_condensed).
int cgmr_graph_pack_host(cgmr_graph* g, void* send_out) {
  if (!g || !send_out) return CGMR_E_INVALID;
  const int R = g->n_robots, cap = g->cap;
  const size_t wb = wire_bytes(R, cap);
  if (g->ctx) {
    HIP_TRY(g->ctx, hipSetDevice(g->ctx->device));
    int rc = cond_finish(g);
    if (rc && rc != CGMR_E_CHOLESKY_BASE && rc != CGMR_E_TIMEOUT) return rc;     // (a failed batch: its peers get no edges, the message still goes out)
    rc = cgmr_graph_pack(g, nullptr);
    if (rc) return rc;
    cgmr_ctx* ctx = g->ctx;
    HIP_TRY(ctx, hipMemcpyAsync(send_out, g->d_send, wb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CGMR_OK;
  }
  count_skipped(g);
  for (int p = 0; p < R; p++)
    if (g->out[p].n > 0 && !g->out[p].host_valid) return gerr(g, CGMR_E_INVALID, "condensed graph not available on the host");
  unsigned char* buf = (unsigned char*)send_out;
  memset(buf, 0, wb);
  fill_header(g, buf);
  WireEdge* edges = reinterpret_cast<WireEdge*>(buf + wire_edges_off(R));
  for (int p = 0; p < R; p++)
    for (int k = 0; k < g->out[p].n && k < cap; k++) edges[(size_t)p * cap + k] = g->out[p].host[k];
  return CGMR_OK;
}

// MRGraphSLAM::addInterRobotData for the messages of all robots at once (mr_graph_slam.cpp:331-395): d_recv holds the
// n_robots wire buffers in rank order (the all-gather's output).  Closure requests become out-closures; the edges
// addressed to me whose end points I know replace the set previously received from that robot
// (CondensedGraphBuffer::insertEdgesFromRobot, condensed_graph_buffer.cpp:487-510) -- an empty or fully unknown set
// leaves the previous one in place (mr_graph_slam.cpp:393-394).  Numeric payload stays on the device (float32 ->
// double, staging -> compact second edge segment); only ids and counts travel to the host.
// n_edges_out (nullable) [n_robots]: accepted edges per sender this round (0 = nothing replaced).
// skip_senders: bit s set = sender s has no message in this round whatever its slice of the buffer holds (the slice is left
// alone: cgmr_graph_ingest_delivered below, a delivery that waits for a later round)
static int graph_ingest_core(cgmr_graph* g, const void* d_recv, int32_t* n_edges_out, unsigned long long skip_senders) {
  if (!g) return CGMR_E_INVALID;
  if (!g->ctx) return gerr(g, CGMR_E_NO_DEVICE, "cgmr_graph_ingest: no device context (use cgmr_graph_ingest_host)");
  cgmr_ctx* ctx = g->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int R = g->n_robots, cap = g->cap;
  const size_t wb = wire_bytes(R, cap), ids_bytes = 4 * (size_t)R * (2 + 3 * (size_t)cap);
  const unsigned char* recv = d_recv ? (const unsigned char*)d_recv : g->d_recv;
  g->msg_in_flight = false;            // (the synchronisation below covers a message's uploads: same stream)
  launch_wire_read(st, R, cap, g->robot, wb, recv, g->d_tmp_meas, g->d_tmp_info, g->d_ids_out);
  char* h_ids = g->pinned + round256(wb);
  HIP_TRY(ctx, hipMemcpyAsync(h_ids, g->d_ids_out, ids_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int s = 0; s < R && skip_senders; s++)
    if (s < 64 && ((skip_senders >> s) & 1)) {                    // no edges, no closure requests from this sender this round
      int32_t* io = (int32_t*)h_ids + (size_t)s * (2 + 3 * (size_t)cap);
      io[0] = 0; io[1] = 0;
    }
  std::vector<uint8_t> accepted;
  ingest_decide(g, (const int32_t*)h_ids, accepted);
  unsigned long long fresh = 0;                                   // senders whose message replaced their previous set (R <= 64)
  for (int s = 0; s < R; s++) {
    if (n_edges_out) n_edges_out[s] = accepted[s] ? (int32_t)g->in[s].slot.size() : 0;
    if (!accepted[s]) continue;
    g->hs_fresh[s] = 0;
    fresh |= 1ULL << s;
  }
  int32_t* h_slot = (int32_t*)(g->pinned + round256(wb) + round256(ids_bytes));
  int j = 0;
  for (int s = 0; s < R; s++) for (int32_t sl : g->in[s].slot) h_slot[j++] = sl;
  if (j > 0) {
    // one launch: the accepted senders' records move from the widened wire data into the staging and, with the sets kept
    // from earlier rounds, into the compact second edge segment (two device copies per accepted sender + a gather before)
    HIP_TRY(ctx, hipMemcpyAsync(g->d_slot, h_slot, 4 * (size_t)j, hipMemcpyHostToDevice, st));
    launch_accept_gather_edges(st, j, cap, fresh, g->d_slot, g->d_tmp_meas, g->d_tmp_info, g->d_stage_meas, g->d_stage_info, g->d_meas_b,
                               g->d_info_b);
  }
  return CGMR_OK;
}

int cgmr_graph_ingest(cgmr_graph* g, const void* d_recv, int32_t* n_edges_out) { return graph_ingest_core(g, d_recv, n_edges_out, 0); }

// The ingest that goes with cgmr_graph_deliver: the k-th call digests the k-th message of every peer (receive buffer k & 1).
int cgmr_graph_ingest_delivered(cgmr_graph* g, int32_t* n_edges_out) {
  if (!g || !g->ctx) return CGMR_E_INVALID;
  const int64_t k = g->n_ingested_delivered;
  unsigned char* recv = (k & 1) ? g->d_recv2 : g->d_recv;
  // a sender whose k-th delivery is not what lies in this buffer (it skipped a round, or is a round ahead or behind) has no
  // message in this round: its slice's header is cleared instead of being ingested stale (the sender id of a cleared slice is
  // -1, which k_wire_read / the host mirror reject)
  cgmr_ctx* ctx = g->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t wb = wire_bytes(g->n_robots, g->cap);
  // A sender that is two (four, ..) rounds AHEAD has already put a later delivery into this buffer (over the k-th one, which is
  // lost): that message belongs to a later ingest -- the sender has no message in this round, and neither the slice nor the
  // note of what lies in it is touched (round 5 cleared both: two rounds lost where one was missed).
  unsigned long long skip = 0;
  for (int s = 0; s < g->n_robots; s++) {
    if (s == g->robot) continue;
    const int64_t have = g->recv_round[k & 1][s];
    if (have > k) { if (s < 64) skip |= 1ULL << s; continue; }
    if (have != k) HIP_TRY(ctx, hipMemsetAsync(recv + (size_t)s * wb, 0xff, 4, ctx->stream));
    g->recv_round[k & 1][s] = -1;
  }
  g->n_ingested_delivered = k + 1;
  return graph_ingest_core(g, recv, n_edges_out, skip);
}

int cgmr_graph_ingest_host(cgmr_graph* g, const void* recv, int32_t* n_edges_out) {
  if (!g || !recv) return CGMR_E_INVALID;
  const int R = g->n_robots, cap = g->cap;
  const size_t wb = wire_bytes(R, cap);
  if (g->ctx) {
    cgmr_ctx* ctx = g->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(g->d_recv, recv, (size_t)R * wb, hipMemcpyHostToDevice, ctx->stream));
    return cgmr_graph_ingest(g, nullptr, n_edges_out);
  }
  // host-only mirror of k_wire_read + the staging copies
  std::vector<int32_t> ids((size_t)R * (2 + 3 * (size_t)cap), 0);
  std::vector<double> tm(3 * (size_t)R * cap), ti(6 * (size_t)R * cap);
  for (int s = 0; s < R; s++) {
    const unsigned char* buf = (const unsigned char*)recv + (size_t)s * wb;
    const int32_t* hdr = (const int32_t*)buf;
    int32_t* io = ids.data() + (size_t)s * (2 + 3 * (size_t)cap);
    const bool ok = hdr[0] == s && s != g->robot;
    const int n_e = std::min(std::max(hdr[2 + g->robot], 0), cap), n_c = std::min(std::max(hdr[2 + R + g->robot], 0), cap);
    io[0] = ok ? n_e : 0; io[1] = ok ? n_c : 0;
    const WireEdge* e = (const WireEdge*)(buf + wire_edges_off(R)) + (size_t)g->robot * cap;
    const int32_t* c = (const int32_t*)(buf + wire_clos_off(R, cap)) + (size_t)g->robot * cap;
    for (int k = 0; k < n_e; k++) {
      io[2 + 2 * k] = e[k].from; io[2 + 2 * k + 1] = e[k].to;
      for (int a = 0; a < 3; a++) tm[3 * ((size_t)s * cap + k) + a] = (double)e[k].est[a];
      for (int a = 0; a < 6; a++) ti[6 * ((size_t)s * cap + k) + a] = (double)e[k].info[a];
    }
    for (int k = 0; k < n_c; k++) io[2 + 2 * cap + k] = c[k];
  }
  std::vector<uint8_t> accepted;
  ingest_decide(g, ids.data(), accepted);
  for (int s = 0; s < R; s++) {
    if (n_edges_out) n_edges_out[s] = accepted[s] ? (int32_t)g->in[s].slot.size() : 0;
    if (!accepted[s]) continue;
    memcpy(g->hs_meas.data() + 3 * (size_t)s * cap, tm.data() + 3 * (size_t)s * cap, 24 * (size_t)cap);
    memcpy(g->hs_info.data() + 6 * (size_t)s * cap, ti.data() + 6 * (size_t)s * cap, 48 * (size_t)cap);
  }
  return CGMR_OK;
}

// MRGraphSLAM::constructCondensedGraphMessage(idRobotTo) (mr_graph_slam.cpp:607-670): the part of this robot's round
// message that is addressed to ONE peer, as the reference's CondensedGraphMessage carries it -- the condensed edges built
// for `peer` in wire precision (44 bytes each) and the ids of `peer`'s vertices this robot wants condensed in return.
// Returns 1 if there is a message (a closure list for the peer exists or there are edges, :664-667), 0 if not.
int cgmr_graph_message_for(cgmr_graph* g, int peer, int cap_edges, void* edges44_out, int32_t* n_edges_out, int cap_closures,
                           int32_t* closure_ids_out, int32_t* n_closures_out) {
  if (!g || peer < 0 || peer >= g->n_robots || cap_edges < 0 || cap_closures < 0 || !n_edges_out || !n_closures_out)
    return CGMR_E_INVALID;
  const int R = g->n_robots, cap = g->cap;
  if (g->ctx && g->cond_pending) {
    HIP_TRY(g->ctx, hipSetDevice(g->ctx->device));
    int rc = cond_finish(g);
    if (rc) return rc;
  }
  // one peer's part of the round message: the counts and the closure requests are host bookkeeping (what fill_header()
  // writes), the edges are this peer's slice of the send buffer -- on the device when there is one: only that slice comes
  // back (round 2 packed and downloaded the whole buffer, 400 KB for four robots, for every peer and tick)
  const std::vector<int32_t>& cl = g->in_closures[peer];
  // This message travels as the reference's byte string, so the reference's limit holds for it besides the slice capacity:
  // header, two counters, 44 bytes per edge and 4 per closure id must fit MAX_LENGTH_MSG as a whole (at cap = 2270 the
  // edges alone nearly fill it: 2270 edges leave room for 24 ids).  A message beyond either limit is not sent -- no
  // message, one count -- as GraphComm::send skips a message whose toCharArray returned 0 (graph_comm.cpp:112-122).
  const bool skip = (int)cl.size() > cap || g->out[peer].n > cap ||
                    condensed_message_bytes(g->out[peer].n, (int)cl.size()) > kMaxLengthMsg;
  if (skip) {
    if (peer != g->robot) g->skipped_messages++;
    *n_edges_out = 0;
    *n_closures_out = 0;
    return 0;
  }
  const int n_e = g->out[peer].n, n_c = (int)cl.size();
  if (n_e > cap_edges || n_c > cap_closures) return gerr(g, CGMR_E_INVALID, "cgmr_graph_message_for: output capacity too small");
  if (n_e > 0 && !edges44_out) return CGMR_E_INVALID;
  if (n_c > 0 && !closure_ids_out) return CGMR_E_INVALID;
  if (n_e > 0) {
    if (g->ctx) {
      cgmr_ctx* ctx = g->ctx;
      HIP_TRY(ctx, hipSetDevice(ctx->device));
      const WireEdge* src = reinterpret_cast<const WireEdge*>(g->d_send + wire_edges_off(R)) + (size_t)cap * peer;
      HIP_TRY(ctx, hipMemcpyAsync(edges44_out, src, (size_t)n_e * sizeof(WireEdge), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    } else {
      if (!g->out[peer].host_valid) return gerr(g, CGMR_E_INVALID, "condensed graph not available on the host");
      memcpy(edges44_out, g->out[peer].host.data(), (size_t)n_e * sizeof(WireEdge));
    }
  }
  if (n_c > 0) memcpy(closure_ids_out, cl.data(), (size_t)n_c * 4);
  *n_edges_out = n_e;
  *n_closures_out = n_c;
  return (n_e > 0 || !g->in_closures[peer].empty()) ? 1 : 0;
}

// MRGraphSLAM::addInterRobotData(CondensedGraphMessage*) (mr_graph_slam.cpp:331-395) for ONE message: the closure requests
// for vertices this robot has become out-closures and the condensed graph for `sender` is rebuilt at once (:345-348); the
// edges whose end points exist replace the set previously received from `sender`, unless none survives (:393-394).
// n_accepted_out (nullable): edges now held from `sender` because of this message (0 = previous set kept).
int cgmr_graph_message_from(cgmr_graph* g, int sender, int n_edges, const void* edges44, int n_closures,
                            const int32_t* closure_ids, int32_t* n_accepted_out) {
  if (!g || sender < 0 || sender >= g->n_robots || sender == g->robot || n_edges < 0 || n_closures < 0 ||
      (n_edges > 0 && !edges44) || (n_closures > 0 && !closure_ids))
    return CGMR_E_INVALID;
  const int R = g->n_robots, cap = g->cap;
  if (n_edges > cap || n_closures > cap) {           // beyond what a reference node's receive buffer holds: dropped, not an error
    g->skipped_messages++;
    if (n_accepted_out) *n_accepted_out = 0;
    return CGMR_OK;
  }
  const size_t wb = wire_bytes(R, cap);
  bool any_known = false;
  for (int k = 0; k < n_closures; k++) any_known = any_known || g->index.count(closure_ids[k]);
  std::vector<int32_t> acc(R, 0);
  int rc;
  if (g->ctx) {
    // One message: the host holds everything the decision needs (the end point ids are in the wire records), and widening
    // 9 floats per edge is no work for it.  So nothing is read back: the accepted set's numbers go to the sender's staging
    // slots (and to the host mirror of the staging), the slot list of the compact second segment follows, the gather is
    // queued behind them -- no synchronisation.  (Round 2 built and uploaded the whole receive buffer, 1.7 MB for four
    // robots, for every message; until the end of round 3 the message went through k_wire_read with a 109 KB read-back of
    // ids per message: 156 us per call in the C4 leg.)
    cgmr_ctx* ctx = g->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<int32_t> ft(2 * (size_t)n_edges);
    const unsigned char* eb = (const unsigned char*)edges44;
    for (int k = 0; k < n_edges; k++) memcpy(&ft[2 * (size_t)k], eb + (size_t)k * sizeof(WireEdge), 8);   // from, to lead the record
    static_assert(offsetof(WireEdge, from) == 0 && offsetof(WireEdge, to) == 4, "wire record layout");
    const bool ok = ingest_decide_sender(g, sender, n_edges, ft.data(), n_closures, closure_ids);
    rebuild_all_edges(g);
    acc[sender] = ok ? (int32_t)g->in[sender].slot.size() : 0;
    if (ok) {
      if (g->msg_in_flight) { HIP_TRY(ctx, hipEventSynchronize(g->ev_msg)); g->msg_in_flight = false; }
      double* pm = (double*)(g->pinned + g->pinned_msg_off);
      double* pi = pm + 3 * (size_t)cap;
      for (int k = 0; k < n_edges; k++) {
        WireEdge w;
        memcpy(&w, eb + (size_t)k * sizeof(WireEdge), sizeof w);
        for (int a = 0; a < 3; a++) pm[3 * (size_t)k + a] = (double)w.est[a];
        for (int a = 0; a < 6; a++) pi[6 * (size_t)k + a] = (double)w.info[a];
      }
      memcpy(g->hs_meas.data() + 3 * (size_t)sender * cap, pm, 24 * (size_t)n_edges);
      memcpy(g->hs_info.data() + 6 * (size_t)sender * cap, pi, 48 * (size_t)n_edges);
      g->hs_fresh[sender] = 1;
      HIP_TRY(ctx, hipMemcpyAsync(g->d_stage_meas + 3 * (size_t)sender * cap, pm, 24 * (size_t)n_edges, hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(g->d_stage_info + 6 * (size_t)sender * cap, pi, 48 * (size_t)n_edges, hipMemcpyHostToDevice, st));
      int32_t* h_slot = (int32_t*)(g->pinned + round256(wb) + round256(4 * (size_t)R * (2 + 3 * (size_t)cap)));
      int j = 0;
      for (int s = 0; s < R; s++) for (int32_t sl : g->in[s].slot) h_slot[j++] = sl;
      HIP_TRY(ctx, hipMemcpyAsync(g->d_slot, h_slot, 4 * (size_t)j, hipMemcpyHostToDevice, st));
      launch_gather_edges(st, j, g->d_slot, g->d_stage_meas, g->d_stage_info, g->d_meas_b, g->d_info_b);
      HIP_TRY(ctx, hipEventRecord(g->ev_msg, st));
      g->msg_in_flight = true;
    }
    rc = CGMR_OK;
  } else {
    std::vector<unsigned char> buf((size_t)R * wb, 0);
    for (int s = 0; s < R; s++) {                               // every block needs its sender id; only one carries data
      int32_t* h = reinterpret_cast<int32_t*>(buf.data() + (size_t)s * wb);
      h[0] = s; h[1] = R;
    }
    unsigned char* blk = buf.data() + (size_t)sender * wb;
    int32_t* hdr = reinterpret_cast<int32_t*>(blk);
    hdr[2 + g->robot] = n_edges;
    hdr[2 + R + g->robot] = n_closures;
    if (n_edges) memcpy(blk + wire_edges_off(R) + (size_t)g->robot * cap * sizeof(WireEdge), edges44, (size_t)n_edges * sizeof(WireEdge));
    if (n_closures) memcpy(blk + wire_clos_off(R, cap) + (size_t)g->robot * cap * 4, closure_ids, (size_t)n_closures * 4);
    rc = cgmr_graph_ingest_host(g, buf.data(), acc.data());
  }
  if (rc) return rc;
  if (n_accepted_out) *n_accepted_out = acc[sender];
  if (any_known && g->ctx) {
    rc = cgmr_graph_compute_condensed(g, sender);
    if (rc < 0) return rc;
  }
  return CGMR_OK;
}

// The edges currently held from `peer` (the second edge segment's slice): end point ids, measurement, information
int cgmr_graph_received_edges(cgmr_graph* g, int peer, int cap, int32_t* from_ids_out, int32_t* to_ids_out, double* meas_out,
                              double* info_upper_out) {
  if (!g || peer < 0 || peer >= g->n_robots || cap < 0) return CGMR_E_INVALID;
  const PeerIn& I = g->in[peer];
  const int n = std::min((int)I.slot.size(), cap);
  for (int k = 0; k < n; k++) {
    if (from_ids_out) from_ids_out[k] = g->ids[I.from_idx[k]];
    if (to_ids_out) to_ids_out[k] = g->ids[I.to_idx[k]];
  }
  if ((meas_out || info_upper_out) && n > 0) {
    if (g->ctx && !g->hs_fresh[peer]) {
      cgmr_ctx* ctx = g->ctx;
      HIP_TRY(ctx, hipSetDevice(ctx->device));
      // (a set that arrived through cgmr_graph_message_from is mirrored on the host: nothing to fetch)
      // only the staging slots this peer's edges occupy (round 2 fetched the staging of all peers: 650 KB per call at the
      // reference's capacity)
      size_t lo = (size_t)I.slot[0], hi = (size_t)I.slot[0] + 1;
      for (int k = 1; k < (int)I.slot.size(); k++) { lo = std::min(lo, (size_t)I.slot[k]); hi = std::max(hi, (size_t)I.slot[k] + 1); }
      HIP_TRY(ctx, hipMemcpyAsync(g->hs_meas.data() + 3 * lo, g->d_stage_meas + 3 * lo, 24 * (hi - lo), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(g->hs_info.data() + 6 * lo, g->d_stage_info + 6 * lo, 48 * (hi - lo), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int k = 0; k < n; k++) {
      if (meas_out) memcpy(meas_out + 3 * k, g->hs_meas.data() + 3 * (size_t)I.slot[k], 24);
      if (info_upper_out) memcpy(info_upper_out + 6 * k, g->hs_info.data() + 6 * (size_t)I.slot[k], 48);
    }
  }
  return (int)I.slot.size();
}

// Test support: the compact second edge segment as the solver reads it (what k_accept_gather_edges / k_gather_edges wrote),
// peer order -- the order of cgmr_graph_debug_edges behind the own edges.  cgmr_graph_received_edges reads the staging.
int cgmr_graph_debug_received_segment(cgmr_graph* g, int cap, double* meas_out, double* info_upper_out) {
  if (!g || cap < 0) return CGMR_E_INVALID;
  if (!g->ctx) return gerr(g, CGMR_E_NO_DEVICE, "cgmr_graph_debug_received_segment: no device context");
  cgmr_ctx* ctx = g->ctx;
  const int n = std::min(g->nB, cap);
  if (n > 0 && (meas_out || info_upper_out)) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (meas_out) HIP_TRY(ctx, hipMemcpyAsync(meas_out, g->d_meas_b, 24 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (info_upper_out) HIP_TRY(ctx, hipMemcpyAsync(info_upper_out, g->d_info_b, 48 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return g->nB;
}

namespace {
struct ScratchDev {                   // device scratch of one test-support call
  std::vector<void*> blocks;
  ~ScratchDev() { for (void* p : blocks) (void)hipFree(p); }
  void* alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max(bytes, (size_t)16)) != hipSuccess) return nullptr;
    blocks.push_back(p);
    return p;
  }
  // a copy of `bytes` host bytes on the device
  void* up(cgmr_ctx* ctx, const void* host, size_t bytes) {
    void* p = alloc(bytes);
    if (p && bytes && hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return nullptr;
    return p;
  }
};
}  // namespace

// Test support: k_wire_write_edges on host data.  The kernel only ever sees solver output; this is the way in for values
// the solver never produces (float32 subnormals, ties, overflow).  Every index is checked here: the kernel checks none.
int cgmr_wire_narrow_edges(cgmr_ctx* ctx, int n, int32_t from_id, const int32_t* to_vertex, int n_vertices, const int32_t* vertex_ids,
                           const double* est, const double* info_upper, void* edges44_out) {
  if (!ctx || n < 0 || n_vertices < 0 || (n > 0 && (!to_vertex || !vertex_ids || !est || !info_upper || !edges44_out)))
    return CGMR_E_INVALID;
  for (int k = 0; k < n; k++)
    if (to_vertex[k] < 0 || to_vertex[k] >= n_vertices) return set_err(ctx, CGMR_E_INVALID, "cgmr_wire_narrow_edges: vertex index out of range");
  if (n == 0) return CGMR_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ScratchDev S;
  void* d_to = S.up(ctx, to_vertex, 4 * (size_t)n);
  void* d_ids = S.up(ctx, vertex_ids, 4 * (size_t)n_vertices);
  void* d_est = S.up(ctx, est, 24 * (size_t)n);
  void* d_info = S.up(ctx, info_upper, 48 * (size_t)n);
  void* d_out = S.alloc(sizeof(WireEdge) * (size_t)n);
  if (!d_to || !d_ids || !d_est || !d_info || !d_out) return set_err(ctx, CGMR_E_ALLOC, "cgmr_wire_narrow_edges: device scratch");
  launch_wire_write_edges(ctx->stream, n, from_id, (const int32_t*)d_to, (const int32_t*)d_ids, (const double*)d_est, (const double*)d_info,
                          (WireEdge*)d_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(edges44_out, d_out, sizeof(WireEdge) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CGMR_OK;
}

// The batched form, as a batch of condensed-graph passes launches it: job j reads its vertex indices at to_vertex + j * marg_stride
// bytes, and -- by its OUTPUT SLOT -- est / info at out_slot[j] * est_stride / info_stride bytes, and writes nq[j] records at
// wire_inout + out_slot[j] * wire_stride bytes.  to_vertex holds njobs * marg_stride bytes, est / info / wire_inout n_slots strides
// each; wire_inout goes to the device as it is and comes back whole (what the kernel must not touch keeps the caller's bytes).
int cgmr_wire_narrow_edges_batched(cgmr_ctx* ctx, int njobs, const int32_t* nq, const int32_t* gauge_id, const int32_t* out_slot, int n_slots,
                                   long long marg_stride, long long est_stride, long long info_stride, long long wire_stride,
                                   const void* to_vertex, int n_vertices, const int32_t* vertex_ids, const void* est, const void* info_upper,
                                   void* wire_inout) {
  if (!ctx || njobs < 1 || n_slots < 1 || n_vertices < 0 || !nq || !gauge_id || !out_slot || !to_vertex || !vertex_ids || !est ||
      !info_upper || !wire_inout || marg_stride < 4 || est_stride < 8 || info_stride < 8 || wire_stride < 4 || marg_stride % 4 ||
      est_stride % 8 || info_stride % 8 || wire_stride % 4)
    return CGMR_E_INVALID;
  int nmax = 0;
  std::vector<CondJobDev> jobs(njobs);
  for (int j = 0; j < njobs; j++) {
    const long long q = nq[j];
    if (q < 0 || out_slot[j] < 0 || out_slot[j] >= n_slots || 4 * q > marg_stride || 24 * q > est_stride || 48 * q > info_stride ||
        (long long)sizeof(WireEdge) * q > wire_stride)
      return set_err(ctx, CGMR_E_INVALID, "cgmr_wire_narrow_edges_batched: job %d does not fit its strides", j);
    const int32_t* tv = (const int32_t*)((const char*)to_vertex + (long long)j * marg_stride);
    for (int k = 0; k < q; k++)
      if (tv[k] < 0 || tv[k] >= n_vertices) return set_err(ctx, CGMR_E_INVALID, "cgmr_wire_narrow_edges_batched: vertex index out of range");
    jobs[j] = CondJobDev{nq[j], 0, gauge_id[j], out_slot[j]};
    nmax = std::max(nmax, nq[j]);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ScratchDev S;
  void* d_jobs = S.up(ctx, jobs.data(), sizeof(CondJobDev) * (size_t)njobs);
  void* d_to = S.up(ctx, to_vertex, (size_t)njobs * (size_t)marg_stride);
  void* d_ids = S.up(ctx, vertex_ids, 4 * (size_t)n_vertices);
  void* d_est = S.up(ctx, est, (size_t)n_slots * (size_t)est_stride);
  void* d_info = S.up(ctx, info_upper, (size_t)n_slots * (size_t)info_stride);
  void* d_out = S.up(ctx, wire_inout, (size_t)n_slots * (size_t)wire_stride);
  if (!d_jobs || !d_to || !d_ids || !d_est || !d_info || !d_out) return set_err(ctx, CGMR_E_ALLOC, "cgmr_wire_narrow_edges_batched: device scratch");
  MargBatch mb;
  mb.jobs = (const CondJobDev*)d_jobs;
  mb.marg_stride = marg_stride; mb.est_stride = est_stride; mb.info_stride = info_stride; mb.wire_stride = wire_stride;
  launch_wire_write_edges(ctx->stream, nmax, 0, (const int32_t*)d_to, (const int32_t*)d_ids, (const double*)d_est, (const double*)d_info,
                          (WireEdge*)d_out, njobs, &mb);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(wire_inout, d_out, (size_t)n_slots * (size_t)wire_stride, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CGMR_OK;
}

int cgmr_graph_last_seconds(const cgmr_graph* g, double out[2]) {
  if (!g || !out) return CGMR_E_INVALID;
  out[0] = g->last_optimize_seconds; out[1] = g->last_condense_seconds;
  return CGMR_OK;
}

}  // extern "C"
