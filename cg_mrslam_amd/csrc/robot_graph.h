// The robot graph (include/cgmr.h, "robot graph" and "exchange") as its host layer's translation units share it: the struct, and
// the helpers more than one of them calls.
//   robot_graph.cpp      create / destroy, growth, poses, closure lists, robust and GNC settings, the optimisers' entry points
//   condensed_host.cpp   the condensed-graph batches: gauges, staging, the launches, how a batch ends
//   exchange_host.cpp    pack, the in-process transport, the ingests, the one-peer messages, what was received
//   cgmr_debug.cpp       the test hooks (cgmr_graph_debug_*, cgmr_wire_narrow_edges*)
// The wire geometry -- buffer offsets, the ids read-back, the rule for a message that is not sent -- is in wire_format.h only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <unordered_map>
#include <mutex>
#include <string>
#include <vector>

#include "cgmr_ctx.h"
#include "gn_host.h"
#include "gnc_device.h"
#include "mrslam_device.h"

namespace cgmr {

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

// The graph's pinned block: a rank's wire buffer (header + closures staging), the ids read-back of k_wire_read, the flattened
// slot list of all peers, one message's widened numbers (cap measurements, then cap information matrices)
struct PinnedLayout {
  size_t wire = 0, ids = 0, slot = 0, msg = 0, bytes = 0;
};

}  // namespace cgmr

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
  std::vector<cgmr::PeerIn> in;             // per peer
  std::vector<cgmr::PeerOut> out;           // per peer
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
  cgmr::DevBuf d_poses, d_meas_a, d_info_a, d_vids;
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
  cgmr::PinnedLayout pin;            // where those lie in it (alloc_fixed)
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
  cgmr::DevBuf d_rk_kind, d_rk_delta;
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
  cgmr::DevBuf d_gnc_w;                     // the weights of a keep_gnc_weights solve: own edges, then ones for the received
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
  const cgmr::CondJobDev* cond_jobs_dev = nullptr;    // the batch's job table on the device (peer of job j = out_slot)
  const int* cond_status_dev = nullptr;         // first job's status words on the device; cond_status_stride bytes to the next
  long long cond_status_stride = 0;
  char* cond_pinned = nullptr;        // staging block of an asynchronous batch (the context's is the solver's)
  size_t cond_pinned_cap = 0;
  hipEvent_t ev_cond_done = nullptr, ev_pack = nullptr, ev_packed = nullptr;
  bool pack_in_flight = false;        // the uploads of the last cgmr_graph_pack may not have left the pinned block yet
  std::vector<hipEvent_t> ev_consumed;          // per destination robot: its copy of my send buffer is done (cgmr_graph_deliver)
  std::vector<uint8_t> consumed_pending;
};

namespace cgmr {

inline size_t round256(size_t v) { return (v + 255) & ~size_t(255); }
inline int graph_device(cgmr_graph* g) {                         // makes the graph's device current
  HIP_TRY(g->ctx, hipSetDevice(g->ctx->device));
  return 0;
}
// asynchronous batches are in use on this context from now on (the cached structure's chained solve was sized for the whole device)
inline void use_side_stream(cgmr_ctx* ctx) {
  if (ctx && !ctx->side_used) { ctx->side_used = true; ctx->sym_valid = false; }
}
// robot_graph.cpp
int gerr(cgmr_graph* g, int code, const char* msg);
int dev_grow(cgmr_graph* g, DevBuf& B, size_t used_bytes, size_t need_bytes);
void rebuild_all_edges(cgmr_graph* g);
void insert_sorted_unique(std::vector<int32_t>& v, const int32_t* ids, int n);
GnEdges graph_edges(const cgmr_graph* g, int n_active);         // the level-0 edges on the device, the first n_active switched on
// condensed_host.cpp
// the pending batch, if any, is waited for on the graph's device; tolerate_failed_batch: its failure (on record) is not this call's
int finish_pending(cgmr_graph* g, bool tolerate_failed_batch);
// exchange_host.cpp
int wait_consumers(cgmr_graph* g, hipStream_t st);
bool ingest_decide_sender(cgmr_graph* g, int s, int n_e, const int32_t* from_to, int n_c, const int32_t* closures);

}  // namespace cgmr
