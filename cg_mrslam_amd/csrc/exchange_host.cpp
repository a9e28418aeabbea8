// The robot graph's exchange (include/cgmr.h, "exchange"): the round message packed on the device or on the host, the
// in-process transport, the ingests of a round's receive buffer, the one-peer messages, what is held from a peer.  The bytes
// themselves -- offsets, the ids read-back, when a message is not sent, the host's writer and reader -- are wire_format.h's.
// Reference behaviour being replaced:
//   MRGraphSLAM::addInterRobotData, constructCondensedGraphMessage      src/mrslam/mr_graph_slam.cpp:331-395, 607-670
//   CondensedGraphBuffer::insertEdgesFromRobot                           condensed_graph_buffer.cpp:487-510
//   GraphComm::send (a message beyond MAX_LENGTH_MSG is skipped)         src/mrslam/graph_comm.cpp:112-122
#include "robot_graph.h"

using namespace cgmr;

namespace cgmr {

// whatever is about to overwrite my send buffer waits for the robots that are still copying it (cgmr_graph_deliver)
// (a flag per stream that may write the buffer: bit 0 = the context's stream, bit 1 = its side stream; an event wait queued on one
// of them orders nothing on the other)
int wait_consumers(cgmr_graph* g, hipStream_t st) {
  const uint8_t bit = st == g->ctx->stream ? 1 : 2;
  for (size_t d = 0; d < g->consumed_pending.size(); d++)
    if (g->consumed_pending[d] & bit) { HIP_TRY(g->ctx, hipStreamWaitEvent(st, g->ev_consumed[d], 0)); g->consumed_pending[d] &= (uint8_t)~bit; }
  return 0;
}

// What every ingest path decides per sender s (mr_graph_slam.cpp:331-395), from the (from, to) id pairs of its n_e edges and
// its n_c closure requests: the requests become out-closures, the edges whose end points exist take staging slots
// s * cap + k and replace the set held from s.  Returns false when no edge survives (the previous set is kept).
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

}  // namespace cgmr

namespace {

// The tail the all-robot ingests share: ids = the read-back of k_wire_read or of its host mirror (wire_format.h: IdsLayout).
// n_edges_out (nullable) [n_robots]: accepted edges per sender this round (0 = nothing replaced).
void ingest_decide(cgmr_graph* g, const int32_t* ids, std::vector<uint8_t>& accepted, int32_t* n_edges_out) {
  const IdsLayout L{g->cap};
  accepted.assign(g->n_robots, 0);
  for (int s = 0; s < g->n_robots; s++) {
    if (s != g->robot) {
      const int32_t* rec = L.record(ids, s);
      accepted[s] = ingest_decide_sender(g, s, rec[0], L.pairs(rec), rec[1], L.closures(rec)) ? 1 : 0;
    }
    if (n_edges_out) n_edges_out[s] = accepted[s] ? (int32_t)g->in[s].slot.size() : 0;
  }
  rebuild_all_edges(g);
}

// header + closure requests of this robot's wire buffer (host side)
void fill_header(const cgmr_graph* g, unsigned char* buf) {
  int32_t n_edges[64];                                           // (cgmr_graph_create: n_robots <= 64)
  for (int p = 0; p < g->n_robots; p++) n_edges[p] = g->out[p].n;
  write_header(buf, g->robot, g->n_robots, g->cap, n_edges, g->in_closures.data());
}
// counts the messages fill_header() is about to leave out
void count_skipped(cgmr_graph* g) {
  for (int p = 0; p < g->n_robots; p++)
    if (p != g->robot && slice_not_sent(g->out[p].n, (int)g->in_closures[p].size(), g->cap)) g->skipped_messages++;
}

// the flattened slot list of all peers (the order of the compact second edge segment) into the pinned block; returns its length
int stage_slots(cgmr_graph* g) {
  int32_t* h_slot = (int32_t*)(g->pinned + g->pin.slot);
  int j = 0;
  for (int s = 0; s < g->n_robots; s++) for (int32_t sl : g->in[s].slot) h_slot[j++] = sl;
  return j;
}

}  // namespace

extern "C" {

int64_t cgmr_graph_wire_bytes(const cgmr_graph* g) { return g ? (int64_t)wire_bytes(g->n_robots, g->cap) : -1; }

// Serialise this robot's round message (ComboMessage of condensed edges + closure requests, mr_graph_slam.cpp:527-562,
// 607-670) into a device buffer of cgmr_graph_wire_bytes() bytes.  The edges are already in the graph's send buffer as
// wire records (cgmr_graph_compute_condensed writes them there); the header and the request lists -- host bookkeeping --
// are staged through pinned memory.  d_send_out may be NULL: the graph's own send buffer is then the message.
int cgmr_graph_pack(cgmr_graph* g, void* d_send_out) {
  if (!g) return CGMR_E_INVALID;
  if (!g->ctx) return gerr(g, CGMR_E_NO_DEVICE, "cgmr_graph_pack: no device context (use cgmr_graph_pack_host)");
  cgmr_ctx* ctx = g->ctx;
  if (int rc = graph_device(g)) return rc;
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
  unsigned char* h_wire = (unsigned char*)g->pinned + g->pin.wire;
  memset(h_wire, 0, wb);
  fill_header(g, h_wire);
  HIP_TRY(ctx, hipMemcpyAsync(g->d_send, h_wire, wire_edges_off(R), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(g->d_send + wire_clos_off(R, cap), h_wire + wire_clos_off(R, cap), (size_t)R * cap * 4,
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
  if (int rc = graph_device(dst)) return rc;
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
    int rc = finish_pending(g, /*tolerate_failed_batch=*/true);  // (a failed batch: its peers get no edges, the message still goes out)
    if (rc) return rc;
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
  if (int rc = graph_device(g)) return rc;
  hipStream_t st = ctx->stream;
  const int R = g->n_robots, cap = g->cap;
  const IdsLayout L{cap};
  const unsigned char* recv = d_recv ? (const unsigned char*)d_recv : g->d_recv;
  g->msg_in_flight = false;            // (the synchronisation below covers a message's uploads: same stream)
  launch_wire_read(st, R, cap, g->robot, wire_bytes(R, cap), recv, g->d_tmp_meas, g->d_tmp_info, g->d_ids_out);
  int32_t* h_ids = (int32_t*)(g->pinned + g->pin.ids);
  HIP_TRY(ctx, hipMemcpyAsync(h_ids, g->d_ids_out, L.bytes(R), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int s = 0; s < R && skip_senders; s++)
    if (s < 64 && ((skip_senders >> s) & 1)) {                    // no edges, no closure requests from this sender this round
      int32_t* rec = L.record(h_ids, s);
      rec[0] = 0; rec[1] = 0;
    }
  std::vector<uint8_t> accepted;
  ingest_decide(g, h_ids, accepted, n_edges_out);
  unsigned long long fresh = 0;                                   // senders whose message replaced their previous set (R <= 64)
  for (int s = 0; s < R; s++) {
    if (!accepted[s]) continue;
    g->hs_fresh[s] = 0;
    fresh |= 1ULL << s;
  }
  const int j = stage_slots(g);
  if (j > 0) {
    // one launch: the accepted senders' records move from the widened wire data into the staging and, with the sets kept
    // from earlier rounds, into the compact second edge segment (two device copies per accepted sender + a gather before)
    HIP_TRY(ctx, hipMemcpyAsync(g->d_slot, g->pinned + g->pin.slot, 4 * (size_t)j, hipMemcpyHostToDevice, st));
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
  if (int rc = graph_device(g)) return rc;
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
    if (int rc = graph_device(g)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(g->d_recv, recv, (size_t)R * wb, hipMemcpyHostToDevice, ctx->stream));
    return cgmr_graph_ingest(g, nullptr, n_edges_out);
  }
  // host-only mirror of k_wire_read (wire_format.h: read_slice) + the staging copies
  const IdsLayout L{cap};
  std::vector<int32_t> ids(L.bytes(R) / 4, 0);
  std::vector<double> tm(3 * (size_t)R * cap), ti(6 * (size_t)R * cap);
  for (int s = 0; s < R; s++)
    read_slice((const unsigned char*)recv + (size_t)s * wb, s, g->robot, R, cap, L.record(ids.data(), s), tm.data() + 3 * (size_t)s * cap,
               ti.data() + 6 * (size_t)s * cap);
  std::vector<uint8_t> accepted;
  ingest_decide(g, ids.data(), accepted, n_edges_out);
  for (int s = 0; s < R; s++) {
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
  if (int rc = finish_pending(g, false)) return rc;
  // one peer's part of the round message: the counts and the closure requests are host bookkeeping (what fill_header()
  // writes), the edges are this peer's slice of the send buffer -- on the device when there is one: only that slice comes
  // back (round 2 packed and downloaded the whole buffer, 400 KB for four robots, for every peer and tick)
  const std::vector<int32_t>& cl = g->in_closures[peer];
  // A message beyond the slice capacity or the reference's byte limit (wire_format.h: message_not_sent) is not sent -- no
  // message, one count -- as GraphComm::send skips a message whose toCharArray returned 0 (graph_comm.cpp:112-122).
  if (message_not_sent(g->out[peer].n, (int)cl.size(), cap)) {
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
      if (int rc = graph_device(g)) return rc;
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
  const int cap = g->cap;
  if (slice_not_sent(n_edges, n_closures, cap)) {    // beyond what a reference node's receive buffer holds: dropped, not an error
    g->skipped_messages++;
    if (n_accepted_out) *n_accepted_out = 0;
    return CGMR_OK;
  }
  bool any_known = false;
  for (int k = 0; k < n_closures; k++) any_known = any_known || g->index.count(closure_ids[k]);
  // One message: the host holds everything the decision needs (the end point ids are in the wire records), and widening
  // 9 floats per edge is no work for it.  So nothing is read back: the accepted set's numbers go to the host mirror of the
  // staging at the sender's slots and, with a device, to the staging itself; the slot list of the compact second segment
  // follows, the gather is queued behind them -- no synchronisation.  (Round 2 built and uploaded the whole receive buffer,
  // 1.7 MB for four robots, for every message; until the end of round 3 the message went through k_wire_read with a
  // 109 KB read-back of ids per message: 156 us per call in the C4 leg.)
  if (g->ctx) { if (int rc = graph_device(g)) return rc; }
  std::vector<int32_t> ft(2 * (size_t)n_edges);
  const unsigned char* eb = (const unsigned char*)edges44;
  for (int k = 0; k < n_edges; k++) memcpy(&ft[2 * (size_t)k], eb + (size_t)k * sizeof(WireEdge), 8);   // from, to lead the record
  static_assert(offsetof(WireEdge, from) == 0 && offsetof(WireEdge, to) == 4, "wire record layout");
  const bool ok = ingest_decide_sender(g, sender, n_edges, ft.data(), n_closures, closure_ids);
  rebuild_all_edges(g);
  if (ok) {
    double* hm = g->hs_meas.data() + 3 * (size_t)sender * cap;
    double* hi = g->hs_info.data() + 6 * (size_t)sender * cap;
    for (int k = 0; k < n_edges; k++) {
      WireEdge w;
      memcpy(&w, eb + (size_t)k * sizeof(WireEdge), sizeof w);
      widen(w, hm + 3 * (size_t)k, hi + 6 * (size_t)k);
    }
    g->hs_fresh[sender] = 1;
  }
  if (ok && g->ctx) {                 // the uploads: pinned copies of the numbers and of the slot list, the gather behind them
    cgmr_ctx* ctx = g->ctx;
    hipStream_t st = ctx->stream;
    if (g->msg_in_flight) { HIP_TRY(ctx, hipEventSynchronize(g->ev_msg)); g->msg_in_flight = false; }
    double* pm = (double*)(g->pinned + g->pin.msg);
    double* pi = pm + 3 * (size_t)cap;
    memcpy(pm, g->hs_meas.data() + 3 * (size_t)sender * cap, 24 * (size_t)n_edges);
    memcpy(pi, g->hs_info.data() + 6 * (size_t)sender * cap, 48 * (size_t)n_edges);
    HIP_TRY(ctx, hipMemcpyAsync(g->d_stage_meas + 3 * (size_t)sender * cap, pm, 24 * (size_t)n_edges, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(g->d_stage_info + 6 * (size_t)sender * cap, pi, 48 * (size_t)n_edges, hipMemcpyHostToDevice, st));
    const int j = stage_slots(g);
    HIP_TRY(ctx, hipMemcpyAsync(g->d_slot, g->pinned + g->pin.slot, 4 * (size_t)j, hipMemcpyHostToDevice, st));
    launch_gather_edges(st, j, g->d_slot, g->d_stage_meas, g->d_stage_info, g->d_meas_b, g->d_info_b);
    HIP_TRY(ctx, hipEventRecord(g->ev_msg, st));
    g->msg_in_flight = true;
  }
  if (n_accepted_out) *n_accepted_out = ok ? (int32_t)g->in[sender].slot.size() : 0;
  if (any_known && g->ctx) {
    const int rc = cgmr_graph_compute_condensed(g, sender);
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
      if (int rc = graph_device(g)) return rc;
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

}  // extern "C"
