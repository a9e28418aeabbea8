// The inter-robot wire format: the 44-byte record, the geometry of a rank's round buffer and of the ids read-back, the rule for
// a message that is not sent, and the host's writer and reader of a buffer.  Plain C++17, nothing of HIP: the kernels
// (mrslam_kernels.hip), the robot graph's host layer (exchange_host.cpp) and the sanitised harness (tests/host/wire_sweep.cpp)
// all include this file, and the geometry is written down nowhere else.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace cgmr {

// EdgeArrayMessage::ESE2Data as it travels (src/mrslam/msg_factory.h:200-205, doubles narrowed to float32 by
// msg_factory.h:78-112): 44 bytes
struct WireEdge {
  int32_t from, to;      // vertex ids (robot * baseId + k)
  float est[3];          // condensed measurement (x, y, theta)
  float info[6];         // upper triangle of the information matrix
};
static_assert(sizeof(WireEdge) == 44, "wire edge must be 44 bytes");

// One CondensedGraphMessage as the reference serialises it (msg_factory.cpp:256-262): int32 type and robot, a size_t counter
// and 44 bytes per edge, a size_t counter and 4 bytes per closure id; one datagram holds MAX_LENGTH_MSG bytes (msg_factory.h:115)
constexpr size_t kMaxLengthMsg = 100000;
inline size_t condensed_message_bytes(int n_edges, int n_closures) {
  return 8 + 8 + sizeof(WireEdge) * (size_t)n_edges + 8 + 4 * (size_t)n_closures;
}

// One rank's buffer: int32 header {robot, n_robots, n_edges[R], n_closures[R]}, WireEdge edges[R][cap] (slice p = the
// edges for peer p), int32 closures[R][cap] (slice p = the ids this robot requests from p).
inline size_t wire_bytes(int n_robots, int cap) {
  return 4 * (size_t)(2 + 2 * n_robots) + (size_t)n_robots * cap * sizeof(WireEdge) + (size_t)n_robots * cap * 4;
}
inline size_t wire_edges_off(int n_robots) { return 4 * (size_t)(2 + 2 * n_robots); }
inline size_t wire_clos_off(int n_robots, int cap) { return wire_edges_off(n_robots) + (size_t)n_robots * cap * sizeof(WireEdge); }

// A slice that does not fit the wire buffer is not sent at all -- the reference's toCharArray() returns 0 for a message beyond
// MAX_LENGTH_MSG and GraphComm::send skips it (graph_comm.cpp:112-122, msg_factory.h:115) -- instead of failing the round
// (every rank still contributes its fixed-size buffer to the all-gather): its two counts travel as zeros.
inline bool slice_not_sent(int n_edges, int n_closures, int cap) { return n_edges > cap || n_closures > cap; }
// The one-peer form.  That message travels as the reference's byte string, so the reference's limit holds for it besides the
// slice capacity: header, two counters, 44 bytes per edge and 4 per closure id must fit MAX_LENGTH_MSG as a whole (at
// cap = 2270 the edges alone nearly fill it: 2270 edges leave room for 24 ids).
inline bool message_not_sent(int n_edges, int n_closures, int cap) {
  return slice_not_sent(n_edges, n_closures, cap) || condensed_message_bytes(n_edges, n_closures) > kMaxLengthMsg;
}

// The ids read-back of k_wire_read (mrslam_kernels.hip; its comment is the statement of record): one record of int32 per
// sender -- n_edges, n_closures, the (from, to) id pairs of cap edges, cap closure ids.
struct IdsLayout {
  int cap = 0;
  size_t stride() const { return 2 + 3 * (size_t)cap; }                       // int32 per sender
  size_t bytes(int n_robots) const { return 4 * (size_t)n_robots * stride(); }
  template <class T> T* record(T* ids, int sender) const { return ids + (size_t)sender * stride(); }
  // inside a record: [0] = n_edges, [1] = n_closures, then
  template <class T> T* pairs(T* rec) const { return rec + 2; }
  template <class T> T* closures(T* rec) const { return rec + 2 + 2 * (size_t)cap; }
};

// float32 -> double of a record's numbers (exact)
inline void widen(const WireEdge& e, double meas[3], double info[6]) {
  for (int a = 0; a < 3; a++) meas[a] = (double)e.est[a];
  for (int a = 0; a < 6; a++) info[a] = (double)e.info[a];
}

// Header and closure requests of `robot`'s buffer `buf` (wire_bytes(n_robots, cap) bytes; what is not written keeps the
// caller's bytes): n_edges[p] = the edges in slice p, closures[p] = the ids requested from p.  A slice over capacity is not
// sent (slice_not_sent).
inline void write_header(unsigned char* buf, int robot, int n_robots, int cap, const int32_t* n_edges,
                         const std::vector<int32_t>* closures) {
  int32_t* hdr = reinterpret_cast<int32_t*>(buf);
  hdr[0] = robot; hdr[1] = n_robots;
  int32_t* clos = reinterpret_cast<int32_t*>(buf + wire_clos_off(n_robots, cap));
  for (int p = 0; p < n_robots; p++) {
    const int n = (int)closures[p].size();
    if (slice_not_sent(n_edges[p], n, cap)) { hdr[2 + p] = 0; hdr[2 + n_robots + p] = 0; continue; }
    hdr[2 + p] = n_edges[p];
    hdr[2 + n_robots + p] = n;
    for (int k = 0; k < n; k++) clos[(size_t)p * cap + k] = closures[p][k];
  }
}

// The host mirror of k_wire_read for ONE sender: `buf` is the buffer at position `sender` of a round's receive buffer, `me`
// the receiver.  Writes the sender's ids record `rec` (IdsLayout) and the widened numbers of its edges for me (meas: 3 per
// edge, info: 6 per edge, cap edges at most).  The counts are clamped to [0, cap]; a buffer whose sender id is not its
// position (or is my own) counts as empty.
inline void read_slice(const unsigned char* buf, int sender, int me, int n_robots, int cap, int32_t* rec, double* meas, double* info) {
  const IdsLayout L{cap};
  const int32_t* hdr = reinterpret_cast<const int32_t*>(buf);
  const bool ok = hdr[0] == sender && sender != me;
  const int n_e = hdr[2 + me] < 0 ? 0 : (hdr[2 + me] > cap ? cap : hdr[2 + me]);
  const int n_c = hdr[2 + n_robots + me] < 0 ? 0 : (hdr[2 + n_robots + me] > cap ? cap : hdr[2 + n_robots + me]);
  rec[0] = ok ? n_e : 0; rec[1] = ok ? n_c : 0;
  const WireEdge* e = reinterpret_cast<const WireEdge*>(buf + wire_edges_off(n_robots)) + (size_t)me * cap;
  const int32_t* c = reinterpret_cast<const int32_t*>(buf + wire_clos_off(n_robots, cap)) + (size_t)me * cap;
  int32_t* ft = L.pairs(rec);
  for (int k = 0; k < n_e; k++) {
    ft[2 * k] = e[k].from; ft[2 * k + 1] = e[k].to;
    widen(e[k], meas + 3 * (size_t)k, info + 6 * (size_t)k);
  }
  for (int k = 0; k < n_c; k++) L.closures(rec)[k] = c[k];
}

}  // namespace cgmr
