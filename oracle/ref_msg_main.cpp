// Driver around the reference's own message serialiser (src/mrslam/msg_factory.{h,cpp}), which needs nothing but the
// standard library.  The reference is reached only through the include below and by linking its msg_factory.cpp
// unmodified (oracle/Makefile, target _ref/ref_msg); nothing of it is restated here.
//
//   ref_msg encode < records > replies      every record -> int64 length (-1: toCharArray returned null), the bytes
//   ref_msg decode < messages > records     every {int64 length, bytes} -> one record
//
// A record (host byte order, no padding) carries every field any of the five message types has; a type uses its own:
//   int32 type, robot
//   int64 nv;  int32 vertex_id[nv];  double vertex_estimate[nv][3]
//   int32 nodeId;  int64 nr;  double readings[nr];  double minangle, angleincrement, maxrange, accuracy
//   int64 ne;  int32 from_to[ne][2];  double estimate_information[ne][9]
//   int64 nc;  int32 closures[nc]
// Types: 1 VertexArrayMessage, 4 ComboMessage, 5 EdgeArrayMessage, 6 ClosuresMessage, 7 CondensedGraphMessage.
// toCharArray is called with bsize = MAX_LENGTH_MSG on a buffer four times that size: the combined messages check each part
// against the whole bsize and write up to twice MAX_LENGTH_MSG.
#include "msg_factory.h"

#include <cstdint>
#include <cstdio>

namespace {

struct Record {
  int32_t type = 0, robot = -1;
  std::vector<int32_t> vid;
  std::vector<double> vest;
  int32_t node_id = 0;
  std::vector<double> readings;
  double laser[4] = {0, 0, 0, 0};
  std::vector<int32_t> from_to;
  std::vector<double> edge_numbers;
  std::vector<int32_t> closures;
};

bool get(void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, stdin) == bytes; }
void put(const void* p, size_t bytes) {
  if (bytes && fwrite(p, 1, bytes, stdout) != bytes) exit(3);
}

// false at a clean end of input; a record cut short ends the program
bool read_record(Record& r) {
  if (fread(&r.type, 1, 4, stdin) != 4) return false;
  int64_t nv = 0, nr = 0, ne = 0, nc = 0;
  bool ok = get(&r.robot, 4) && get(&nv, 8) && nv >= 0;
  if (ok) { r.vid.resize(nv); r.vest.resize(3 * nv); ok = get(r.vid.data(), 4 * nv) && get(r.vest.data(), 24 * nv); }
  ok = ok && get(&r.node_id, 4) && get(&nr, 8) && nr >= 0;
  if (ok) { r.readings.resize(nr); ok = get(r.readings.data(), 8 * nr) && get(r.laser, 32); }
  ok = ok && get(&ne, 8) && ne >= 0;
  if (ok) { r.from_to.resize(2 * ne); r.edge_numbers.resize(9 * ne); ok = get(r.from_to.data(), 8 * ne) && get(r.edge_numbers.data(), 72 * ne); }
  ok = ok && get(&nc, 8) && nc >= 0;
  if (ok) { r.closures.resize(nc); ok = get(r.closures.data(), 4 * nc); }
  if (!ok) { fprintf(stderr, "ref_msg: truncated record\n"); exit(2); }
  return true;
}

void write_record(const Record& r) {
  const int64_t nv = r.vid.size(), nr = r.readings.size(), ne = r.from_to.size() / 2, nc = r.closures.size();
  put(&r.type, 4); put(&r.robot, 4);
  put(&nv, 8); put(r.vid.data(), 4 * nv); put(r.vest.data(), 24 * nv);
  put(&r.node_id, 4); put(&nr, 8); put(r.readings.data(), 8 * nr); put(r.laser, 32);
  put(&ne, 8); put(r.from_to.data(), 8 * ne); put(r.edge_numbers.data(), 72 * ne);
  put(&nc, 8); put(r.closures.data(), 4 * nc);
}

void fill(VertexArrayMessage& m, const Record& r) {
  m.vertexVector.resize(r.vid.size());
  for (size_t k = 0; k < r.vid.size(); k++) {
    m.vertexVector[k].id = r.vid[k];
    for (int a = 0; a < 3; a++) m.vertexVector[k].estimate[a] = r.vest[3 * k + a];
  }
}
void fill(RobotLaserMessage& m, const Record& r) {
  m.nodeId = r.node_id;
  m.readings = r.readings;
  m.minangle = r.laser[0]; m.angleincrement = r.laser[1]; m.maxrange = r.laser[2]; m.accuracy = r.laser[3];
}
void fill(EdgeArrayMessage& m, const Record& r) {
  m.edgeVector.resize(r.from_to.size() / 2);
  for (size_t k = 0; k < m.edgeVector.size(); k++) {
    m.edgeVector[k].idfrom = r.from_to[2 * k];
    m.edgeVector[k].idto = r.from_to[2 * k + 1];
    for (int a = 0; a < 3; a++) m.edgeVector[k].estimate[a] = r.edge_numbers[9 * k + a];
    for (int a = 0; a < 6; a++) m.edgeVector[k].information[a] = r.edge_numbers[9 * k + 3 + a];
  }
}
void fill(ClosuresMessage& m, const Record& r) { m.closures = r.closures; }

void take(Record& r, const VertexArrayMessage& m) {
  for (size_t k = 0; k < m.vertexVector.size(); k++) {
    r.vid.push_back(m.vertexVector[k].id);
    for (int a = 0; a < 3; a++) r.vest.push_back(m.vertexVector[k].estimate[a]);
  }
}
void take(Record& r, const RobotLaserMessage& m) {
  r.node_id = m.nodeId;
  r.readings = m.readings;
  r.laser[0] = m.minangle; r.laser[1] = m.angleincrement; r.laser[2] = m.maxrange; r.laser[3] = m.accuracy;
}
void take(Record& r, const EdgeArrayMessage& m) {
  for (size_t k = 0; k < m.edgeVector.size(); k++) {
    r.from_to.push_back(m.edgeVector[k].idfrom);
    r.from_to.push_back(m.edgeVector[k].idto);
    for (int a = 0; a < 3; a++) r.edge_numbers.push_back(m.edgeVector[k].estimate[a]);
    for (int a = 0; a < 6; a++) r.edge_numbers.push_back(m.edgeVector[k].information[a]);
  }
}
void take(Record& r, const ClosuresMessage& m) { r.closures = m.closures; }

void reply(const RobotMessage& m, std::vector<char>& buf) {
  const char* end = m.toCharArray(buf.data(), MAX_LENGTH_MSG);
  const int64_t len = end ? (int64_t)(end - buf.data()) : -1;
  put(&len, 8);
  if (len > 0) put(buf.data(), (size_t)len);
}

int encode() {
  std::vector<char> buf(4 * (size_t)MAX_LENGTH_MSG);
  for (;;) {
    Record r;
    if (!read_record(r)) return 0;
    // (the virtual base is built by its default constructor in the combined messages: the id is set afterwards)
    if (r.type == VertexArrayMessage::_type()) { VertexArrayMessage m; m.setRobotId(r.robot); fill(m, r); reply(m, buf); }
    else if (r.type == ComboMessage::_type()) {
      ComboMessage m; m.setRobotId(r.robot); fill((VertexArrayMessage&)m, r); fill((RobotLaserMessage&)m, r); reply(m, buf);
    }
    else if (r.type == EdgeArrayMessage::_type()) { EdgeArrayMessage m; m.setRobotId(r.robot); fill(m, r); reply(m, buf); }
    else if (r.type == ClosuresMessage::_type()) { ClosuresMessage m; m.setRobotId(r.robot); fill(m, r); reply(m, buf); }
    else if (r.type == CondensedGraphMessage::_type()) {
      CondensedGraphMessage m; m.setRobotId(r.robot); fill((EdgeArrayMessage&)m, r); fill((ClosuresMessage&)m, r); reply(m, buf);
    }
    else { fprintf(stderr, "ref_msg: unknown message type %d\n", r.type); return 2; }
  }
}

int decode() {
  MessageFactory factory;
  factory.registerMessageType<VertexArrayMessage>();
  factory.registerMessageType<ComboMessage>();
  factory.registerMessageType<EdgeArrayMessage>();
  factory.registerMessageType<ClosuresMessage>();
  factory.registerMessageType<CondensedGraphMessage>();
  for (;;) {
    int64_t len = 0;
    if (fread(&len, 1, 8, stdin) != 8) return 0;
    if (len <= 4) { fprintf(stderr, "ref_msg: message too short\n"); return 2; }
    std::vector<char> buf((size_t)len);
    if (!get(buf.data(), (size_t)len)) { fprintf(stderr, "ref_msg: truncated message\n"); return 2; }
    RobotMessage* m = factory.fromCharArray(buf.data(), (size_t)len);
    Record r;
    r.type = m->type(); r.robot = m->robotId();
    if (const VertexArrayMessage* v = dynamic_cast<const VertexArrayMessage*>(m)) take(r, *v);
    if (const RobotLaserMessage* l = dynamic_cast<const RobotLaserMessage*>(m)) take(r, *l);
    if (const EdgeArrayMessage* e = dynamic_cast<const EdgeArrayMessage*>(m)) take(r, *e);
    if (const ClosuresMessage* c = dynamic_cast<const ClosuresMessage*>(m)) take(r, *c);
    write_record(r);
    delete m;
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  int rc = 2;
  if (mode == "encode") rc = encode();
  else if (mode == "decode") rc = decode();
  else fprintf(stderr, "usage: ref_msg encode|decode  (binary records on stdin / stdout, see the head of ref_msg_main.cpp)\n");
  fflush(stdout);
  return rc;
}
