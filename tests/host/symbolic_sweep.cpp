// Stand-alone host harness of the symbolic analysis (cg_mrslam_amd/csrc/gn_symbolic.cpp), meant to be built with the host
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/host/Makefile) and run as its own process on a machine without a GPU.
// It calls analyze() on the boundary families of tests/boundary_cases.py, on chains around the 2048-vertex threshold of the
// root's multi-start sweep, on graphs that grow 50 vertices at a time across that threshold (the key-frame pattern, with the
// previous analysis handed over as cgmr_gn_symbolic_info_grown does) and with named hub vertices, and checks every result:
// the permutation is a bijection, the fronts partition the columns, every front's parent, level, children and border rows
// are consistent; and structure_reference() -- the serial builder of the arrays the device makes for itself, which the GPU tests
// hold the kernels to -- runs on every analysis: its lists are complete and every row map entry lies inside the parent.  The
// helper pool reads CGMR_HOST_THREADS once per process: run it once with 1 and once with 4 (make check).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "gn_symbolic.h"
#include "switches.h"

using cgmr::FrontDesc;
using cgmr::Symbolic;

namespace {

struct Graph {
  int nV = 0;
  std::vector<int32_t> ef, et;
  std::vector<int32_t> edges_at;      // grown graphs: edges_at[v] = edges whose end points are all < v (a prefix of the list)
  void edge(int a, int b) { ef.push_back(a); et.push_back(b); }
};

int n_fail = 0, n_cases = 0;

#define EXPECT(cond, ...) \
  do { if (!(cond)) { if (n_fail < 50) { fprintf(stderr, "FAIL %s: %s: ", name.c_str(), #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } n_fail++; return; } } while (0)

void check(const std::string& name, const Symbolic& S, int nV, int nE, const int32_t* ef, const int32_t* et) {
  n_cases++;
  std::vector<uint8_t> active(nV, 0);
  for (int k = 0; k < nE; k++) active[ef[k]] = active[et[k]] = 1;
  int nf = 0;
  for (int v = 0; v < nV; v++) nf += active[v];
  EXPECT(S.nf == nf && (int)S.vperm.size() == nV, "nf %d, expected %d", S.nf, nf);
  if (nf == 0) return;
  EXPECT((int)S.perm.size() == nf, "perm has %zu entries", S.perm.size());
  std::vector<uint8_t> seen(nf, 0);
  for (int v = 0; v < nV; v++) {
    const int c = S.vperm[v];
    if (!active[v]) { EXPECT(c == -1, "vertex %d has no edge and column %d", v, c); continue; }
    EXPECT(c >= 0 && c < nf, "vertex %d: column %d of %d", v, c, nf);
    EXPECT(!seen[c], "column %d taken twice (vertex %d)", c, v);
    seen[c] = 1;
    EXPECT(S.perm[c] == v, "perm[%d] = %d, vperm[%d] = %d", c, S.perm[c], v, c);
  }
  const int nfr = (int)S.fronts.size();
  EXPECT(nfr > 0 && (int)S.col_front.size() == nf, "%d fronts, col_front %zu", nfr, S.col_front.size());
  int next_col = 0, n_children = 0, n_with_parent = 0, max_level = 0;
  for (int f = 0; f < nfr; f++) {
    const FrontDesc& F = S.fronts[f];
    EXPECT(F.c0 == next_col && F.nc >= 1 && F.nc <= cgmr::kPanelW, "front %d: columns %d + %d, expected to start at %d", f, F.c0, F.nc, next_col);
    next_col += F.nc;
    for (int c = F.c0; c < F.c0 + F.nc; c++) EXPECT(S.col_front[c] == f, "col_front[%d] = %d, front %d", c, S.col_front[c], f);
    EXPECT(F.ns >= 0 && F.rows_off >= 0 && (size_t)F.rows_off + F.ns <= S.rows.size(), "front %d: border %d at %d of %zu", f, F.ns, F.rows_off, S.rows.size());
    int last = F.c0 + F.nc - 1;
    for (int k = 0; k < F.ns; k++) {
      const int r = S.rows[F.rows_off + k];
      EXPECT(r > last && r < nf, "front %d: border row %d = %d after %d (nf %d)", f, k, r, last, nf);
      last = r;
    }
    EXPECT((F.parent < 0) == (F.ns == 0), "front %d: parent %d, border %d", f, F.parent, F.ns);
    if (F.parent >= 0) {
      EXPECT(F.parent > f && F.parent < nfr, "front %d: parent %d of %d fronts", f, F.parent, nfr);
      const FrontDesc& P = S.fronts[F.parent];
      EXPECT(S.col_front[S.rows[F.rows_off]] == F.parent, "front %d: first border row %d belongs to front %d, parent %d", f, S.rows[F.rows_off], S.col_front[S.rows[F.rows_off]], F.parent);
      EXPECT(P.level > F.level, "front %d on level %d, parent %d on level %d", f, F.level, F.parent, P.level);
      // every border row is a column or a border row of the parent
      int q = 0;
      for (int k = 0; k < F.ns; k++) {
        const int r = S.rows[F.rows_off + k];
        if (r < P.c0 + P.nc) { EXPECT(r >= P.c0, "front %d: border row %d before its parent's columns", f, r); continue; }
        while (q < P.ns && S.rows[P.rows_off + q] < r) q++;
        EXPECT(q < P.ns && S.rows[P.rows_off + q] == r, "front %d: border row %d is not in parent %d", f, r, F.parent);
      }
      n_with_parent++;
    }
    EXPECT(F.level >= 0 && (F.nchild > 0 || F.level == 0), "front %d: level %d with %d children", f, F.level, F.nchild);
    EXPECT(F.nchild >= 0 && F.child_off >= 0 && (size_t)F.child_off + F.nchild <= S.children.size(), "front %d: children %d at %d", f, F.nchild, F.child_off);
    for (int k = 0; k < F.nchild; k++) {
      const int c = S.children[F.child_off + k];
      EXPECT(c >= 0 && c < f && S.fronts[c].parent == f, "front %d: child %d", f, c);
    }
    n_children += F.nchild;
    max_level = std::max(max_level, F.level);
  }
  EXPECT(next_col == nf && n_children == n_with_parent, "columns %d of %d, children %d, fronts with a parent %d", next_col, nf, n_children, n_with_parent);
  EXPECT((int)S.level_ptr.size() == max_level + 2 && S.level_ptr.back() == nfr && (int)S.level_fronts.size() == nfr, "level lists: %zu levels for a highest level %d", S.level_ptr.size() - 1, max_level);
  for (int l = 0; l <= max_level; l++)
    for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) EXPECT(S.fronts[S.level_fronts[q]].level == l, "level list %d holds front %d of level %d", l, S.level_fronts[q], S.fronts[S.level_fronts[q]].level);
  // every edge lies inside a front: the later end point is a column or a border row of the front that owns the earlier one
  for (int k = 0; k < nE; k++) {
    int a = S.vperm[ef[k]], b = S.vperm[et[k]];
    if (a == b) continue;
    if (a > b) std::swap(a, b);
    const FrontDesc& F = S.fronts[S.col_front[a]];
    if (b < F.c0 + F.nc) continue;
    const int32_t* r = S.rows.data() + F.rows_off;
    EXPECT(std::binary_search(r, r + F.ns, b), "edge %d: column %d is not in the border of front %d", k, b, S.col_front[a]);
  }
  cgmr::StructureRef R;
  EXPECT(cgmr::structure_reference(S, nE, ef, et, R) == 0, "structure_reference failed");
  EXPECT((int)R.asm_ptr.size() == nf + S.nb + 1 && R.asm_ptr[nf + S.nb] == (int)R.asm_src.size(), "assembly lists: %zu keys, %zu entries", R.asm_ptr.size(), R.asm_src.size());
  EXPECT((int64_t)R.rel.size() == S.n_rel && (int64_t)R.inv.size() == S.n_inv, "row maps: %zu and %zu entries", R.rel.size(), R.inv.size());
  for (int f = 0; f < nfr; f++) {
    const FrontDesc& F = S.fronts[f];
    if (F.parent < 0) continue;
    const FrontDesc& P = S.fronts[F.parent];
    for (int k = 0; k < F.ns; k++) {
      const int p = R.rel[F.rel_off + k];
      EXPECT(p >= 0 && p < P.nc + P.ns, "front %d: border row %d at position %d of parent %d (%d + %d)", f, k, p, F.parent, P.nc, P.ns);
    }
  }
}

void run(const std::string& name, const Graph& g, const std::vector<int32_t>& hubs = {}) {
  Symbolic S;
  const int rc = cgmr::analyze(g.nV, nullptr, (int)g.ef.size(), g.ef.data(), g.et.data(), S, cgmr::read_switches(), nullptr, -1, hubs.empty() ? nullptr : hubs.data(), (int)hubs.size());
  if (rc) { fprintf(stderr, "FAIL %s: analyze returned %d\n", name.c_str(), rc); n_fail++; return; }
  check(name, S, g.nV, (int)g.ef.size(), g.ef.data(), g.et.data());
}

// the key-frame pattern: the first nV0 vertices, then `step` more at a time, every analysis handed the one before
void run_grown(const std::string& name, const Graph& g, int nV0, int step) {
  Symbolic S;
  int nV = nV0, n_ext = 0;
  if (cgmr::analyze(nV, nullptr, g.edges_at[nV], g.ef.data(), g.et.data(), S, cgmr::read_switches())) { fprintf(stderr, "FAIL %s: first analysis\n", name.c_str()); n_fail++; return; }
  check(name + " @" + std::to_string(nV), S, nV, g.edges_at[nV], g.ef.data(), g.et.data());
  while (nV < g.nV) {
    nV = std::min(g.nV, nV + step);
    Symbolic old = std::move(S);
    if (cgmr::analyze(nV, nullptr, g.edges_at[nV], g.ef.data(), g.et.data(), S, cgmr::read_switches(), &old)) { fprintf(stderr, "FAIL %s: analysis at %d\n", name.c_str(), nV); n_fail++; return; }
    n_ext += S.extended ? 1 : 0;
    check(name + " @" + std::to_string(nV), S, nV, g.edges_at[nV], g.ef.data(), g.et.data());
  }
  printf("  %s: %d of the steps extended the ordering\n", name.c_str(), n_ext);
}

// ---- the families of tests/boundary_cases.py (edge lists only: the analysis reads nothing else)
void add_clique(Graph& g, int lo, int n) {
  for (int i = 0; i < n; i++) for (int j = i + 1; j < n; j++) g.edge(lo + i, lo + j);
}
Graph clique(int n) { Graph g; g.nV = n; add_clique(g, 0, n); return g; }
Graph forest(int k, int n) { Graph g; g.nV = k * n; for (int c = 0; c < k; c++) add_clique(g, c * n, n); return g; }
Graph blobs(int b, int c, int m, int copies = 1) {
  Graph g;
  const int V1 = b + m * c;
  g.nV = copies * V1;
  for (int q = 0; q < copies; q++) {
    const int lo = q * V1;
    add_clique(g, lo, b);
    for (int j = 0; j < m; j++) {
      const int o = lo + b + j * c;
      add_clique(g, o, c);
      for (int s = 0; s < b; s++) for (int i = 0; i < c; i++) g.edge(lo + s, o + i);
    }
  }
  return g;
}
Graph star(int k) { Graph g; g.nV = k + 1; for (int i = 1; i <= k; i++) g.edge(0, i); return g; }
Graph dup(int d) { Graph g; g.nV = 2; for (int i = 0; i < d; i++) g.edge(0, 1); return g; }
Graph chain(int V, bool closed = false) {
  Graph g;
  g.nV = V;
  g.edges_at.assign(V + 1, 0);
  for (int v = 1; v < V; v++) { g.edge(v - 1, v); g.edges_at[v + 1] = (int)g.ef.size(); }
  if (closed) g.edge(0, V - 1);
  return g;
}
// odometry plus loop closures to earlier vertices, near ones mostly, in vertex order (the shape of synth.make_pose_graph)
Graph pose_graph(int V, int closures_per_100, uint64_t seed) {
  Graph g;
  g.nV = V;
  g.edges_at.assign(V + 1, 0);
  uint64_t s = seed * 6364136223846793005ull + 1442695040888963407ull;
  auto rnd = [&s](uint32_t n) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((s >> 33) % n); };
  for (int v = 1; v < V; v++) {
    g.edge(v - 1, v);
    while (v > 2 && (int)rnd(100) < closures_per_100) {
      const int back = rnd(4) == 0 ? 2 + (int)rnd(v - 2) : 2 + (int)rnd(std::min(v - 2, 60));
      g.edge(v - back, v);
    }
    g.edges_at[v + 1] = (int)g.ef.size();
  }
  return g;
}

}  // namespace

int main() {
  printf("symbolic_sweep: CGMR_HOST_THREADS=%d\n", cgmr::process_switches().host_threads);
  for (int n = 2; n <= 71; n++) run("clique_" + std::to_string(n), clique(n));
  for (int b = 1; b <= 54; b++) run("blobs_" + std::to_string(b), blobs(b, 16, 4));
  for (int k : {2, 9}) for (int n = 17; n <= 64; n++) run("forest" + std::to_string(k) + "_" + std::to_string(n), forest(k, n));
  for (int m : {2, 3, 4, 5, 6, 7, 8, 9, 10, 31, 32, 33, 34, 63, 64, 65, 66}) run("fan_" + std::to_string(m), blobs(6, 20, m));
  for (int m : {4, 5, 8, 9, 16, 17, 32, 33, 64, 65}) run("fan2_" + std::to_string(m), blobs(6, 20, m, 2));
  for (int m : {7, 8, 9, 10}) run("fanlow_" + std::to_string(m), blobs(44, 16, m));
  for (int k = 1; k <= 1026; k++) if (k <= 20 || (k >= 63 && k <= 66) || (k >= 255 && k <= 258) || k >= 1023) run("star_" + std::to_string(k), star(k));
  for (int d : {3, 4, 5, 8, 9, 16, 17}) run("dup_" + std::to_string(d), dup(d));
  for (int V : {2047, 2048, 2049, 2050, 4096, 32767, 32768, 32769, 32770}) {
    run("chain_" + std::to_string(V), chain(V));
    run("ring_" + std::to_string(V), chain(V, true));
  }
  // repeated in one process: the overflow of the root's sweep corrupted the heap for a later analysis
  for (int rep = 0; rep < 3; rep++) for (int V : {2048, 32770, 4096}) run("chain_" + std::to_string(V) + " again", chain(V));
  printf("  %d analyses of the families checked\n", n_cases);
  // grown: 50 vertices at a time across the 2048-vertex threshold
  run_grown("grown chain", chain(2400), 1900, 50);
  run_grown("grown chain from 2000", chain(2100), 2000, 50);
  for (uint64_t seed = 1; seed <= 3; seed++) run_grown("grown pose graph " + std::to_string(seed), pose_graph(2400, 30, seed), 1900, 50);
  run_grown("grown pose graph from 50", pose_graph(2300, 20, 9), 50, 50);
  // named hub vertices
  run("star_1026 hub centre", star(1026), {0});
  run("star_20 hub leaf", star(20), {7});
  run("fan_9 hub separator", blobs(6, 20, 9), {0, 1, 2, 3, 4, 5});
  run("fan2_9 hubs", blobs(6, 20, 9, 2), {0, 186});
  run("chain_2048 hub ends", chain(2048), {0, 2047});
  run("chain_2049 hub middle", chain(2049), {1024});
  run("ring_32769 hub", chain(32769, true), {0});
  {
    Graph g = pose_graph(3000, 30, 5);
    for (int v = 100; v < 3000; v += 37) { g.edge(17, v); g.edge(v, 2500); }       // two gauges of received stars
    run("pose graph 3000, hubs named", g, {17, 2500});
    run("pose graph 3000, hubs found", g);
    run("pose graph 3000, hub without an edge in the list", pose_graph(3000, 30, 6), {5, 2999});
  }
  printf("symbolic_sweep: %d analyses checked, %d failed\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
