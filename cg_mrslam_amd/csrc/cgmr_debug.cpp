// The cgmr_debug_* entry points of libcgmr.so: test hooks and debugging aids; behind them the robot graph's (cgmr_graph_debug_*)
// and the wire kernels' (cgmr_wire_narrow_edges*).
#include "gn_host.h"
#include "robot_graph.h"

#include <algorithm>
#include <cstring>

using namespace cgmr;

// the front table of an analysis, 6 ints per front: c0, nc, ns, parent, level, nchild; returns the number of fronts
static int front_table_out(const Symbolic& S, int cap, int32_t* out) {
  const int n = (int)S.fronts.size();
  for (int f = 0; f < n && f < cap && out; f++) {
    const FrontDesc& F = S.fronts[f];
    int32_t* o = out + 6 * f;
    o[0] = F.c0; o[1] = F.nc; o[2] = F.ns; o[3] = F.parent; o[4] = F.level; o[5] = F.nchild;
  }
  return n;
}

// Debugging aid (host only): the front table of a graph's symbolic analysis
extern "C" int cgmr_debug_fronts(int nV, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et, int cap, int32_t* out) {
  Symbolic S;
  (void)fixed;
  if (analyze(nV, nullptr, nE, ef, et, S, read_switches())) return -1;
  return front_table_out(S, cap, out);
}

// The children's schedule of every front (tests): out[4 f ..] = sched_t, sched_slot, pan_slots, 1 if the front adds into its
// parent's panel (0: root, or child of the top block)
extern "C" int cgmr_debug_schedule(int nV, int nE, const int32_t* ef, const int32_t* et, int cap, int32_t* out) {
  Symbolic S;
  if (analyze(nV, nullptr, nE, ef, et, S, read_switches())) return -1;
  int n = (int)S.fronts.size();
  for (int f = 0; f < n && f < cap; f++) {
    const FrontDesc& F = S.fronts[f];
    int32_t* o = out + 4 * f;
    o[0] = F.sched_t; o[1] = F.sched_slot; o[2] = F.pan_slots; o[3] = F.ppan_off >= 0 ? 1 : 0;
  }
  return n;
}

// Debugging aid: the (front, chunk) of every work item of the last analysed graph, and each front's parent / level.
extern "C" int cgmr_debug_worklist(const cgmr_ctx* ctx, int32_t* front_out, int32_t* chunk_out, int cap, int32_t* parent_out,
                                   int32_t* level_out, int32_t* ns_out, int fcap) {
  if (!ctx) return -1;
  const Symbolic& S = ctx->sym;
  int n = 0;
  for (int l = 0; l + 1 < (int)S.level_ptr.size(); l++)
    for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) {
      int f = S.level_fronts[q];
      int r = 3 * S.fronts[f].ns;
      const int chunk_rows = l < (int)ctx->gn.h_level_chunk.size() ? ctx->gn.h_level_chunk[l] : kChunkRows;
      int nchunk = std::max(1, (r + chunk_rows - 1) / chunk_rows);
      for (int c = 0; c < nchunk; c++) { if (n < cap) { front_out[n] = f; chunk_out[n] = c; } n++; }
    }
  for (int f = 0; f < (int)S.fronts.size() && f < fcap; f++) { parent_out[f] = S.fronts[f].parent; level_out[f] = S.fronts[f].level; ns_out[f] = S.fronts[f].ns; }
  return n;
}

// Host-only test hook: a sequence of complete edge lists analysed one after the other the way a context with the analysis
// cache on does (step k: vertices nV[k], edges e_ptr[k] .. e_ptr[k+1] of ef / et, hub hints h_ptr[k] .. h_ptr[k+1] of hubs).
// out / perm_out / fronts_out (6 ints per front as cgmr_debug_fronts) describe the last analysis; returns its front count.
extern "C" int cgmr_debug_symbolic_steps(int n_steps, const int32_t* nV, const int32_t* e_ptr, const int32_t* ef, const int32_t* et,
                                         const int32_t* h_ptr, const int32_t* hubs, int64_t out[16], int32_t* perm_out,
                                         int32_t* n_extended_out, int fcap, int32_t* fronts_out, int64_t* per_step_out) {
  if (n_steps < 1 || !nV || !e_ptr || !out) return -1;
  Symbolic S;
  const Switches sw = read_switches();
  std::vector<int32_t> pef, pet;
  int prev_nV = 0, next = 0;
  for (int k = 0; k < n_steps; k++) {
    const int nE = e_ptr[k + 1] - e_ptr[k];
    const int nh = h_ptr ? h_ptr[k + 1] - h_ptr[k] : 0;
    if (analyze_next(S, sw, k > 0, prev_nV, pef, pet, {nV[k], nullptr, nullptr, nE, ef + e_ptr[k], et + e_ptr[k], nh ? hubs + h_ptr[k] : nullptr, nh})) return -1;
    if (k > 0 && S.extended) next++;
    if (per_step_out) {                                     // per step: levels, extended, ordering us, structure us, factor flops
      int64_t* o = per_step_out + 5 * (size_t)k;
      o[0] = (int64_t)S.level_ptr.size() - 1; o[1] = S.extended ? 1 : 0; o[2] = (int64_t)(1e6 * S.t_order); o[3] = (int64_t)(1e6 * S.t_struct); o[4] = (int64_t)S.flops;
    }
    pef.assign(ef + e_ptr[k], ef + e_ptr[k + 1]);
    pet.assign(et + e_ptr[k], et + e_ptr[k + 1]);
    prev_nV = nV[k];
  }
  if (n_extended_out) *n_extended_out = next;
  symbolic_info_out(S, nV[n_steps - 1], out, perm_out);
  return front_table_out(S, fcap, fronts_out);
}

// Tests: the assembly lists (gn_symbolic.h: asm_ptr / asm_src) as the host's reference builds them for an edge list (ctx ==
// nullptr: structure_reference), or as they stand on the device for the graph the context analysed last (ef / et ignored).  Returns nf + nb (the number of
// keys; -1: error), the number of list entries in *n_src_out.
extern "C" int cgmr_debug_asm_lists(cgmr_ctx* ctx, int nV, int nE, const int32_t* ef, const int32_t* et, int cap_ptr, int32_t* ptr_out,
                                    int cap_src, int32_t* src_out, int32_t* n_src_out) {
  if (!ptr_out || !src_out || !n_src_out) return -1;
  if (!ctx) {
    Symbolic S;
    StructureRef R;
    if (analyze(nV, nullptr, nE, ef, et, S, read_switches()) || structure_reference(S, nE, ef, et, R)) return -1;
    const int nk = S.nf + S.nb;
    if (nk + 1 > cap_ptr || (int)R.asm_src.size() > cap_src) return -1;
    if (R.asm_ptr.empty()) { *n_src_out = 0; return nk; }
    memcpy(ptr_out, R.asm_ptr.data(), 4 * (size_t)(nk + 1));
    memcpy(src_out, R.asm_src.data(), 4 * R.asm_src.size());
    *n_src_out = (int)R.asm_src.size();
    return nk;
  }
  const GnDevice& D = ctx->gn;
  const int nk = D.nf + D.nb;
  if (nk + 1 > cap_ptr || !D.asm_ptr) return -1;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
  if (hipMemcpy(ptr_out, D.asm_ptr, 4 * (size_t)(nk + 1), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const int ns = ptr_out[nk];
  if (ns > cap_src) return -1;
  if (ns > 0 && hipMemcpy(src_out, D.asm_src, 4 * (size_t)ns, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  *n_src_out = ns;
  return nk;
}

// Tests: rel | inv | blk_dst | b_dst (gn_symbolic.h) one behind the other, as the host's reference builds them for an edge list
// (ctx == nullptr: structure_reference) or as they stand on the device for the graph the context analysed last.  Returns the number of ints, -1: error.
extern "C" int cgmr_debug_maps(cgmr_ctx* ctx, int nV, int nE, const int32_t* ef, const int32_t* et, int cap, int32_t* out) {
  if (!out) return -1;
  if (!ctx) {
    Symbolic S;
    StructureRef R;
    if (analyze(nV, nullptr, nE, ef, et, S, read_switches()) || structure_reference(S, nE, ef, et, R)) return -1;
    const size_t n = R.rel.size() + R.inv.size() + R.blk_dst.size() + R.b_dst.size();
    if (n > (size_t)cap) return -1;
    int32_t* o = out;
    for (const std::vector<int32_t>* v : {&R.rel, &R.inv, &R.blk_dst, &R.b_dst}) { memcpy(o, v->data(), 4 * v->size()); o += v->size(); }
    return (int)n;
  }
  const GnDevice& D = ctx->gn;
  const Symbolic& S = ctx->sym;
  const size_t sizes[4] = {(size_t)S.n_rel, (size_t)S.n_inv, (size_t)S.nf + S.nb, (size_t)S.nf};
  const int32_t* srcs[4] = {D.rel, D.inv, D.blk_dst, D.b_dst};
  if (sizes[0] + sizes[1] + sizes[2] + sizes[3] > (size_t)cap) return -1;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
  int32_t* o = out;
  for (int k = 0; k < 4; k++) {
    if (sizes[k] && hipMemcpy(o, srcs[k], 4 * sizes[k], hipMemcpyDeviceToHost) != hipSuccess) return -1;
    o += sizes[k];
  }
  return (int)(o - out);
}

// Tests: the factor kernel's work records (gn_symbolic.h: WorkRec) of the graph the context analysed last, as they stand on the
// device (dev_out) and as a host loop over the context's analysis and chunk lengths writes them (ref_out); cap records each.
// Returns the number of records (more than cap: nothing was written), -1: error.
extern "C" int cgmr_debug_work_records(cgmr_ctx* ctx, int cap, void* dev_out, void* ref_out) {
  if (!ctx) return -1;
  const GnDevice& D = ctx->gn;
  const Symbolic& S = ctx->sym;
  const int n_work = D.h_work_ptr.empty() ? 0 : D.h_work_ptr.back();
  if (n_work > cap || n_work == 0) return n_work;
  if (!dev_out || !ref_out) return -1;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
  if (n_work && hipMemcpy(dev_out, D.work, sizeof(WorkRec) * (size_t)n_work, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  WorkRec* work = static_cast<WorkRec*>(ref_out);
  for (int l = 0; l < D.nlevels; l++) {
    const int chunk_rows = D.h_level_chunk[l];
    int w = D.h_work_ptr[l];
    for (int q = S.gn_level_ptr[l]; q < S.gn_level_ptr[l + 1]; q++) {
      const int f = S.gn_level_fronts[q];
      const int r = 3 * S.fronts[f].ns;
      const int nchunk = std::max(1, (r + chunk_rows - 1) / chunk_rows);
      for (int c = 0; c < nchunk; c++) {
        WorkRec& wr = work[w++];
        memset(&wr, 0, sizeof wr);
        wr.F = S.fronts[f];
        wr.front = f;
        wr.chunk = c;
        for (int k = 0; k < std::min<int>(wr.F.nchild, kWorkChildren); k++) {
          const FrontDesc& G = S.fronts[S.children[wr.F.child_off + k]];
          WorkChild& wc = wr.ch[k];
          wc.U_off = G.U_off; wc.ns = G.ns; wc.na = G.na;
          wc.rel_off = G.rel_off; wc.inv_off = G.inv_off; wc.rows_off = G.rows_off;
        }
      }
    }
    if (w != D.h_work_ptr[l + 1]) return -1;
  }
  return n_work;
}

// ---- the robot graph and the wire (robot_graph.h, mrslam_device.h)

extern "C" {

// Debugging aid: the level-0 edge list (vertex indices) the solver sees: own edges first, then the received ones.
int cgmr_graph_debug_edges(const cgmr_graph* g, int cap, int32_t* from_out, int32_t* to_out, int32_t* n_own_out) {
  if (!g || cap < 0) return CGMR_E_INVALID;
  const int n = (int)g->all_ef.size();
  for (int k = 0; k < n && k < cap; k++) { from_out[k] = g->all_ef[k]; to_out[k] = g->all_et[k]; }
  if (n_own_out) *n_own_out = (int32_t)g->ef.size();
  return n;
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

}  // extern "C"
