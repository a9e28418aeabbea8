// cgmr_remove_nodes (include/cgmr.h): the host side of vertex removal.  Compiled with hipcc; contains no kernels.
//
// Everything that can be refused is refused here, before anything is queued.  One pass over the edge list collects each removed
// vertex' incident edges (a CSR of edge indices, in index order); its neighbours are their other ends, sorted and unique, and
// the node of every incident edge is its other end's place among them.  The device (remove_nodes_kernels.hip) does the
// arithmetic, one workgroup per vertex, into slots sized by the degrees; the vertices that were removed are packed here.
#include "host_call.h"
#include "remove_nodes_device.h"

#include <algorithm>

namespace cgmr {

int remove_nodes_driver(cgmr_ctx* ctx, int nV, int nE, const int32_t* ef, const int32_t* et, const double* meas, const double* info,
                        int nR, const int32_t* remove, int cap_out, int32_t* off_out, int32_t* from_out, int32_t* to_out,
                        double* meas_out, double* info_out, double* weight_out, int32_t* flags_out) {
  const char* who = "cgmr_remove_nodes";
  if (nV <= 0 || nE < 0 || nR < 0 || cap_out < 0 || (nE > 0 && (!ef || !et || !meas || !info)) ||
      (nR > 0 && (!remove || !off_out || !flags_out)) || (cap_out > 0 && (!from_out || !to_out || !meas_out || !info_out)))
    return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", who);
  for (int e = 0; e < nE; e++)
    if (ef[e] < 0 || ef[e] >= nV || et[e] < 0 || et[e] >= nV) return set_err(ctx, CGMR_E_INVALID, "%s: edge %d: vertex index out of range", who, e);
  std::vector<int32_t> slot(nV, -1);                               // a removed vertex' place in `remove`
  for (int r = 0; r < nR; r++) {
    if (remove[r] < 0 || remove[r] >= nV) return set_err(ctx, CGMR_E_INVALID, "%s: remove_idx[%d] out of range", who, r);
    if (slot[remove[r]] >= 0) return set_err(ctx, CGMR_E_INVALID, "%s: vertex %d is listed twice", who, remove[r]);
    slot[remove[r]] = r;
  }
  if (nR == 0) return 0;
  // the incident edges of every removed vertex, in index order
  std::vector<int32_t> inc_off(nR + 1, 0);
  for (int e = 0; e < nE; e++) {
    const int ra = slot[ef[e]], rb = slot[et[e]];
    if (ra < 0 && rb < 0) continue;
    if (ef[e] == et[e]) return set_err(ctx, CGMR_E_INVALID, "%s: edge %d joins removed vertex %d to itself", who, e, ef[e]);
    if (ra >= 0 && rb >= 0)
      return set_err(ctx, CGMR_E_INVALID, "%s: edge %d joins the removed vertices %d and %d (one call removes an independent set)", who, e, ef[e], et[e]);
    inc_off[(ra >= 0 ? ra : rb) + 1]++;
  }
  for (int r = 0; r < nR; r++) inc_off[r + 1] += inc_off[r];
  const int nI = inc_off[nR];
  std::vector<int32_t> inc_edge(nI), inc_node(nI), fill(inc_off.begin(), inc_off.end() - 1);
  for (int e = 0; e < nE; e++) {
    const int ra = slot[ef[e]], rb = slot[et[e]];
    if (ra >= 0 || rb >= 0) inc_edge[fill[ra >= 0 ? ra : rb]++] = e;
  }
  // the neighbours n_1 < .. < n_m of every removed vertex, the node of every incident edge, the output slots
  std::vector<int32_t> nbr_off(nR + 1, 0), nbr, deg(nR), out_off(nR + 1, 0);
  std::vector<int32_t> other;
  for (int r = 0; r < nR; r++) {
    other.clear();
    for (int q = inc_off[r]; q < inc_off[r + 1]; q++) other.push_back(ef[inc_edge[q]] == remove[r] ? et[inc_edge[q]] : ef[inc_edge[q]]);
    std::vector<int32_t> uniq(other);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    const int m = (int)uniq.size();
    for (int q = inc_off[r]; q < inc_off[r + 1]; q++)
      inc_node[q] = (int32_t)(std::lower_bound(uniq.begin(), uniq.end(), other[q - inc_off[r]]) - uniq.begin());
    deg[r] = m > CGMR_REMOVE_MAX_DEGREE ? -1 : m;
    nbr.insert(nbr.end(), uniq.begin(), uniq.end());
    nbr_off[r + 1] = (int32_t)nbr.size();
    out_off[r + 1] = out_off[r] + (deg[r] > 1 ? deg[r] - 1 : 0);
  }
  const int need = out_off[nR];
  if (cap_out < need) return set_err(ctx, CGMR_E_INVALID, "%s: cap_out %d, the new edges may number %d", who, cap_out, need);

  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Layout256 L;
  const size_t nEs = (size_t)nE, nRs = (size_t)nR, nIs = (size_t)nI, nO = (size_t)need;
  const size_t o_ef = L.add(4 * nEs), o_et = L.add(4 * nEs), o_m = L.add(24 * nEs), o_i = L.add(48 * nEs), o_rm = L.add(4 * nRs),
               o_io = L.add(4 * (nRs + 1)), o_ie = L.add(4 * nIs), o_in = L.add(4 * nIs), o_dg = L.add(4 * nRs), o_oo = L.add(4 * nRs),
               o_par = L.add(4 * nO), o_est = L.add(24 * nO), o_inf = L.add(48 * nO), o_w = L.add(8 * nO), o_fl = L.add(4 * nRs);
  int rc = arena_reserve(ctx, ctx->io_arena, L.off + 256);
  if (rc) return rc;
  char* d = ctx->io_arena.ptr;
  hipStream_t st = ctx->stream;
  auto up = [&](size_t o, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(d + o, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
  HIP_TRY(ctx, up(o_ef, ef, 4 * nEs));
  HIP_TRY(ctx, up(o_et, et, 4 * nEs));
  HIP_TRY(ctx, up(o_m, meas, 24 * nEs));
  HIP_TRY(ctx, up(o_i, info, 48 * nEs));
  HIP_TRY(ctx, up(o_rm, remove, 4 * nRs));
  HIP_TRY(ctx, up(o_io, inc_off.data(), 4 * (nRs + 1)));
  HIP_TRY(ctx, up(o_ie, inc_edge.data(), 4 * nIs));
  HIP_TRY(ctx, up(o_in, inc_node.data(), 4 * nIs));
  HIP_TRY(ctx, up(o_dg, deg.data(), 4 * nRs));
  HIP_TRY(ctx, up(o_oo, out_off.data(), 4 * nRs));
  RemoveNodes P;
  P.nR = nR;
  P.ef = (const int32_t*)(d + o_ef); P.et = (const int32_t*)(d + o_et);
  P.meas = (const double*)(d + o_m); P.info = (const double*)(d + o_i);
  P.remove = (const int32_t*)(d + o_rm); P.inc_off = (const int32_t*)(d + o_io); P.inc_edge = (const int32_t*)(d + o_ie);
  P.inc_node = (const int32_t*)(d + o_in); P.deg = (const int32_t*)(d + o_dg); P.out_off = (const int32_t*)(d + o_oo);
  P.parent = (int32_t*)(d + o_par); P.est = (double*)(d + o_est); P.info_out = (double*)(d + o_inf); P.weight = (double*)(d + o_w);
  P.flags = (int32_t*)(d + o_fl);
  KTimer KT{ctx, st};
  KT.run(11, 1, [&] { launch_remove_nodes(st, P); });
  std::vector<int32_t> parent(nO), flags(nRs);
  std::vector<double> est(3 * nO), inf(6 * nO), w(nO);
  auto down = [&](void* dst, size_t o, size_t bytes) { return bytes ? hipMemcpyAsync(dst, d + o, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
  HIP_TRY(ctx, down(parent.data(), o_par, 4 * nO));
  HIP_TRY(ctx, down(est.data(), o_est, 24 * nO));
  HIP_TRY(ctx, down(inf.data(), o_inf, 48 * nO));
  HIP_TRY(ctx, down(w.data(), o_w, 8 * nO));
  HIP_TRY(ctx, down(flags.data(), o_fl, 4 * nRs));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipGetLastError());
  if (ctx->profiling) profile_collect(ctx);
  // the removed vertices' edges, packed in the order of `remove`
  int n = 0;
  off_out[0] = 0;
  for (int r = 0; r < nR; r++) {
    flags_out[r] = flags[r];
    if (flags[r] == 0)
      for (int q = out_off[r]; q < out_off[r + 1]; q++, n++) {
        const int32_t* nb = nbr.data() + nbr_off[r];
        from_out[n] = nb[parent[q]];
        to_out[n] = nb[q - out_off[r] + 1];
        for (int k = 0; k < 3; k++) meas_out[3 * (size_t)n + k] = est[3 * (size_t)q + k];
        for (int k = 0; k < 6; k++) info_out[6 * (size_t)n + k] = inf[6 * (size_t)q + k];
        if (weight_out) weight_out[n] = w[q];
      }
    off_out[r + 1] = n;
  }
  return n;
}

}  // namespace cgmr
