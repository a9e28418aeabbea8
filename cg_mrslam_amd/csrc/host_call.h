// What a solver entry point was given, and what cgmr_api.cpp and marginals_host.cpp share to check and stage it.
#pragma once
#include "gn_host.h"

namespace cgmr {

// The problem arguments of an entry point as the caller passed them -- host pointers, or with `dev` device pointers for poses,
// meas and info -- and the optional descriptions that go with them.  The marginals family never writes through `poses`.
struct HostCall {
  int nV;
  double* poses;
  const uint8_t* fixed;
  int nE;
  const int32_t *ef, *et;
  const double *meas, *info;
  bool dev;
  const cgmr_robust* rk;
  const cgmr_factor_types* ft;
  const cgmr_mixture* mix;
};
struct HostCallHow { bool dev = false; const cgmr_robust* rk = nullptr; const cgmr_factor_types* ft = nullptr; const cgmr_mixture* mix = nullptr; };
inline HostCall host_call(int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et,
                          const double* meas, const double* info, const HostCallHow& how = HostCallHow()) {
  return {nV, const_cast<double*>(poses), fixed, nE, ef, et, meas, info, how.dev, how.rk, how.ft, how.mix};
}

// The factor types of a typed entry point (include/cgmr.h: cgmr_factor_types), checked on the host before the device is
// touched: every vertex kind 0 or 1, every edge kind with the vertex kinds and the arity its factor needs.  `any`: some kind
// is not zero (all zero: the call is the plain one, bit for bit -- the plain launches).  The priors grouped by vertex, in edge
// order, for k_add_unary.
struct TypedHost {
  bool any = false;
  std::vector<uint8_t> vk, ek;
  std::vector<int32_t> uv_vertex, uv_ptr, uv_edge;
};
int typed_check(cgmr_ctx* ctx, const char* who, const HostCall& c, TypedHost& T);
// ... staged through ty_arena into Ed (nothing when every kind is zero)
int typed_upload(cgmr_ctx* ctx, const TypedHost* T, GnEdges& Ed);
// The robust description of an entry point (include/cgmr.h: cgmr_robust) into Ed, checked before anything is queued; the
// statistics of the call's final pass to the caller's host arrays (cgmr_api.cpp)
int robust_setup(cgmr_ctx* ctx, const cgmr_robust* rk, int nE, bool dev, GnEdges& Ed, const char* who);
int robust_stats_out(cgmr_ctx* ctx, const cgmr_robust* rk, int nE, const GnEdges& Ed);

// The marginals family (marginals_host.cpp).  marginal_driver: mode 0 marginals at c.poses with c.fixed; 1 covariance estimate
// (gauge); 2 condense (gauge).  joint_driver: mode 0 joint, 1 pairs, 2 relative / observation covariance.
int marginal_driver(cgmr_ctx* ctx, int mode, const HostCall& c, int gauge, int nK, const int32_t* query, int32_t* to_out,
                    double* est_out, double* info_out, double* cov_out);
int marginals_all_driver(cgmr_ctx* ctx, const HostCall& c, double* cov_out, double* cross_out);
int joint_driver(cgmr_ctx* ctx, const char* who, int mode, const HostCall& c, int nQ, const int32_t* va, const int32_t* vb,
                 double* out_a, double* out_b, double* out_c, const double* hyp_meas, const double* hyp_info, bool obs = false,
                 const uint8_t* obs_kind = nullptr);
// pcm_driver / clique_driver with `ex`: the exact solver behind the greedy clique (cgmr_closure_consistency_exact,
// cgmr_max_clique_exact); proven_out takes seed_out's place among the outputs, seed_out is not read.  Without: the greedy pair.
struct CliqueExact { int64_t node_limit; int32_t* proven_out; int64_t* nodes_out; };
// pcm_driver with `inter`: the two-graph form (cgmr_closure_consistency_inter[_exact]) -- candidate k ends at a peer's vertex
// known by peer_pose[3 k ..], cb is not read; peer_cov [3 nC * 3 nC] or null (pcm_device.h: PcmInterClosures).
struct PcmInter { const double* peer_pose; const double* peer_cov; };
int pcm_driver(cgmr_ctx* ctx, const HostCall& c, int nC, const int32_t* ca, const int32_t* cb, const double* cmeas,
               const double* cinfo, double gamma, double* d2_out, uint64_t* adj_out, int32_t* clique_out, int32_t* size_out,
               int32_t* seed_out, const CliqueExact* ex = nullptr, const PcmInter* inter = nullptr);
int clique_driver(cgmr_ctx* ctx, int n, const uint64_t* adj, int32_t* clique_out, int32_t* size_out, int32_t* seed_out,
                  const CliqueExact* ex = nullptr);
// The condensed graph as a spanning tree of relative poses (include/cgmr.h: cgmr_condense_tree; c.fixed is not read: the gauge
// alone is fixed), and the spanning tree alone on a caller's weights (cgmr_min_spanning_tree)
int condense_tree_driver(cgmr_ctx* ctx, const HostCall& c, int gauge, int nK, const int32_t* query, int32_t* from_out,
                         int32_t* to_out, double* est_out, double* info_out, double* weight_out, int32_t* flags_out);
int mst_driver(cgmr_ctx* ctx, int n, const double* weights, int root, int32_t* parent_out);
// Vertex removal (remove_nodes_host.cpp; include/cgmr.h: cgmr_remove_nodes): every check, the CSR of incident edges, one launch on
// the context's stream (in profiling mode in class 11, with the other spanning-tree launches), the packed result
int remove_nodes_driver(cgmr_ctx* ctx, int nV, int nE, const int32_t* ef, const int32_t* et, const double* meas, const double* info,
                        int nR, const int32_t* remove, int cap_out, int32_t* off_out, int32_t* from_out, int32_t* to_out,
                        double* meas_out, double* info_out, double* weight_out, int32_t* flags_out);
// Joint-compatibility data association (jcbb_host.cpp; include/cgmr.h: cgmr_jcbb_dense, cgmr_joint_compatibility).  The
// outputs of both: ic [nM * nL] and nodes nullable, the others required; assign holds positions among the candidates
// (jc_dense_driver) or their vertex indices (jc_driver).
struct JcOut { double* ic; int32_t *assign, *count; double* d2; int32_t *dof, *proven; int64_t* nodes; };
int jc_dense_driver(cgmr_ctx* ctx, int nM, int nL, int nA, const int32_t* slot, const int32_t* dim, const double* sigma,
                    const double* e, const double* J, const double* R, const double* gamma, int64_t node_limit, const JcOut& out);
// the pass and the solve half of joint_driver's mode 0 over the observing poses and the candidates, every lower Gram tile
int jc_driver(cgmr_ctx* ctx, const HostCall& c, int nM, const int32_t* obs_pose, const uint8_t* obs_kind, const double* obs_meas,
              const double* obs_info, int nL, const int32_t* lm, const double* gamma, int64_t node_limit, const JcOut& out);

}  // namespace cgmr
