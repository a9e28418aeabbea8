// Device side of vertex removal (remove_nodes_kernels.hip; include/cgmr.h: cgmr_remove_nodes).
//
// A removed vertex v is marginalised out of the star of its incident edges and the star is replaced by a spanning tree of
// relative-pose edges over its neighbours n_1 < .. < n_m (the nodes 0 .. m - 1 here):
//   the local configuration: v at the identity, n at z_vn of the lowest-index edge between v and n (inverted where the edge is
//   stored n -> v) -- the exact optimum of the star when no neighbour has a second edge;
//   H = sum J^T Omega J over every incident edge at that configuration, each with its own measurement's rotation.  A parallel
//   edge adds its term there; its residual against the first edge is dropped;
//   n_1 fixed, v eliminated first by the Cholesky factor, the trailing 3 (m - 1) block inverted: the covariance of n_2 .. n_m
//   with v marginalised out (zero blocks for n_1);
//   w(a, b) = log det Sigma_z(a, b) (relative_cov_device.h, tree_order_device.h), the minimum spanning tree under the total
//   order (w, max, min) rooted at n_1, and a first-order label for each tree edge parent -> child: est = x_p^-1 x_c,
//   information = (R(est.theta)^T Sigma_z R(est.theta))^-1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cgmr {

// One call: nR removed vertices over the edge list (ef, et, meas [3 nE], info [6 nE]).
//   inc_off [nR + 1], inc_edge, inc_node: per removed vertex its incident edges in index order and the node (0 .. m - 1) of
//   each one's other end;  deg [nR]: m, or -1 with more than CGMR_REMOVE_MAX_DEGREE neighbours;  out_off [nR]: where the
//   vertex' m - 1 edges go in the outputs, edge k - 1 the one of node k.
//   parent: the node of the edge's from-end;  est [3], info [6] (upper triangle), weight: the edge's label and its w;
//   flags [nR]: 0 removed, 1 no Cholesky factor of H, 2 too many neighbours, 3 a tree edge without a finite weight (Sigma_z has
//   no factor) -- with a flag other than 0 the vertex' output slots are not written.
struct RemoveNodes {
  int nR = 0;
  const int32_t *ef = nullptr, *et = nullptr;
  const double *meas = nullptr, *info = nullptr;
  const int32_t *remove = nullptr, *inc_off = nullptr, *inc_edge = nullptr, *inc_node = nullptr, *deg = nullptr, *out_off = nullptr;
  int32_t* parent = nullptr;
  double *est = nullptr, *info_out = nullptr, *weight = nullptr;
  int32_t* flags = nullptr;
};

// One 64-lane workgroup per removed vertex, no atomics: two calls give identical bytes.
void launch_remove_nodes(hipStream_t st, const RemoveNodes& P);

}  // namespace cgmr
