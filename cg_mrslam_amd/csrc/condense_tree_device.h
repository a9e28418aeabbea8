// Device side of the condensed graph as a spanning tree of relative poses (condense_tree_kernels.hip; include/cgmr.h:
// cgmr_condense_tree, cgmr_min_spanning_tree).
//
// The nodes are the gauge (node 0) and the unique requested vertices (nodes 1 .. n - 1).  Every unordered pair is a candidate
// edge of weight w(a, b) = log det Sigma_z(a, b), Sigma_z the first-order covariance of z = x_a^-1 x_b under the joint
// covariance of the two vertices (relative_cov_device.h); the condensed graph is the minimum spanning tree under the total
// order (w, max(a, b), min(a, b)), rooted at the gauge, each edge parent -> child labelled as g2o's EdgeLabeler labels it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cgmr {

// The nodes of a tree call on the device: vert[k] the vertex of node k (vert[0] the gauge), slot[k] its 4-column group of Y
// among the queries, or -1 (the gauge, a fixed or inactive vertex: zero rows of Sigma).
struct TreeNodes {
  int n = 0;
  const int32_t *vert = nullptr, *slot = nullptr;
};

// W [n * n], symmetric, +inf on the diagonal: W[a][b] = log det Sigma_z(min(a, b), max(a, b)) from the dense tile set G
// (joint_marginals_kernels.hip) at `poses`, the determinant from a 3x3 Cholesky factor; +inf where a pivot is not positive and
// finite, and for every pair of a node other than the gauge whose slot is -1.  One thread per unordered pair.
void launch_tree_weights(hipStream_t st, const TreeNodes& N, const double* poses, const double* G, double* W);
// The minimum spanning tree of the dense symmetric W [n * n] (a NaN counts as +inf; the diagonal is not read) under the total
// order (w, max(a, b), min(a, b)), rooted at `root`: parent[root] = -1, parent[v] the next node on v's path to the root,
// wsel[v] = W[v][parent[v]] (wsel[root] = 0).  One workgroup, no atomics: two calls give identical bytes.
// 1 <= n <= CGMR_TREE_MAX_NODES, 0 <= root < n.
void launch_min_spanning_tree(hipStream_t st, int n, const double* W, int root, int32_t* parent, double* wsel);
// The edges parent[k] -> k of nodes k = 1 .. n - 1 at `poses`, edge k - 1 of the outputs: est [3] the relative pose, info [6]
// the upper triangle of its information, flags 0, 1 (no Cholesky factor: identity information) or 2 (wsel[k] = +inf: the node
// hangs on the tree by no finite weight, identity information).  A parent with slot -1 (the gauge): label_star_edge
// (label_device.h); otherwise the unscented transform over both ends, 13 sigma points of the 6x6 joint covariance.
void launch_tree_labels(hipStream_t st, const TreeNodes& N, const int32_t* parent, const double* wsel, const double* poses,
                        const double* G, double* est, double* info, int32_t* flags);

}  // namespace cgmr
