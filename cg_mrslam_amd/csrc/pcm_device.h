// Device side of the pairwise consistency maximisation of closure candidates (pcm_kernels.hip; include/cgmr.h:
// cgmr_closure_consistency, cgmr_max_clique_greedy), and the readers of the Gram tiles that it shares with
// joint_marginals_kernels.hip.
//
// The clique search is the greedy heuristic PCM implementations use (seed, then repeatedly the candidate with most neighbours
// left, over every seed): it returns a maximal clique, NOT a maximum one.  The exact solver (clique_exact_kernels.hip;
// cgmr_max_clique_exact, cgmr_closure_consistency_exact) starts from that clique's size and returns a maximum one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cgmr {

// Element (ca, cb) of Y^T Y (columns of Y) out of the lower tiles: tile (I, J), J <= I, at position pos.  The element of a
// diagonal tile is read from its lower half, so that (ca, cb) and (cb, ca) are the same double whatever the tile.
__device__ __forceinline__ double gram_at(const double* __restrict__ G, long long pos, int ca, int cb) {
  int r = ca & 15, c = cb & 15;
  if ((ca >> 4) < (cb >> 4) || ((ca >> 4) == (cb >> 4) && r < c)) { const int t = r; r = c; c = t; }
  return G[(size_t)pos * 256 + r * 16 + c];
}

// position of the tile that holds (ca, cb) in the dense layout: every lower tile, (I, J) at I (I + 1) / 2 + J
__device__ __forceinline__ long long dense_pos(int ca, int cb) {
  int I = ca >> 4, J = cb >> 4;
  if (I < J) { const int t = I; I = J; J = t; }
  return (long long)I * (I + 1) / 2 + J;
}

// The candidates of a consistency call on the device: closure k goes from vertex a[k] to b[k] and measures x_a^-1 x_b as
// meas[3 k ..] with information info[6 k ..] (upper triangle); slot[2 k], slot[2 k + 1]: the 4-column group of Y of a[k] and
// b[k] among the unique endpoints, or -1 (fixed / inactive: zero rows of Sigma).
struct PcmClosures {
  int n = 0;
  const int32_t *a = nullptr, *b = nullptr, *slot = nullptr;
  const double *meas = nullptr, *info = nullptr;
};

// d2 [n * n], symmetric with an exact zero diagonal, from the dense tile set G (joint_marginals_kernels.hip) at `poses`
void launch_closure_consistency(hipStream_t st, const PcmClosures& C, const double* poses, const double* G, double* d2);
// The candidates of an inter-robot consistency call (cgmr_closure_consistency_inter): closure k goes from the own vertex a[k]
// to a peer's vertex with the pose peer[3 k ..] (in the peer's frame; only p_k^-1 p_l enters) and measures x_a^-1 x_p;
// slot[k]: the 4-column group of Y of a[k] among the unique own endpoints, or -1.  peer_cov [3 n * 3 n], row-major, indexed by
// candidate: the joint covariance of the peer poses, of which only the lower triangle is read; null: Sigma_p = 0, the peer's
// poses are taken as exact (as LoopClosureChecker takes them).  That under-states S, so the gate d2 < gamma is stricter than
// the data justify: consistent candidates may be refused, inconsistent ones are not let in.
struct PcmInterClosures {
  int n = 0;
  const int32_t *a = nullptr, *slot = nullptr;
  const double *peer = nullptr, *peer_cov = nullptr, *meas = nullptr, *info = nullptr;
};
// d2 [n * n] as launch_closure_consistency writes it, for the two-graph form
void launch_closure_consistency_inter(hipStream_t st, const PcmInterClosures& C, const double* poses, const double* G, double* d2);
// adj [n * W], W = (n + 63) / 64: bit (l & 63) of word k * W + (l >> 6) = (k != l && d2[k][l] < gamma); padding bits zero
void launch_consistency_bits(hipStream_t st, int n, const double* d2, double gamma, unsigned long long* adj);
// The greedy clique of every seed (seed_bits [n * W]: its members, seed_size [n]), then the best of them: out[0] its size,
// out[1] its seed, out[2 ..] its members ascending, -1 behind them (out: n + 2 ints).  n >= 1; adj symmetric, zero diagonal.
void launch_clique_greedy(hipStream_t st, int n, const unsigned long long* adj, unsigned long long* seed_bits, int32_t* seed_size,
                          int32_t* out);

// What the exact solver works in (clique_exact_kernels.hip), W = (n + 63) / 64.  [2][n]: one entry per round and root.
#define CGMR_EXACT_ROUNDS 2
struct ExactWork {
  int32_t *vtx_of_pos = nullptr, *pos_of_vtx = nullptr;          // [n] each: the fixed order as bit positions
  unsigned long long* B = nullptr;                                // [n * W] the adjacency in bit positions
  unsigned long long* bits = nullptr;                             // [2][n][W] the clique a root found, in bit positions
  int32_t *size = nullptr, *out_of_nodes = nullptr;               // [2][n] its size (0: none above the bound); stopped early
  long long* nodes = nullptr;                                     // [2][n] nodes expanded
  unsigned long long* stack = nullptr;                            // [n][n][W] one P per root and depth
};
// The exact maximum clique behind launch_clique_greedy's result greedy_out (device, n + 2 ints) on the same stream: out[0] its
// size, out[1] proven (no root stopped at node_limit), out[2 ..] its members ascending, -1 behind them (n + 2 ints);
// nodes_out[0] the nodes expanded over all roots and rounds, at most n * CGMR_EXACT_ROUNDS * node_limit.  n >= 1,
// node_limit >= 1.  Five launches more than the greedy two.
void launch_clique_exact(hipStream_t st, int n, const unsigned long long* adj, long long node_limit, const int32_t* greedy_out,
                         const ExactWork& X, int32_t* out, long long* nodes_out);

}  // namespace cgmr
