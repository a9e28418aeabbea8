// HIP kernels of the exact maximum-clique solver behind the pairwise consistency maximisation (include/cgmr.h:
// cgmr_max_clique_exact, cgmr_closure_consistency_exact): a branch and bound on the adjacency words the greedy kernels of
// pcm_kernels.hip read, with the greedy colouring bound of San Segundo's BBMC.  The greedy clique runs first, unchanged
// (launch_clique_greedy), and its size is the lower bound the search starts from.
//
//   k_exact_order     the fixed vertex order: ascending degree, ties by index; vertex v gets bit position n - 1 - rank(v), so
//                     that "later in the order" is "a lower bit" and the first set bit of a set is its member of highest degree
//   k_exact_permute   the adjacency in bit positions, B[p][q] = A[vertex(p)][vertex(q)], one __ballot per word
//   k_exact_search    one wavefront per root p: C = {p}, P = B[p] below bit p (the root's neighbours later in the order).  P and C
//                     are W <= 16 words across the lanes, one word per lane; the first set bit is a __ballot over the non-zero
//                     words and __ffsll, a count is __popcll and a wave reduction.  Four roots per workgroup share B in LDS.
//                     Explicit stack, one P per depth, in global scratch (n levels of 8 W bytes per root: with B in LDS there
//                     is no room for it there, and it is touched once per node where B is read once per vertex coloured); no
//                     recursion.  Launched ROUNDS = 2 times: round 0 with the greedy size as the bound, round 1 only
//                     for the roots that ran out of nodes in round 0, with the best size round 0 found as the bound.
//   k_exact_best      the largest clique over the roots and rounds, ties to the root first in the order; the greedy clique when
//                     no root beat it; members ascending, -1 behind them; proven and the node total
//
// The search at a node (C, P): nothing left in P: C is recorded if it is larger than the best so far.  Otherwise P is coloured
// greedily -- classes peeled off in bit order, Q &= ~B[v] -- and the node is left when |C| + colours <= best; else the last
// vertex that was coloured (it is in the highest class) joins C, the node keeps P without it on the stack, and the child
// (C + v, P & B[v]) is expanded; back at the node, what is left of P is coloured again.  The colour-ordered candidate list is
// not kept: a level costs W words, not n entries, and a node is coloured once more per child instead.
//
// Determinism: a workgroup reads the adjacency, the order, the greedy size and (round 1) what round 0 wrote; it writes only its
// own root's entries of the current round.  Nothing it reads changes during a launch; bounds pass from one launch to the next.
// No workgroup waits for another, nothing spins, every loop is bounded by n or by the node limit, no floating-point atomics
// (no atomics at all): two calls give identical bytes, proven and the node count included.
//
// Measured on an MI355X (tools/gpu_clique_exact_time.py): a node costs one colouring, a chain of |P| dependent
// steps, so the rate follows the candidate sets: over a call on G(1024, p) 4.1e7 nodes/s at p = 0.5, 2.0e7 at 0.9, 5.0e6 at
// 0.98, 1.0e6 at 0.995; the slowest workgroup of the slowest of these graphs (0.995, candidate sets of several hundred)
// expands 3.9e3 nodes/s, and a call at node_limit 512 takes 265 ms there, at 1024 524 ms: CGMR_EXACT_DEFAULT_NODE_LIMIT = 512.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcm_device.h"

namespace cgmr {

typedef unsigned long long u64;

// Bit position of every vertex and back.  One workgroup; n <= 1024.
__global__ __launch_bounds__(256) void k_exact_order(int n, int W, const u64* __restrict__ adj, int32_t* __restrict__ vtx_of_pos,
                                                     int32_t* __restrict__ pos_of_vtx) {
  __shared__ int deg[1024];
  const int tid = threadIdx.x;
  for (int v = tid; v < n; v += 256) {
    int d = 0;
    for (int w = 0; w < W; w++) d += __popcll(adj[(size_t)v * W + w]);
    deg[v] = d;
  }
  __syncthreads();
  for (int v = tid; v < n; v += 256) {
    const int dv = deg[v];
    int rank = 0;
    for (int u = 0; u < n; u++) rank += (deg[u] < dv || (deg[u] == dv && u < v)) ? 1 : 0;
    const int p = n - 1 - rank;
    pos_of_vtx[v] = p;
    vtx_of_pos[p] = v;
  }
}

// Word (p, w) of B: lane t tests A[vertex(p)][vertex(64 w + t)]; padding bits zero.
__global__ __launch_bounds__(64) void k_exact_permute(int n, int W, const u64* __restrict__ adj, const int32_t* __restrict__ vtx_of_pos,
                                                      u64* __restrict__ B) {
  const int w = blockIdx.x, p = blockIdx.y, q = 64 * w + (int)threadIdx.x;
  bool on = false;
  if (q < n) {
    const int v = vtx_of_pos[p], u = vtx_of_pos[q];
    on = (adj[(size_t)v * W + (u >> 6)] >> (u & 63)) & 1ull;
  }
  const u64 word = __ballot(on);
  if (threadIdx.x == 0) B[(size_t)p * W + w] = word;
}

namespace {

// the lowest set bit of a set held one word per lane (the same value in every lane), -1 when the set is empty
__device__ __forceinline__ int first_bit(u64 word) {
  const u64 m = __ballot(word != 0);
  if (!m) return -1;
  const int l = __ffsll((long long)m) - 1;                        // (wave-uniform: the lane's word is read as two scalars)
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)word, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(word >> 32), l);
  const u64 w = ((u64)hi << 32) | lo;
  return 64 * l + __ffsll((long long)w) - 1;
}

// |set|, the same value in every lane
__device__ __forceinline__ int count_bits(u64 word) {
  int c = __popcll(word);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  return c;
}

}  // namespace

// Root p = 4 blockIdx.x + wave: one wavefront per root, four roots per workgroup, which share a copy of B in LDS (8 n W bytes,
// 128 KiB at n = 1024: one workgroup per CU, 1024 roots resident at once) -- every step of a colouring is a row of B read at an
// address the step before it decides, so the row's latency is what a node costs.  The waves meet at one barrier, behind the
// copy, and never again.  Round 0: every root, bound = the greedy size.  Round 1: the roots whose round 0 ran out of nodes,
// bound = max(greedy size, the sizes round 0 found); the others write zeros.  X.size[round][p] = the size of the clique found
// (0: none above the bound), X.bits[round][p] its members in bit positions, X.out_of_nodes[round][p], X.nodes[round][p] = the
// (C, P) nodes expanded, the root's own counted.
__global__ __launch_bounds__(256) void k_exact_search(int n, int W, int round, long long node_limit, const int32_t* __restrict__ greedy_out,
                                                      ExactWork X) {
  __shared__ u64 B[1024 * 16];                                    // n <= 1024, W <= 16 (CGMR_PCM_MAX_CLOSURES)
  __shared__ uint16_t chosen_all[4][1024];                        // per wave: the vertex that joined C at every depth
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = 4 * blockIdx.x + wave;
  const size_t ro = (size_t)round * n + p;
  uint16_t* chosen = chosen_all[wave];
  if (round > 0) {                                                // (the same four flags in every thread of the workgroup)
    int open = 0;
    for (int k = 0; k < 4; k++) open |= 4 * blockIdx.x + k < n ? X.out_of_nodes[4 * blockIdx.x + k] : 0;
    if (!open) {                                                  // every root of the workgroup was settled in round 0
      if (lane == 0 && p < n) { X.size[ro] = 0; X.out_of_nodes[ro] = 0; X.nodes[ro] = 0; }
      return;
    }
  }
  for (int i = tid; i < n * W; i += 256) B[i] = X.B[i];
  __syncthreads();
  if (p >= n) return;                                             // (wave-uniform, as everything below)
  int best = greedy_out[0];
  if (round > 0) {
    int m = 0;
    for (int r = lane; r < n; r += 64) m = max(m, X.size[r]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
    best = max(best, m);
    if (!X.out_of_nodes[p]) {                                     // settled in round 0
      if (lane == 0) { X.size[ro] = 0; X.out_of_nodes[ro] = 0; X.nodes[ro] = 0; }
      return;
    }
  }
  u64* __restrict__ S = X.stack + (size_t)p * n * W;               // level d at S + d W
  // P = B[p] below bit p; C = {p}
  u64 P = 0, Cw = 0;
  if (lane < W) {
    const u64 below = lane < (p >> 6) ? ~0ull : lane == (p >> 6) ? (1ull << (p & 63)) - 1 : 0ull;
    P = B[p * W + lane] & below;
    Cw = lane == (p >> 6) ? 1ull << (p & 63) : 0ull;
  }
  int d = 0, found = 0, stopped = 0;
  long long nodes = 1;
  // every turn of the loop pushes one node (at most node_limit - 1 of them) or pops one
  for (long long turn = 0; turn < 2 * node_limit + 2; turn++) {
    const int csize = d + 1;
    const int left = count_bits(P);
    bool down = false;
    int vlast = -1;
    if (left == 0) {
      if (csize > best) {
        best = found = csize;
        if (lane < W) X.bits[ro * W + lane] = Cw;
      }
    } else if (csize + left > best) {
      // greedy colouring: R the uncoloured vertices that may still join the current class, Q the uncoloured ones
      u64 Q = P, R = 0;
      int ncol = 0;
      for (int step = 0; step < n; step++) {
        int v = first_bit(R);
        if (v < 0) {
          R = Q;
          v = first_bit(R);
          if (v < 0) break;
          ncol++;
        }
        vlast = v;
        const u64 bit = lane == (v >> 6) ? 1ull << (v & 63) : 0ull;
        const u64 a = lane < W ? B[v * W + lane] : 0ull;
        R &= ~(a | bit);
        Q &= ~bit;
      }
      down = csize + ncol > best;
    }
    if (down) {
      if (nodes >= node_limit || d + 1 >= n) { stopped = 1; break; }
      nodes++;
      const u64 bit = lane == (vlast >> 6) ? 1ull << (vlast & 63) : 0ull;
      if (lane < W) S[(size_t)d * W + lane] = P & ~bit;
      chosen[d] = (uint16_t)vlast;                                // (every lane the same value: each reads its own)
      Cw |= bit;
      P = lane < W ? P & B[vlast * W + lane] : 0ull;
      d++;
    } else {
      if (d == 0) break;
      d--;
      const int v = chosen[d];
      Cw &= ~(lane == (v >> 6) ? 1ull << (v & 63) : 0ull);
      P = lane < W ? S[(size_t)d * W + lane] : 0ull;
    }
  }
  if (lane == 0) { X.size[ro] = found; X.out_of_nodes[ro] = stopped; X.nodes[ro] = nodes; }
}

// out[0] = size, out[1] = proven, out[2 ..] the members ascending, -1 behind them; nodes_out[0] = the nodes of every root and
// round.  The winner: the largest size over roots and rounds, ties to the highest bit position (the root first in the order),
// of one root the later round; the greedy clique (greedy_out: size, seed, members) when no root found a larger one.
__global__ __launch_bounds__(256) void k_exact_best(int n, int W, const int32_t* __restrict__ greedy_out, ExactWork X,
                                                    int32_t* __restrict__ out, long long* __restrict__ nodes_out) {
  __shared__ u64 red[256];
  __shared__ long long nsum[256];
  __shared__ int open[256];
  __shared__ u64 member[16];
  const int tid = threadIdx.x;
  u64 best = 0;
  long long ns = 0;
  int op = 0;
  for (int p = tid; p < n; p += 256) {
    const int s0 = X.size[p], s1 = X.size[n + p];
    const int s = s1 > 0 ? s1 : s0, r = s1 > 0 ? 1 : 0;
    if (s > 0) {
      const u64 key = ((u64)s << 32) | ((u64)p << 1) | (u64)r;
      best = key > best ? key : best;
    }
    ns += X.nodes[p] + X.nodes[n + p];
    op |= X.out_of_nodes[p] ? X.out_of_nodes[n + p] : 0;
  }
  red[tid] = best; nsum[tid] = ns; open[tid] = op;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      if (red[tid + h] > red[tid]) red[tid] = red[tid + h];
      nsum[tid] += nsum[tid + h];
      open[tid] |= open[tid + h];
    }
    __syncthreads();
  }
  const int size = (int)(red[0] >> 32);
  if (size <= greedy_out[0]) {                                    // (0, or never above the bound it was searched with)
    for (int k = tid; k < n; k += 256) out[2 + k] = greedy_out[2 + k];
    if (tid == 0) { out[0] = greedy_out[0]; out[1] = open[0] ? 0 : 1; nodes_out[0] = nsum[0]; }
    return;
  }
  // the winner's members from bit positions to vertices: wave t / 64 of a pass tests 64 consecutive vertices
  const int p = (int)((red[0] & 0xFFFFFFFFull) >> 1), r = (int)(red[0] & 1ull);
  const u64* bits = X.bits + ((size_t)r * n + p) * W;
  for (int base = 0; base < 64 * W; base += 256) {
    const int v = base + tid;
    bool on = false;
    if (v < n) { const int q = X.pos_of_vtx[v]; on = (bits[q >> 6] >> (q & 63)) & 1ull; }
    const u64 word = __ballot(on);
    if ((tid & 63) == 0 && (v >> 6) < W) member[v >> 6] = word;
  }
  __syncthreads();
  if (tid != 0) return;
  out[0] = size;
  out[1] = open[0] ? 0 : 1;
  nodes_out[0] = nsum[0];
  int m = 0;
  for (int w = 0; w < W; w++) {
    u64 word = member[w];
    while (word) {
      out[2 + m++] = 64 * w + (__ffsll((long long)word) - 1);
      word &= word - 1;
    }
  }
  for (; m < n; m++) out[2 + m] = -1;
}

// ----------------------------------------------------------------------------------- launcher
void launch_clique_exact(hipStream_t st, int n, const unsigned long long* adj, long long node_limit, const int32_t* greedy_out,
                         const ExactWork& X, int32_t* out, long long* nodes_out) {
  const int W = (n + 63) / 64;
  if (node_limit > (1ll << 60)) node_limit = 1ll << 60;           // (2 node_limit + 2 turns; beyond any search)
  hipLaunchKernelGGL(k_exact_order, dim3(1), dim3(256), 0, st, n, W, adj, X.vtx_of_pos, X.pos_of_vtx);
  hipLaunchKernelGGL(k_exact_permute, dim3(W, n), dim3(64), 0, st, n, W, adj, X.vtx_of_pos, X.B);
  for (int round = 0; round < CGMR_EXACT_ROUNDS; round++)
    hipLaunchKernelGGL(k_exact_search, dim3((n + 3) / 4), dim3(256), 0, st, n, W, round, node_limit, greedy_out, X);
  hipLaunchKernelGGL(k_exact_best, dim3(1), dim3(256), 0, st, n, W, greedy_out, X, out, nodes_out);
}

}  // namespace cgmr
