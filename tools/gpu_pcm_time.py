"""Timing of the pairwise consistency maximisation (cgmr_closure_consistency) on the benchmark graph (10 000 poses, 40 000
edges) after optimize(10), for N = 64, 256 and 1024 random closure candidates (a third of them outliers).

  python tools/gpu_pcm_time.py [reps]

Per N: wall ms of the whole call (host arrays in and out) and device ms (events on the context's stream around it), median and
minimum of ``reps`` (9) warm calls; the same for cgmr_relative_covariance over the same candidates taken singly (the pass, the
forward solve and the candidates' own tiles: the part both share); then, from one call in profiling mode
(cgmr_gn_kernel_times_ex, classes 9..11), the split into forward solve + Gram tiles, k_closure_consistency, and bit words +
clique -- the last separated with cgmr_max_clique_greedy on the same adjacency, which times the clique alone.  The device
memory the call stages is computed from the shapes.  The figures are in DESIGN.md section 2.14."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cg_mrslam_amd import Context, synth  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
GAMMA = 11.344866730144373
IU = np.array([500.0, 0, 0, 500.0, 0, 5000.0])
stream = torch.cuda.Stream(0)
ctx = Context(0, stream=stream.cuda_stream)

g = synth.make_pose_graph(10000, 40000, seed=12345, strict=True)
rest = (g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
rc, p, chi = ctx.gn_optimize(g["poses"], *rest, 10)
assert rc == 0
print(f"optimize(10): chi2 {chi[0]:.6g} -> {chi[-1]:.6f}")
nfree = int((g["fixed"] == 0).sum())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    t0 = time.perf_counter()
    out = fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1), out


def stats(fn):
    fn()
    t = [timed(fn) for _ in range(REPS)]
    w, d = [x[0] for x in t], [x[1] for x in t]
    return f"wall median {np.median(w):.3f} min {min(w):.3f} ms, device median {np.median(d):.3f} min {min(d):.3f} ms", t[-1][2]


def relative_pose(xa, xb):
    c, s = np.cos(xa[:, 2]), np.sin(xa[:, 2])
    dx, dy = xb[:, 0] - xa[:, 0], xb[:, 1] - xa[:, 1]
    return np.stack([c * dx + s * dy, -s * dx + c * dy, xb[:, 2] - xa[:, 2]], axis=1)


for N in (64, 256, 1024):
    rng = np.random.default_rng(N)
    V = len(p)
    ca = rng.integers(0, V, N).astype(np.int32)
    cb = ((ca + rng.integers(1, V, N)) % V).astype(np.int32)
    z = relative_pose(p[ca], p[cb]) + rng.normal(0, 1, (N, 3)) / np.sqrt(IU[[0, 3, 5]])
    out = rng.permutation(N)[:N // 3]
    z[out] += rng.choice([-1.0, 1.0], (len(out), 3)) * (np.array([1, 1, 0.3]) + rng.random((len(out), 3)) * np.array([4, 4, 1.5]))
    ci = np.tile(IU, (N, 1))
    nU = len(np.unique(np.r_[ca, cb]))
    m = (4 * nU + 15) // 16 * 16
    T = m // 16
    print(f"N = {N}: {nU} unique endpoints; Y {8 * 3 * nfree * m / 2**20:.1f} MiB, Gram tiles {2048 * T * (T + 1) // 2 / 2**20:.1f} MiB, "
          f"d2 {8 * N * N / 2**20:.3f} MiB")
    line, r = stats(lambda: ctx.closure_consistency(p, *rest, ca, cb, z, ci, GAMMA))
    d2, adj, clique, seed = r
    print(f"  closure_consistency: {line}; clique {len(clique)} of {N} (inliers {N - len(out)}), seed {seed}, "
          f"{int(adj.sum()) // 2} adjacent pairs")
    line, _ = stats(lambda: ctx.relative_covariance(p, *rest, ca, cb, z, ci))
    print(f"  relative_covariance, the candidates singly: {line}")
    line, _ = stats(lambda: ctx.max_clique_greedy(adj))
    print(f"  max_clique_greedy on that adjacency: {line}")
    ctx.set_profiling(True)
    ctx.closure_consistency(p, *rest, ca, cb, z, ci, GAMMA)
    full = ctx.pcm_kernel_times()
    ctx.set_profiling(True)                                        # (clears the sums)
    ctx.max_clique_greedy(adj)
    alone = ctx.pcm_kernel_times()
    ctx.set_profiling(False)
    bits = full["bits_clique"][0] - alone["bits_clique"][0]
    print(f"  split (one call, events per launch class): solve + Gram {1e3 * full['gram'][0]:.3f} ms, consistency "
          f"{1e3 * full['consistency'][0]:.3f} ms, bits + clique {1e3 * full['bits_clique'][0]:.3f} ms (the clique alone "
          f"{1e3 * alone['bits_clique'][0]:.3f} ms: bits about {1e3 * bits:.3f} ms)")
ctx.close()
