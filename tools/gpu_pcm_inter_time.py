"""Timing of the inter-robot pairwise consistency (cgmr_closure_consistency_inter) on the benchmark graph (10 000 poses,
40 000 edges) after optimize(10), for N = 64, 256 and 1024 candidates from random own vertices to a peer's vertices (a third of
them outliers), beside cgmr_closure_consistency over as many candidates between the same own vertices and others of the graph.

  python tools/gpu_pcm_inter_time.py [reps]

Per N: wall ms of the whole call (host arrays in and out) and device ms (events on the context's stream around it), median and
minimum of ``reps`` (9) warm calls, for the inter call without a peer covariance, with one ([3 N, 3 N], a random positive
semidefinite matrix: its values do not change the work), and for the single-graph call; then, from one call each in profiling
mode (cgmr_gn_kernel_times_ex, classes 9..11), the split into forward solve + Gram tiles, the consistency kernel, and bit words
+ clique.  The device memory the calls stage is computed from the shapes.  The figures are in DESIGN.md section 2.14."""
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
FRAME = np.array([2.0, -1.0, 0.7])
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


def se2_mul(a, b):
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.stack([a[0] + c * b[:, 0] - s * b[:, 1], a[1] + s * b[:, 0] + c * b[:, 1], a[2] + b[:, 2]], axis=1)


def split(call):
    ctx.set_profiling(True)
    call()
    t = ctx.pcm_kernel_times()
    ctx.set_profiling(False)
    return (f"solve + Gram {1e3 * t['gram'][0]:.3f} ms, consistency {1e3 * t['consistency'][0]:.3f} ms, bits + clique "
            f"{1e3 * t['bits_clique'][0]:.3f} ms")


def tiles(nU):
    m = (4 * nU + 15) // 16 * 16
    T = m // 16
    return f"Y {8 * 3 * nfree * m / 2**20:.1f} MiB, Gram tiles {2048 * T * (T + 1) // 2 / 2**20:.1f} MiB"


for N in (64, 256, 1024):
    rng = np.random.default_rng(N)
    V = len(p)
    ca = rng.integers(0, V, N).astype(np.int32)
    cb = ((ca + rng.integers(1, V, N)) % V).astype(np.int32)
    peer = rng.uniform(-40, 40, (N, 3)) * [1, 1, np.pi / 40]
    z = relative_pose(p[ca], se2_mul(FRAME, peer)) + rng.normal(0, 1, (N, 3)) / np.sqrt(IU[[0, 3, 5]])
    z1 = relative_pose(p[ca], p[cb]) + rng.normal(0, 1, (N, 3)) / np.sqrt(IU[[0, 3, 5]])
    out = rng.permutation(N)[:N // 3]
    shift = rng.choice([-1.0, 1.0], (len(out), 3)) * (np.array([1, 1, 0.3]) + rng.random((len(out), 3)) * np.array([4, 4, 1.5]))
    z[out] += shift
    z1[out] += shift
    ci = np.tile(IU, (N, 1))
    B = rng.normal(0, 1, (3 * N, 24)) * 0.03
    pc = B @ B.T
    print(f"N = {N}: inter {len(np.unique(ca))} unique endpoints ({tiles(len(np.unique(ca)))}), single-graph "
          f"{len(np.unique(np.r_[ca, cb]))} ({tiles(len(np.unique(np.r_[ca, cb])))}); d2 {8 * N * N / 2**20:.3f} MiB, peer_cov "
          f"{72 * N * N / 2**20:.3f} MiB")
    calls = (("closure_consistency_inter, peer_cov None", lambda: ctx.closure_consistency_inter(p, *rest, ca, peer, z, ci, GAMMA)),
             ("closure_consistency_inter, peer_cov given", lambda: ctx.closure_consistency_inter(p, *rest, ca, peer, z, ci, GAMMA, peer_cov=pc)),
             ("closure_consistency", lambda: ctx.closure_consistency(p, *rest, ca, cb, z1, ci, GAMMA)))
    for name, call in calls:
        line, r = stats(call)
        print(f"  {name}: {line}; clique {len(r[2])} of {N} (inliers {N - len(out)})")
        print(f"    split (one call, events per launch class): {split(call)}")
ctx.close()
