"""Node rate of the exact maximum-clique search (cgmr_max_clique_exact) and what a node limit costs, for the choice of
CGMR_EXACT_DEFAULT_NODE_LIMIT; then the exact call beside the greedy one on the candidate sets of tools/gpu_pcm_time.py.

  python tools/gpu_clique_exact_time.py [reps] [--no-pcm]

1. Random graphs G(1024, p), p = 0.5 .. 0.999, and node limits 64 .. 4096: device ms of one call (events on the
   context's stream; the median of ``reps`` (5) warm calls), the nodes it expanded, the share of the budget
   n * rounds * node_limit they are, and nodes per second over the call.  One wavefront works on each root and 1024 of them
   are resident at once, so a call lasts as long as its slowest root: the roots with the largest candidate sets, which in the
   dense graphs are the ones that run out of nodes in both rounds.  The largest time of a limit over the graphs is what
   "every one of 1024 roots runs out" costs at that limit; nodes per second per workgroup is limit * rounds over that time.
2. Unless --no-pcm: the benchmark graph after optimize(10) and the N = 64 / 256 / 1024 candidate sets of gpu_pcm_time.py (same
   generator): closure_consistency and closure_consistency_exact (device ms, median and minimum), the clique sizes, the
   inliers among them, proven, and max_clique_exact alone on the adjacency with its node count.
The figures are in DESIGN.md section 2.14."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cg_mrslam_amd import Context, synth  # noqa: E402
from cg_mrslam_amd._lib import EXACT_DEFAULT_NODE_LIMIT, EXACT_ROUNDS  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(ARGS[0]) if ARGS else 5
GAMMA = 11.344866730144373
IU = np.array([500.0, 0, 0, 500.0, 0, 5000.0])
stream = torch.cuda.Stream(0)
ctx = Context(0, stream=stream.cuda_stream)


def device_ms(fn):
    """(median, minimum) device ms of REPS warm calls, and the last result."""
    out = fn()
    t = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        out = fn()
        e1.record(stream)
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t)), float(min(t)), out


def random_graph(n, p, rng):
    U = np.triu(rng.random((n, n)) < p, 1)
    return U | U.T


print(f"default node limit {EXACT_DEFAULT_NODE_LIMIT}, {EXACT_ROUNDS} rounds")
n = 1024
worst = {}
for dens in (0.5, 0.9, 0.98, 0.995, 0.999):
    words, _ = Context._adj_words(random_graph(n, dens, np.random.default_rng(int(1000 * dens))))
    med, _, (greedy, _) = device_ms(lambda: ctx.max_clique_greedy(words))
    print(f"G({n}, {dens}): greedy clique {len(greedy)}, {med:.3f} ms", flush=True)
    for limit in (64, 256, 512, 1024, 2048, 4096):
        med, lo, (clique, proven, nodes) = device_ms(lambda: ctx.max_clique_exact(words, node_limit=limit))
        worst[limit] = max(worst.get(limit, 0.0), med)
        print(f"  node_limit {limit}: device median {med:.3f} min {lo:.3f} ms, clique {len(clique)}, proven {proven}, {nodes} nodes "
              f"= {nodes / (n * EXACT_ROUNDS * limit):.1%} of the budget, {nodes / (1e-3 * med):.3e} nodes/s over the call", flush=True)
        if med > 1000.0:
            break
for limit, ms in sorted(worst.items()):
    print(f"node_limit {limit}: slowest graph {ms:.3f} ms; per workgroup {limit * EXACT_ROUNDS / (1e-3 * ms):.3e} nodes/s if its slowest "
          f"root spent the whole budget")

if "--no-pcm" not in sys.argv:
    g = synth.make_pose_graph(10000, 40000, seed=12345, strict=True)
    rest = (g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
    rc, p, chi = ctx.gn_optimize(g["poses"], *rest, 10)
    assert rc == 0
    print(f"optimize(10): chi2 {chi[0]:.6g} -> {chi[-1]:.6f}")

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
        inl = np.ones(N, dtype=bool)
        inl[out] = False
        med, lo, (d2, adj, clique, seed) = device_ms(lambda: ctx.closure_consistency(p, *rest, ca, cb, z, ci, GAMMA))
        print(f"N = {N}: closure_consistency device median {med:.3f} min {lo:.3f} ms; clique {len(clique)}, of them inliers "
              f"{int(inl[clique].sum())} of {int(inl.sum())}", flush=True)
        med, lo, (d2x, adjx, cx, proven) = device_ms(lambda: ctx.closure_consistency_exact(p, *rest, ca, cb, z, ci, GAMMA))
        assert d2x.tobytes() == d2.tobytes() and adjx.tobytes() == adj.tobytes()
        print(f"  closure_consistency_exact device median {med:.3f} min {lo:.3f} ms; clique {len(cx)}, of them inliers "
              f"{int(inl[cx].sum())} of {int(inl.sum())}, proven {proven}", flush=True)
        med, lo, _ = device_ms(lambda: ctx.max_clique_greedy(adj))
        medx, lox, (c2, pr2, nodes) = device_ms(lambda: ctx.max_clique_exact(adj))
        print(f"  on that adjacency: max_clique_greedy {med:.3f} / {lo:.3f} ms, max_clique_exact {medx:.3f} / {lox:.3f} ms, "
              f"{nodes} nodes, proven {pr2}", flush=True)
ctx.close()
