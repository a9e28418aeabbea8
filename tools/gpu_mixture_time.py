"""Timing of the max-mixture path (cgmr_gn_optimize_mixture) beside the plain one, on the C2 graph (10 000 poses, 40 000 edges)
with K components on every closure: the true measurement last, the others gross (tests/ref_robust.py: outlier_graph's
corruption).  Device ms: events on the context's stream around the whole call (uploads, every pass, read-backs, the wait).

  python tools/gpu_mixture_time.py [reps] [K]
      gn_optimize(10) against gn_optimize_mixture(10), medians of ``reps`` (15), with the analysis cached and with the cache
      switched off (every call analyses the edge list again); the final mixture cost beside the plain chi2 of the true graph;
      the selection against the true index; the extra device time per iteration and per extra component evaluation."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cg_mrslam_amd import Context, synth  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
K = int(sys.argv[2]) if len(sys.argv) > 2 else 2
stream = torch.cuda.Stream(0)
ctx = Context(0, stream=stream.cuda_stream)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    t0 = time.perf_counter()
    out = fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1), out


def median_ms(fn, reps=REPS):
    fn()                                                         # (warm-up: analysis, kernel loading)
    t = [timed(fn) for _ in range(reps)]
    return float(np.median([x[1] for x in t])), float(np.median([x[0] for x in t])), t[-1][2]


g = synth.make_pose_graph(10000, 40000, seed=12345, strict=True)
a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
nV, nE = len(g["poses"]), len(g["edge_from"])
rng = np.random.default_rng(1)
closure = np.arange(nE) >= nV - 1
counts = np.where(closure, K, 1)
ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
cm, ci = np.repeat(g["meas"], counts, axis=0), np.repeat(g["info"], counts, axis=0)
wrong = np.ones(len(cm), bool)
wrong[ptr[1:] - 1] = False                                        # the last component of every edge: the true one
nw = int(wrong.sum())
cm[wrong, :2] += rng.choice([-1.0, 1.0], size=(nw, 2)) * rng.uniform(3, 10, size=(nw, 2))
cm[wrong, 2] = rng.uniform(-np.pi, np.pi, size=nw)
mix = (ptr, cm, ci, np.ones(len(cm)))
first = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], cm[ptr[:-1]], ci[ptr[:-1]])

print(f"C2: {nE} edges, {int(closure.sum())} closures with {K} components each, {len(cm)} components in all")
for cached in (True, False):
    ctx.set_symbolic_cache(cached)
    p_med, p_wall, p_out = median_ms(lambda: ctx.gn_optimize(*a, 10))
    m_med, m_wall, m_out = median_ms(lambda: ctx.gn_optimize_mixture(*first, 10, mix))
    print(f"analysis {'cached' if cached else 'not cached'}: gn_optimize(10) {p_med:.3f} ms device ({p_wall:.3f} wall), "
          f"gn_optimize_mixture(10) {m_med:.3f} ms device ({m_wall:.3f} wall): +{m_med - p_med:.3f} ms per call (uploads, 11 linearisations, "
          f"the selection's read-back)")
ctx.set_symbolic_cache(True)
sel = m_out[3]
print(f"final mixture cost {m_out[2][-1]:.6f} against the plain chi2 of the true graph {p_out[2][-1]:.6f}; "
      f"selection equals the true index on {int((sel == counts - 1).sum())} of {nE} edges; "
      f"largest pose difference to the plain result {float(np.abs(m_out[1] - p_out[1]).max()):.3e}")
up_plain, up_mix = 72 * nE, 80 * len(cm) + 4 * (nE + 1)
print(f"host-to-device bytes per call beside the poses: plain {up_plain} (meas, info), mixture {up_mix} (the component lists and "
      f"offsets; the first components are not sent); read back: {4 * nE} bytes of selection")
lin_us = []
ctx.set_profiling(True)                                           # the kernel classes' own times (cgmr_gn_kernel_times_ex)
for name, fn in (("gn_optimize(10)", lambda: ctx.gn_optimize(*a, 10)), ("gn_optimize_mixture(10)", lambda: ctx.gn_optimize_mixture(*first, 10, mix))):
    fn()
    before = ctx.gn_kernel_times()
    for _ in range(5):
        fn()
    after = ctx.gn_kernel_times()
    parts = {k: (1e3 * (after[k][0] - before[k][0]) / 5, (after[k][1] - before[k][1]) // 5) for k in after}
    lin = parts["linearize"]
    print(f"{name}: linearize {1e3 * lin[0] / lin[1]:.2f} us per launch ({lin[1]} launches), all kernels {sum(ms for ms, _ in parts.values()):.3f} ms per call")
    lin_us = lin_us + [1e3 * lin[0] / lin[1]]
extra_evals = (len(cm) - nE) + int(closure.sum())                 # K + 1 evaluations on a K-component edge, 1 on a plain one
print(f"linearisation: +{lin_us[1] - lin_us[0]:.2f} us per launch for {extra_evals} extra error evaluations "
      f"({1e3 * (lin_us[1] - lin_us[0]) / extra_evals:.3f} ns each across the device) and {80 * len(cm) - 72 * nE} more bytes read")
ctx.set_profiling(False)
plain0 = ctx.gn_optimize(*first, 10)
print(f"plain Gauss-Newton on the first components: chi2 {plain0[2][-1]:.6g}, largest pose difference {float(np.abs(plain0[1] - p_out[1]).max()):.3g} m")
ctx.close()
