"""Timing of chordal initialisation (cgmr_chordal_initialize, stages = 3) beside two Gauss-Newton iterations
(cgmr_gn_optimize, iters = 2) on the same context, on the C2 graph (10 000 poses, 40 000 edges) with scrambled estimates.

  python tools/gpu_chordal_time.py [reps]

Wall ms of the whole call (host arrays in and out) and device ms (events on the context's stream around it), medians of
``reps`` (15) after a warm-up, first with the symbolic analysis cached, then with the cache off; the ratio chordal / GN(2) for
each; then the kernel classes' times of one call each from cgmr_gn_kernel_times_ex (profiling mode), which say where a ratio
above 1 goes.  The figures are in DESIGN.md section 2.11."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cg_mrslam_amd import Context, synth  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
stream = torch.cuda.Stream(0)
ctx = Context(0, stream=stream.cuda_stream)

g = synth.make_pose_graph(10000, 40000, seed=12345)
rng = np.random.default_rng(12345)
poses = g["poses"].copy()
free = g["fixed"] == 0
poses[free, 2] = -rng.uniform(-np.pi, np.pi, int(free.sum()))
poses[free, :2] += 5.0 * rng.standard_normal((int(free.sum()), 2))
rest = (g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    t0 = time.perf_counter()
    out = fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1), out


def medians(fn):
    fn()
    t = [timed(fn) for _ in range(REPS)]
    return float(np.median([x[0] for x in t])), float(np.median([x[1] for x in t])), t[-1][2]


def chordal():
    return ctx.chordal_initialize(poses, *rest, 3)


start = chordal()["poses"]                                       # Gauss-Newton runs from the chordal result: a regular system


def gn2():
    return ctx.gn_optimize(start, *rest, 2)


for cached in (True, False):
    ctx.set_symbolic_cache(cached)
    cw, cd, out = medians(chordal)
    gw, gd, _ = medians(gn2)
    print(f"analysis {'cached' if cached else 'not cached'}: chordal(3) wall {cw:.3f} ms device {cd:.3f} ms; gn_optimize(2) wall {gw:.3f} ms "
          f"device {gd:.3f} ms; ratio wall {cw / gw:.3f} device {cd / gd:.3f}")
print(f"chordal(3) from the scramble: chi2 {out['chi2'][0]:.4g} -> {out['chi2'][1]:.6g}, counts {out['counts'].tolist()}")
ctx.set_symbolic_cache(True)
chordal()
ctx.set_profiling(True)
for name, fn in (("chordal(3)", chordal), ("gn_optimize(2)", gn2)):
    before = ctx.gn_kernel_times()
    fn()
    after = ctx.gn_kernel_times()
    parts = {k: (1e3 * (after[k][0] - before[k][0]), after[k][1] - before[k][1]) for k in after}
    print(f"{name}: " + ", ".join(f"{k} {ms:.3f} ms / {n}" for k, (ms, n) in parts.items() if n) +
          f"; sum {sum(ms for ms, _ in parts.values()):.3f} ms")
ctx.set_profiling(False)
ctx.close()
