"""Device ms of one optimize(10) on the C2 graph (10 000 poses, 40 000 edges) for three settings: plain
(cgmr_gn_optimize), Huber on every edge (uniform kind / delta) and per-edge arrays (Cauchy on the closures, none on the
odometry).  HIP events on the context's stream around the whole call (uploads, every pass, read-backs); cold = the first
call of a setting after another edge list was analysed, warm = medians over repeats with the analysis cache hit, the three
settings alternated.
Usage: python tools/robust_time.py [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cg_mrslam_amd import Context, synth  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ITERS = 10

g = synth.make_pose_graph(10000, 40000, seed=12345, strict=True)
a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
closure = np.arange(len(g["edge_from"])) >= len(g["poses"]) - 1
kind = np.where(closure, 3, 0).astype(np.uint8)
delta = np.where(closure, 3.0, 1.0)
small = synth.make_pose_graph(500, 1500, seed=4)
sa = (small["poses"], small["fixed"], small["edge_from"], small["edge_to"], small["meas"], small["info"])
stream = torch.cuda.Stream(0)
ctx = Context(0, stream=stream.cuda_stream)

SETTINGS = {
    "plain": lambda: ctx.gn_optimize(*a, ITERS),
    "huber_uniform": lambda: ctx.gn_optimize_robust(*a, ITERS, kind="huber", delta=1.0),
    "per_edge_arrays": lambda: ctx.gn_optimize_robust(*a, ITERS, kind=kind, delta=delta),
}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


cold = {}
for name, fn in SETTINGS.items():
    ctx.gn_optimize(*sa, 1)                                  # (another edge list: the next call analyses C2 again)
    cold[name] = timed(fn)
warm = {name: [] for name in SETTINGS}
for _ in range(REPS):
    for name, fn in SETTINGS.items():
        warm[name].append(timed(fn))
base = np.median(warm["plain"])
for name in SETTINGS:
    d = np.array(warm[name])
    print(f"{name:16s} optimize({ITERS}): device ms cold {cold[name]:.3f}, warm median {np.median(d):.3f} (min {d.min():.3f}), "
          f"warm / plain {np.median(d) / base:.4f}")
ctx.close()
