"""Device ms of Levenberg-Marquardt (cgmr_lm_optimize) against Gauss-Newton (cgmr_gn_optimize) on the C2 graph (10 000
poses, 40 000 edges), the same number of iterations, warm (the analysis cache hit), the two alternated.  Device ms: events
on the context's stream around the call (the whole call: uploads, every pass, read-backs; for Levenberg-Marquardt also the
host's waits between rounds, if any).  Also prints the trials and the host waits of the Levenberg-Marquardt call.
Usage: python tools/lm_time.py [iters] [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cg_mrslam_amd import Context, synth  # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10

g = synth.make_pose_graph(10000, 40000, seed=12345, strict=True)
a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
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


gn = lambda: ctx.gn_optimize(*a, ITERS)                      # noqa: E731
lm = lambda: ctx.lm_optimize(*a, ITERS)                      # noqa: E731
gn()
lm()                                                         # (warm-up: analysis, kernel loading)
res = {"gn": ([], []), "lm": ([], [])}
stats = None
for k in range(REPS):
    for name, fn in (("gn", gn), ("lm", lm)):
        w, d, out = timed(fn)
        res[name][0].append(w)
        res[name][1].append(d)
        if name == "lm":
            stats = ctx.lm_last_stats()
            tri, done = out[4], out[5]
for name in ("gn", "lm"):
    w, d = np.array(res[name][0]), np.array(res[name][1])
    print(f"{name}_optimize({ITERS}): device ms median {np.median(d):.3f} (min {d.min():.3f}), wall ms median {np.median(w):.3f}")
ratio = np.median(res["lm"][1]) / np.median(res["gn"][1])
print(f"lm / gn device: {ratio:.3f}; lm iterations run {done}, trials per iteration {tri.tolist()}, "
      f"trials {stats['trials']}, host waits {stats['host_waits']}")
ctx.close()
