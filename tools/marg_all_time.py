"""Wall and device ms of the all-pose marginals (cgmr_marginals_all) on the C2 graph (10 000 poses, 40 000 edges), against the
query-based path (cgmr_marginals): marginals_all cold (analysis cache off) and warm (right after gn_optimize on the same edge
list), cgmr_marginals with 1 000 queries (warm), and with all 10 000 when its work space stays under 16 GB (otherwise the
bytes it would need are printed and the run is skipped).  Device ms: events on the context's stream around the call (the whole
call: uploads, Gauss-Newton pass, inversion, read-back).  Also prints the bytes of the Sigma blocks selected inversion keeps.
Usage: python tools/marg_all_time.py [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cg_mrslam_amd import Context, synth  # noqa: E402
from cg_mrslam_amd._lib import gn_front_table  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ARENA_CAP = 16 << 30

g = synth.make_pose_graph(10000, 40000, seed=12345, strict=True)
a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
V = len(g["poses"])
stream = torch.cuda.Stream(0)
ctx = Context(0, stream=stream.cuda_stream)
cold = Context(0, stream=stream.cuda_stream)
cold.set_symbolic_cache(False)
rc, p, _ = ctx.gn_optimize(*a, 5)
assert rc == 0
rest = (g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])


def timed(fn, reps=REPS, before=None):
    wall, dev = [], []
    for k in range(reps + 1):                                  # (the first call is a warm-up)
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        e1.record(stream)
        e1.synchronize()
        if k:
            wall.append(t1 - t0)
            dev.append(1e-3 * e0.elapsed_time(e1))
    return 1e3 * np.median(wall), 1e3 * np.median(dev), out


def line(name, w, d):
    print(f"{name:44s} wall {w:8.3f} ms   device {d:8.3f} ms", flush=True)


fr = gn_front_table(V, np.zeros(V, np.uint8), g["edge_from"], g["edge_to"])     # (c0, nc, ns, parent, level, children)
n = 3 * (fr[:, 1].astype(np.int64) + fr[:, 2])
print(f"C2: {len(fr)} fronts on {fr[:, 4].max() + 1} levels, largest border {3 * fr[:, 2].max()} rows; "
      f"Sigma blocks {8 * int((n * n).sum()) / 1e6:.1f} MB", flush=True)

w, d, cov = timed(lambda: cold.marginals_all(p, *rest))
line("marginals_all, cold (analysis every call)", w, d)
w, d, (cov_w, cross) = timed(lambda: ctx.marginals_all(p, *rest, cross=True), before=lambda: ctx.gn_optimize(p, *rest, 0))
line("marginals_all + cross, warm (after optimize)", w, d)
w, d, cov_w = timed(lambda: ctx.marginals_all(p, *rest))
line("marginals_all, warm", w, d)
assert np.array_equal(cov, cov_w)
q1000 = np.linspace(0, V - 1, 1000).astype(np.int32)
w, d, cq = timed(lambda: ctx.marginals(p, *rest, q1000), reps=max(3, REPS // 2))
line("marginals, 1000 queries, warm", w, d)
nz = np.abs(cq).sum(axis=(1, 2)) > 0
rel = np.linalg.norm(cov[q1000] - cq, axis=(1, 2))[nz] / np.linalg.norm(cq, axis=(1, 2))[nz]
print(f"  largest difference marginals_all / marginals on those 1000: {rel.max():.2e}")
# cgmr_marginals' work space for nK queries (marginals_host.cpp marginal_driver): Y (3 nf x m), the border vectors
# ((3 * border rows + 3) x m), the Gram partials (nchunk x 16 x m), m = 4 nK padded to 16
nf = V - int(g["fixed"].sum())
m = (4 * V + 15) // 16 * 16
need = 8 * m * (3 * nf + 3 * int(fr[:, 2].sum()) + 3 + 16 * ((3 * nf + 2047) // 2048) + 16)
if need <= ARENA_CAP:
    w, d, _ = timed(lambda: ctx.marginals(p, *rest, np.arange(V, dtype=np.int32)), reps=1)
    line(f"marginals, all {V} queries, warm", w, d)
else:
    print(f"marginals, all {V} queries: skipped, its work space would take {need / 2**30:.1f} GiB (> {ARENA_CAP / 2**30:.0f} GiB)")
