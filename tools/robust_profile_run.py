"""The C2 solve under three robust settings for a rocprofv3 --kernel-trace --stats run (tools/robust_time.py's settings, five
optimize(10) calls each after a warm-up): the per-kernel stats separate k_linearize's plain and robust instances."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from cg_mrslam_amd import Context, synth  # noqa: E402

g = synth.make_pose_graph(10000, 40000, seed=12345, strict=True)
a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
closure = np.arange(len(g["edge_from"])) >= len(g["poses"]) - 1
ctx = Context(0)
ctx.gn_optimize(*a, 1)
for _ in range(5):
    ctx.gn_optimize(*a, 10)
    ctx.gn_optimize_robust(*a, 10, kind="huber", delta=1.0)
    ctx.gn_optimize_robust(*a, 10, kind=np.where(closure, 3, 0).astype(np.uint8), delta=np.where(closure, 3.0, 1.0))
ctx.close()
print("done")
