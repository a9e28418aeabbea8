#!/usr/bin/env python3
"""Times the condensed graph as a spanning tree next to the star for the same queries.

    python tools/time_condense_tree.py [--reps 7] [--out FILE]

Per graph (the 1500/5000 graph, C2) and K = 16, 64, 128, 512 requested vertices, the gauge the middle one: condense (the
star), condense_tree, and marginals_joint over the same vertices with the same gauge fixed -- the forward solve and the dense
Gram tiles the tree adds to the star's pass, without the weights, the tree and the labels.  Whole calls, host staging and
read-back included, the analysis cached: the median of `reps` calls after two warm-up calls, in milliseconds.  Then the
spanning-tree kernel alone (profiling mode, device events around its one launch) on random weights at n = 129 and n = 1025:
its n - 1 dependent rounds are the part of the call that does not shrink with more compute units (call_ms beside it is the
whole min_spanning_tree call: the host's mirrored copy of the matrix, 8.4 MB up, the kernel, the parents back).  One JSON line
per row."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cg_mrslam_amd import Context, synth  # noqa: E402


def _median_ms(fn, reps):
    for _ in range(2):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    out = open(o.out, "w") if o.out else None

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")

    ctx = Context(0)
    for name, g in (("pg1500", synth.make_pose_graph(1500, 5000, seed=47)), ("c2", synth.make_pose_graph(10000, 40000, seed=12345))):
        a = (g["edge_from"], g["edge_to"], g["meas"], g["info"])
        rc, p, _ = ctx.gn_optimize(g["poses"], g["fixed"], *a, 5)
        assert rc == 0
        V = len(p)
        for K in (16, 64, 128, 512):
            q = np.linspace(1, V - 1, K).astype(np.int32)
            gauge = int(q[K // 2])
            fixed = np.zeros(V, np.uint8)
            fixed[gauge] = 1
            others = q[q != gauge]
            star = _median_ms(lambda: ctx.condense(p, *a, gauge, q), o.reps)
            tree = _median_ms(lambda: ctx.condense_tree(p, *a, gauge, q), o.reps)
            joint = _median_ms(lambda: ctx.marginals_joint(p, fixed, *a, others), o.reps)
            fr = ctx.condense_tree(p, *a, gauge, q)[0]
            emit(dict(graph=name, K=K, condense_ms=round(star, 3), condense_tree_ms=round(tree, 3), marginals_joint_ms=round(joint, 3),
                      edges_from_the_gauge=int((fr == gauge).sum())))
    for n in (129, 1025):
        W = np.random.default_rng(n).normal(size=(n, n))
        W = np.tril(W, -1) + np.tril(W, -1).T
        call = _median_ms(lambda: ctx.min_spanning_tree(W), o.reps)
        ctx.set_profiling(True)
        for _ in range(o.reps):
            ctx.min_spanning_tree(W)
        sec, launches = ctx.pcm_kernel_times()["bits_clique"]     # (class 11: here the spanning-tree launches alone)
        ctx.set_profiling(False)
        emit(dict(call="min_spanning_tree", n=n, call_ms=round(call, 3), kernel_ms=round(1e3 * sec / launches, 4), launches=launches))
    if out:
        out.close()


if __name__ == "__main__":
    main()
