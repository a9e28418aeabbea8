#!/usr/bin/env python3
"""What one vertex-removal call costs on C2, beside one Gauss-Newton iteration on the same graph from the same run
(DESIGN.md section 2.15).

    python tools/gpu_remove_nodes_time.py [--reps 7] [--out FILE]

The removed set is a maximal independent set of C2's free vertices with at most 16 distinct neighbours, taken greedily in
index order.  remove_nodes: the whole call (the host's checks and its CSR of incident edges, the edge list up, one launch, the
new edges back), the median of `reps` calls after two warm-up calls, and the kernel alone (profiling mode, device events around
its one launch).  gn_optimize(1): the whole call with the analysis cached, and its device share (cgmr_gn_last_timing).  One JSON
line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cg_mrslam_amd import Context, synth  # noqa: E402
from cg_mrslam_amd._lib import REMOVE_MAX_DEGREE  # noqa: E402


def independent_set(nV, fixed, ef, et, max_degree):
    """Greedy in index order: the free vertices with at most max_degree distinct neighbours, none adjacent to one taken."""
    adj = [set() for _ in range(nV)]
    for a, b in zip(ef.tolist(), et.tolist()):
        adj[a].add(b)
        adj[b].add(a)
    blocked = np.zeros(nV, dtype=bool)
    out = []
    for v in range(nV):
        if fixed[v] or blocked[v] or len(adj[v]) > max_degree:
            continue
        out.append(v)
        blocked[list(adj[v])] = True
    return np.array(out, dtype=np.int32), np.array([len(adj[v]) for v in out])


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
    g = synth.make_pose_graph(10000, 40000, seed=12345)
    a = (g["edge_from"], g["edge_to"], g["meas"], g["info"])
    nV = len(g["poses"])
    remove, deg = independent_set(nV, g["fixed"], a[0], a[1], REMOVE_MAX_DEGREE)
    ctx = Context(0)
    call = _median_ms(lambda: ctx.remove_nodes(*a, remove, num_vertices=nV), o.reps)
    off, fr, to, z, iu, w, fl = ctx.remove_nodes(*a, remove, num_vertices=nV)
    ctx.set_profiling(True)
    for _ in range(o.reps):
        ctx.remove_nodes(*a, remove, num_vertices=nV)
    sec, launches = ctx.pcm_kernel_times()["bits_clique"]          # (class 11: here the removal launches alone)
    ctx.set_profiling(False)
    gn, dev = [], []
    for k in range(o.reps + 2):
        t0 = time.perf_counter()
        rc, _, _ = ctx.gn_optimize(g["poses"], g["fixed"], *a, 1)
        assert rc == 0
        if k >= 2:
            gn.append(time.perf_counter() - t0)
            dev.append(ctx.gn_last_timing()["device"])
    r = dict(graph="c2", vertices=nV, edges=len(a[0]), removed=int((fl == 0).sum()), requested=len(remove), new_edges=len(to),
             degree_mean=round(float(deg.mean()), 2), degree_max=int(deg.max()), flags=np.bincount(fl, minlength=4).tolist(),
             remove_nodes_call_ms=round(call, 3), remove_nodes_kernel_ms=round(1e3 * sec / launches, 4), launches=launches,
             gn_iteration_call_ms=round(1e3 * float(np.median(gn)), 3), gn_iteration_device_ms=round(1e3 * float(np.median(dev)), 3))
    line = json.dumps(r)
    print(line, flush=True)
    if o.out:
        with open(o.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
