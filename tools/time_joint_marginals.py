#!/usr/bin/env python3
"""Times the joint / pairwise marginals next to cgmr_marginals for the same queries.

    python tools/time_joint_marginals.py [--reps 7] [--out FILE]

Per graph (the 1500/5000 graph, C2): marginals_joint for 64 and 512 queries, the same blocks through the tile list
(marginals_pairs over every pair of the 64), marginals_pairs over the graph's edges (as many as fit the limit on unique
vertices), and cgmr_marginals for the same vertices.  Whole calls, host staging and read-back included: the median of
`reps` calls after two warm-up calls, in milliseconds, with the bytes of Y one contraction reads.  One JSON line per row."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cg_mrslam_amd import Context, synth  # noqa: E402
from cg_mrslam_amd._lib import JOINT_MAX_QUERIES  # noqa: E402


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
    ctx = Context(0)
    for name, g in (("pg1500", synth.make_pose_graph(1500, 5000, seed=47)), ("c2", synth.make_pose_graph(10000, 40000, seed=12345))):
        a = (g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
        rc, p, _ = ctx.gn_optimize(g["poses"], *a, 5)
        assert rc == 0
        V = len(p)
        n_rows = 3 * int((np.asarray(g["fixed"]) == 0).sum())
        rows = []

        def row(what, nq, n_unique, tiles, ms, rows=rows):
            # every contracted tile reads its two 16-column slices of Y over all rows (the dense layout shares them 4 ways)
            rows.append(dict(graph=name, call=what, queries=nq, unique=n_unique, tiles=tiles, ms=round(ms, 3),
                             y_bytes=8 * n_rows * 4 * n_unique))

        for nK in (64, 512):
            q = np.linspace(1, V - 1, nK).astype(np.int32)
            T = nK // 4
            row("marginals", nK, nK, T, _median_ms(lambda: ctx.marginals(p, *a, q), o.reps))
            row("marginals_joint", nK, nK, T * (T + 1) // 2, _median_ms(lambda: ctx.marginals_joint(p, *a, q), o.reps))
            if nK == 64:
                k, l = np.tril_indices(nK)
                row("marginals_pairs(all pairs of the queries)", len(k), nK, T * (T + 1) // 2,
                    _median_ms(lambda: ctx.marginals_pairs(p, *a, q[k], q[l]), o.reps))
        ef, et = g["edge_from"], g["edge_to"]
        m = (ef < JOINT_MAX_QUERIES) & (et < JOINT_MAX_QUERIES)          # the edges among the first vertices: within the limit
        ea, eb = ef[m], et[m]
        nu = len(np.unique(np.r_[ea, eb]))
        row("marginals_pairs(edges)", int(m.sum()), nu, -1, _median_ms(lambda: ctx.marginals_pairs(p, *a, ea, eb), o.reps))
        row("marginals(the edges' vertices)", nu, nu, (nu + 3) // 4,
            _median_ms(lambda: ctx.marginals(p, *a, np.unique(np.r_[ea, eb]).astype(np.int32)), o.reps))
        row("marginals_all(cross)", V, V, -1, _median_ms(lambda: ctx.marginals_all(p, *a, cross=True), o.reps))
        for r in rows:
            line = json.dumps(r)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
