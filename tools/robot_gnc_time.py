"""Cost of GNC on the robot graph (cgmr_graph_optimize_gnc) and of condensed graphs under stored weights
(cgmr_graph_set_condensed_gnc): C5's robots (synth.make_multi_robot(8, 5000, 20000, seed=777)) on one GPU with the loopback
exchange, lock step, all rounds.  At the end every robot holds its full graph and its peers' stars; then, per robot and
warm, `reps` times each:
  * computeCondensedGraph(-1) with the switch off and on (every stored weight 1), in alternating order;
  * after appending `n_bad` grossly wrong closures between own vertices: optimize(10) and optimize_gnc (TLS, default c, every
    edge free) from the same estimates -- the wall time inside the call per Gauss-Newton iteration / per outer iteration.
Prints one JSON line: medians over the repetitions, summed over the robots for the condensed batches, per robot (median, min,
max over the robots) for the solves.
argv: robots reps n_bad"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cg_mrslam_amd import Context, synth  # noqa: E402
from cg_mrslam_amd.condensed import RobotGraph  # noqa: E402
from cg_mrslam_amd.mrslam import LoopbackExchange, RobotRounds, RobotWorld  # noqa: E402

nr = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
n_bad = int(sys.argv[3]) if len(sys.argv) > 3 else 6
ctxs = [Context(0) for _ in range(nr)]
R = synth.make_multi_robot(nr, 5000, 20000, seed=777)
rounds = [RobotRounds(RobotGraph(ctxs[r], r, nr, cap_edges=128), RobotWorld(R, r, chunk=50)) for r in range(nr)]
ex = LoopbackExchange([r.g for r in rounds])
out = dict(robots=nr, reps=reps, n_bad=n_bad)
try:
    for t in range(rounds[0].w.n_rounds):
        for r in rounds:
            r.grow()
            r.optimize()
        ex.finish_all()
        for r in rounds:
            r.condense()
        ex.start_all()
    ex.finish_all()
    # condensed batches, switch off / on at all-ones weights
    off, on = np.zeros(reps), np.zeros(reps)
    for r in rounds:
        g = r.g
        g.optimize(5)
        assert np.all(g.gnc_weights() == 1.0)
        for k in range(reps + 1):                       # (the first repetition warms the work spaces up)
            for sw in (False, True) if k % 2 == 0 else (True, False):
                g.set_condensed_gnc(sw)
                t0 = time.perf_counter()
                g.computeCondensedGraph(-1)
                dt = time.perf_counter() - t0
                if k > 0:
                    (on if sw else off)[k - 1] += 1e3 * dt
        g.set_condensed_gnc(False)
    out.update(condense_off_ms=[float(np.median(off)), float(off.min()), float(off.max())],
               condense_on_ms=[float(np.median(on)), float(on.min()), float(on.max())],
               condense_ratio=float(np.median(on / off)))
    # the solves
    rng = np.random.default_rng(5)
    plain_it, gnc_it, outer, rejected, sizes = [], [], [], [], []
    for r in rounds:
        g, ids = r.g, r.w.ids
        a = rng.choice(len(ids), n_bad, replace=False)
        b = (a + len(ids) // 2) % len(ids)
        z = np.c_[rng.uniform(-5, 5, (n_bad, 2)), rng.uniform(-3, 3, n_bad)]
        g.add_edges(ids[a], ids[b], z, np.tile([100.0, 0, 0, 100.0, 0, 1000.0], (n_bad, 1)))
        p0 = g.poses()
        tp, tg = [], []
        for k in range(reps + 1):
            g.set_poses(0, p0)
            g.optimize(10)
            tp.append(1e3 * g.last_seconds()["optimize"] / 10)
            g.set_poses(0, p0)
            res = g.optimize_gnc("tls", raise_on_cholesky=False)
            tg.append(1e3 * g.last_seconds()["optimize"] / max(res["outer_done"], 1))
        plain_it.append(float(np.median(tp[1:])))
        gnc_it.append(float(np.median(tg[1:])))
        outer.append(res["outer_done"])
        rejected.append(int(np.sum(res["weights"] == 0.0)))
        c = g.counts()
        sizes.append([c["vertices"], c["own_edges"], c["received_edges"]])
    med = lambda v: [float(np.median(v)), float(np.min(v)), float(np.max(v))]   # noqa: E731
    out.update(plain_iteration_ms=med(plain_it), gnc_outer_iteration_ms=med(gnc_it), outer_done=outer, rejected=rejected,
               ratio=med(np.array(gnc_it) / np.array(plain_it)), sizes=sizes)
finally:
    for r in rounds:
        r.g.close()
    for c in ctxs:
        c.close()
print(json.dumps(out))
