"""Cost of robust condensed graphs (cgmr_graph_set_condensed_robust): C5's robots (synth.make_multi_robot(8, 5000, 20000,
seed=777)) on one GPU with the loopback exchange, lock step, condensed graphs waited for.  Every round, after the solves, each
robot builds the condensed graphs for all its peers (computeCondensedGraph(-1)) with the switch off and on, in alternating
order, Cauchy(1) on every own edge.  Prints one JSON line: the median over rounds of the summed per-robot times.
argv: robots rounds"""
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
n_rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 30
ctxs = [Context(0) for _ in range(nr)]
R = synth.make_multi_robot(nr, 5000, 20000, seed=777)
rounds = [RobotRounds(RobotGraph(ctxs[r], r, nr, cap_edges=128), RobotWorld(R, r, chunk=50)) for r in range(nr)]
ex = LoopbackExchange([r.g for r in rounds])
off_ms, on_ms, built = [], [], 0
try:
    for t in range(min(n_rounds, rounds[0].w.n_rounds)):
        for r in rounds:
            r.grow()
            r.optimize()
        ex.finish_all()
        tot = {False: 0.0, True: 0.0}
        for r in rounds:
            g = r.g
            if g.counts()["own_edges"] > 0:
                g.set_edge_robust("cauchy", 1.0)
            for on in (False, True) if t % 2 == 0 else (True, False):
                g.set_condensed_robust(on)
                t0 = time.perf_counter()
                n = g.computeCondensedGraph(-1)
                tot[on] += time.perf_counter() - t0
                built += n
            if t % 2:                                   # (what is sent: the plain graphs, as the round's own would be)
                g.set_condensed_robust(False)
                g.computeCondensedGraph(-1)
        if t >= 2:                                      # (the first rounds: structures and work spaces grow)
            off_ms.append(1e3 * tot[False])
            on_ms.append(1e3 * tot[True])
        ex.start_all()
    ex.finish_all()
finally:
    for r in rounds:
        r.g.close()
    for c in ctxs:
        c.close()
print(json.dumps(dict(robots=nr, rounds=len(off_ms), graphs_built=built, condense_off_ms_median=float(np.median(off_ms)),
                      condense_on_ms_median=float(np.median(on_ms)), ratio=float(np.median(np.array(on_ms) / np.array(off_ms))))))
