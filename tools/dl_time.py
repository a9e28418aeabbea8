"""Device ms of dogleg (cgmr_dl_optimize) against Gauss-Newton (cgmr_gn_optimize) and Levenberg-Marquardt
(cgmr_lm_optimize) on the C2 graph (10 000 poses, 40 000 edges), the same number of iterations, warm (the analysis cache
hit), the three alternated.  Device ms: events on the context's stream around the call (the whole call: uploads, every
pass, read-backs, and the host's waits between rounds, if any).  Then the cost of a head and of a rejected tail, on C2 with
bad_start's headings (every free heading moved by N(0, 3 rad)): a one-iteration call with max_trials = 1 is one head and
one tail; a one-iteration call with the default max_trials runs T trials on that head, so (t_T - t_1) / (T - 1) is the
device time per rejected tail (the host waits between its rounds included).
Usage: python tools/dl_time.py [iters] [reps]"""
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
p_bad = g["poses"].copy()
rng = np.random.default_rng(21)
p_bad[1:, 2] = synth.normalize_theta(p_bad[1:, 2] + 3.0 * rng.standard_normal(len(p_bad) - 1))
b = (p_bad,) + a[1:]
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


runs = {
    "gn": lambda: ctx.gn_optimize(*a, ITERS),
    "lm": lambda: ctx.lm_optimize(*a, ITERS),
    "dl": lambda: ctx.dl_optimize(*a, ITERS),
    "head+tail": lambda: ctx.dl_optimize(*b, 1, max_trials=1),
    "head+T tails": lambda: ctx.dl_optimize(*b, 1),
}
for fn in runs.values():
    fn()                                                     # (warm-up: analysis, kernel loading)
res = {k: ([], []) for k in runs}
info = {}
for k in range(REPS):
    for name, fn in runs.items():
        w, d, out = timed(fn)
        res[name][0].append(w)
        res[name][1].append(d)
        if name == "dl":
            info["dl"] = (ctx.dl_last_stats(), out[4].tolist(), out[5].tolist())
        if name == "head+T tails":
            info["T"] = ctx.dl_last_stats()
med = {}
for name in runs:
    w, d = np.array(res[name][0]), np.array(res[name][1])
    med[name] = float(np.median(d))
    print(f"{name:>13}: device ms median {np.median(d):.3f} (min {d.min():.3f}), wall ms median {np.median(w):.3f}")
st, tri, stp = info["dl"]
print(f"dl / gn device: {med['dl'] / med['gn']:.3f}; dl / lm device: {med['dl'] / med['lm']:.3f}; dl trials per iteration {tri}, "
      f"steps {stp}, host waits {st['host_waits']}, factorisations {st['factorisations']}")
T = info["T"]["trials"]
print(f"bad start on C2, one iteration: T = {T} trials, {info['T']['host_waits']} host waits, "
      f"{info['T']['factorisations']} factorisation(s); device ms per rejected tail "
      f"{(med['head+T tails'] - med['head+tail']) / max(T - 1, 1):.4f}; head + one tail {med['head+tail']:.3f}")
ctx.close()
