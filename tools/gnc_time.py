"""Timing of graduated non-convexity (cgmr_gnc_optimize) and of the plain path beside it, on the C2 graph (10 000 poses,
40 000 edges).  Device ms: events on the context's stream around the call (the whole call: uploads, every pass, read-backs,
the host's waits between rounds), warm (the analysis cache hit).

  python tools/gnc_time.py plain [reps]
      gn_optimize(10): the median of ``reps`` (10) device timings and the final chi2 as hex, one line.  CGMR_LIB selects the
      library, so two builds are compared by running this in a process each, alternating.
  python tools/gnc_time.py gnc [reps]
      C2 with 1 % of its closures corrupted (tests/ref_robust.py: outlier_graph's recipe), the odometry chain as known inliers,
      TLS and GM at barc^2 = the 3-dimensional default and 21.1: outer iterations, host waits, device ms per outer iteration
      against a plain Gauss-Newton iteration on the same context, rejected against corrupted edges, RMS to the clean optimum
      (plain Gauss-Newton without the corrupted edges) beside Cauchy(3)'s and plain Gauss-Newton's."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cg_mrslam_amd import Context, synth  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "gnc"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
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


def median_ms(fn, reps=REPS):
    fn()                                                         # (warm-up: analysis, kernel loading)
    t = [timed(fn) for _ in range(reps)]
    return float(np.median([x[1] for x in t])), float(np.min([x[1] for x in t])), t[-1][2]


if MODE == "plain":
    g = synth.make_pose_graph(10000, 40000, seed=12345, strict=True)
    a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
    med, mn, out = median_ms(lambda: ctx.gn_optimize(*a, 10))
    print(f"plain gn_optimize(10) on C2: device ms median {med:.4f} min {mn:.4f} final chi2 {float(out[2][-1]).hex()} "
          f"lib {os.environ.get('CGMR_LIB', 'in-tree')}")
else:
    import ref_robust as RR  # noqa: E402
    g, bad, closure = RR.outlier_graph(nV=10000, nE=40000, seed=12345, frac=100, rng_seed=1)
    a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
    keep = np.ones(len(g["edge_from"]), bool)
    keep[bad] = False
    _, clean, _ = ctx.gn_optimize(g["poses"], g["fixed"], g["edge_from"][keep], g["edge_to"][keep], g["meas"][keep], g["info"][keep], 15)
    known = (~closure).astype(np.uint8)
    gn_med, _, out = median_ms(lambda: ctx.gn_optimize(*a, 10))
    print(f"C2, {len(bad)} of {int(closure.sum())} closures corrupted; plain gn_optimize(10): device ms {gn_med:.3f} "
          f"({gn_med / 10:.4f} per iteration), RMS to the clean optimum {RR.rms(out[1], clean):.4g} m")
    _, p, _, _, _ = ctx.gn_optimize_robust(*a, 10, kind="cauchy", delta=3.0)
    print(f"Cauchy(3) gn_optimize_robust(10): RMS to the clean optimum {RR.rms(p, clean):.4g} m")
    for loss in ("tls", "gm"):
        for c in (None, 21.1):
            for inner in (1, 2):
                fn = lambda: ctx.gnc_optimize(*a, loss=loss, barc_sq=c, known_inliers=known, inner_iters=inner)   # noqa: E731
                med, mn, o = median_ms(fn, max(REPS // 2, 3))
                st = ctx.gnc_last_stats()
                n = o["outer_done"]
                rej = np.flatnonzero(o["weights"] == 0.0) if loss == "tls" else np.flatnonzero(o["weights"] < 1e-3)
                print(f"GNC-{loss.upper()} barc^2 {c or 11.34:g} inner {inner}: outer {n}, waits {st['host_waits']}, device ms {med:.3f} "
                      f"({med / n:.4f} per outer iteration, {med / n / (gn_med / 10):.3f} x a plain iteration), rejected {len(rej)} "
                      f"(corrupted among them {len(np.intersect1d(rej, bad))} of {len(bad)}), RMS to the clean optimum "
                      f"{RR.rms(o['poses'], clean):.4g} m")
ctx.close()
