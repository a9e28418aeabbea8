"""The scan matcher's sub-cell refinement on the GPU (include/cgmr.h, "Refining a match below the grid's resolution")
against the float64 yardstick of tests/ref_match_refine.py: numpy over ``oracle.rasterize``.

Bars (derived, not measured; the response tests' own): the sums are of <= 640 double terms, relative rounding about
1e-13, times the condition bound tests/test_match_refine_cpu.py asserts on the yardstick (1e4) for what goes through the
3x3 solves -- so the pose agrees to 1e-9 of the bound per coordinate, the costs to 1e-9 cost0, the scores to 1e-9 of the
fill value, the Hessian to 1e-8 of its largest entry; the counters, the stop code and the at_bound bits are equal (the
same file asserts that no decision of the yardstick hangs on less than 1e-11 and no point comes within 1e-9 cells of a
cell boundary, which keeps ``floor`` and the comparisons stable).

Shapes: 160-point queries (less than one pass of the workgroup's 512 threads), 120 for the corridor, 640 for `dense` (a
thread sums two points; the room itself has only 320 points, so it is taken twice), the 0.025 m grid of `sparse` for
more tiles.
"""
import os

import numpy as np
import pytest

from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import CgmrError
from cg_mrslam_amd.matcher import LCScanMatcher, RefineParams, ScanMatcher
from cg_mrslam_amd.slam import SM_INFO, GraphSLAMDriver, run_srslam

import ref_match_refine as RR

pytestmark = pytest.mark.gpu

NAMED = ("room", "corridor", "rotated", "clamped", "sparse", "pinned", "dense")
COARSE = ("room", "corridor", "rotated", "clamped", "pinned", "dense")     # the cases on ref_match_response.GRID


def _matcher(ctx, grid):
    ll, ur, res, kr, ks = grid
    m = ScanMatcher(ctx, 1081, -2.35, 0.004, 30.0, resolution=res, kernel_range=kr)
    m.initializeGrid(ll, ur, res)
    m.cfg.kscale = ks
    return m


@pytest.fixture(scope="module")
def runs(oracle):
    """name -> (case, the yardstick's result); computed once, never changed."""
    cases = RR.named_cases(oracle)
    assert tuple(cases) == NAMED
    return {n: (c, RR.refine(oracle, c["grid"], c["ref"], c["qry"], c["theta_res"], c["winner"], c["params"])) for n, c in cases.items()}


def _got(ctx, case, **kw):
    return _matcher(ctx, case["grid"]).matchRefine(case["ref"], case["qry"], case["theta_res"], case["winner"],
                                                   RefineParams(**case["params"]), **kw)


def _check(got, want, what):
    """The bars of the module docstring; every figure is printed before it is asserted."""
    ints = ("status", "stop", "n_iters", "n_halvings", "n_active", "at_bound")
    print(f"{what}: " + " ".join(f"{k} {got[k]}/{want[k]}" for k in ints))
    gaps = dict(pose=np.max(np.abs(got["pose"] - want["pose"]) / want["bound"]), cost=abs(got["cost"] - want["cost"]) / want["cost0"],
                cost0=abs(got["cost0"] - want["cost0"]) / want["cost0"], score=abs(got["score"] - want["score"]) / want["fill"],
                score0=abs(got["score0"] - want["score0"]) / want["fill"],
                hessian=np.max(np.abs(got["hessian"] - want["hessian"])) / np.max(np.abs(want["hessian"])))
    print(f"{what}: " + " ".join(f"{k} gap {v:.3e}" for k, v in gaps.items()))
    for k in ints:
        assert got[k] == want[k], (what, k)
    assert gaps["pose"] <= 1e-9, (what, gaps)
    assert gaps["cost"] <= 1e-9 and gaps["cost0"] <= 1e-9, (what, gaps)
    assert gaps["score"] <= 1e-9 and gaps["score0"] <= 1e-9, (what, gaps)
    assert gaps["hessian"] <= 1e-8, (what, gaps)


def _is_untouched(r, winner, status):
    assert r["status"] == status and np.array_equal(r["pose"], np.asarray(winner)[:3])
    for k in ("cost0", "cost", "score0", "score", "n_active", "n_iters", "n_halvings", "stop", "at_bound"):
        assert r[k] == 0, k
    assert not r["hessian"].any()


@pytest.mark.parametrize("name", NAMED)
def test_parity_with_the_yardstick(ctx, runs, name):
    case, want = runs[name]
    assert want["status"] == 0
    got = _got(ctx, case)
    _check(got, want, name)
    assert got["cost"] <= got["cost0"]


def test_batch_equals_the_single_calls_and_is_deterministic(ctx, runs):
    # a batch shares its grid and its parameters: the cases of the coarse grid under the default parameters, one skipped job
    m = _matcher(ctx, runs["room"][0]["grid"])
    tres = runs["room"][0]["theta_res"]
    jobs = [(runs[n][0]["ref"], runs[n][0]["qry"], runs[n][0]["winner"]) for n in COARSE]
    jobs.append((jobs[0][0], jobs[0][1], None))
    a = m.matchRefineBatch(jobs, tres, raw=True)
    size = len(a) // len(jobs)
    assert size * len(jobs) == len(a) and size == 152
    for k, (ref, qry, win) in enumerate(jobs[:-1]):
        assert a[k * size:(k + 1) * size] == m.matchRefine(ref, qry, tres, win, raw=True), COARSE[k]
    got = m.matchRefineBatch(jobs, tres)
    _is_untouched(got[-1], np.zeros(3), 2)                       # the search before found nothing
    for n in ("room", "rotated", "dense"):                       # (the cases whose own parameters are the defaults)
        _check(got[COARSE.index(n)], runs[n][1], f"batch job {n} against the yardstick")
    assert m.matchRefineBatch(jobs, tres, raw=True) == a
    # every case under its own parameters and on its own grid, beside a skipped job
    for n in NAMED:
        case = runs[n][0]
        mm, par = _matcher(ctx, case["grid"]), RefineParams(**case["params"])
        b = mm.matchRefineBatch([(case["ref"], case["qry"], None), (case["ref"], case["qry"], case["winner"])], case["theta_res"], par, raw=True)
        single = mm.matchRefine(case["ref"], case["qry"], case["theta_res"], case["winner"], par, raw=True)
        assert b[size:] == single, n
        assert single == mm.matchRefine(case["ref"], case["qry"], case["theta_res"], case["winner"], par, raw=True), n
    assert m.matchRefineBatch([], tres) == []


def test_nothing_to_refine(ctx, runs):
    case, _ = runs["room"]
    m = _matcher(ctx, case["grid"])
    win = case["winner"]
    _is_untouched(m.matchRefine(case["ref"], np.zeros((0, 2)), case["theta_res"], win), win, 1)            # no query point
    _is_untouched(m.matchRefine(case["ref"], np.full((7, 2), 7.0), case["theta_res"], win), win, 1)         # all of them off the grid
    _is_untouched(m.matchRefine(case["ref"], case["qry"], case["theta_res"], None), np.zeros(3), 2)
    # points off the grid beside the others: the pose stays, the cost rises by the fill value's square each
    off = np.stack([np.full(20, 5.5), np.linspace(-1, 1, 20)], axis=1)
    a = m.matchRefine(case["ref"], case["qry"], case["theta_res"], win)
    b = m.matchRefine(case["ref"], np.concatenate([case["qry"], off]), case["theta_res"], win)
    print(f"off-grid points: pose gap {np.max(np.abs(a['pose'] - b['pose'])):.3e} cost rise {b['cost'] - a['cost']:.17g}")
    assert np.max(np.abs(a["pose"] - b["pose"])) <= 1e-12 and abs((b["cost"] - a["cost"]) - 20 * (25 / 128) ** 2) <= 1e-12
    assert b["n_active"] == a["n_active"] == 160


@pytest.mark.parametrize("bad,word", [
    (dict(max_iters=0), "max_iters"), (dict(max_iters=65), "max_iters"), (dict(max_halvings=-1), "max_halvings"),
    (dict(max_halvings=17), "max_halvings"), (dict(ridge=-1e-9), "ridge"), (dict(ridge=float("nan")), "ridge"),
    (dict(ridge=float("inf")), "ridge"), (dict(step_tol=0.0), "step_tol"), (dict(step_tol=float("inf")), "step_tol"),
    (dict(step_tol=float("nan")), "step_tol"), (dict(bound_steps=0.0), "bound_steps"), (dict(bound_steps=-1.0), "bound_steps"),
    (dict(bound_steps=float("nan")), "bound_steps")])
def test_invalid_parameters_are_refused(ctx, runs, bad, word):
    case, _ = runs["room"]
    m = _matcher(ctx, case["grid"])
    with pytest.raises(CgmrError, match=word):
        m.matchRefine(case["ref"], case["qry"], case["theta_res"], case["winner"], RefineParams(**bad))
    with pytest.raises(CgmrError, match=word):
        m.matchRefineBatch([(case["ref"], case["qry"], case["winner"])], case["theta_res"], RefineParams(**bad))


def test_a_winner_that_is_not_finite_is_refused(ctx, runs):
    case, _ = runs["room"]
    m = _matcher(ctx, case["grid"])
    for k, v in ((0, float("nan")), (1, float("inf")), (2, float("-inf")), (3, float("nan"))):
        win = case["winner"].copy()
        win[k] = v
        with pytest.raises(CgmrError, match="winner"):
            m.matchRefine(case["ref"], case["qry"], case["theta_res"], win)
        with pytest.raises(CgmrError, match="winner"):
            m.matchRefineBatch([(case["ref"], case["qry"], case["winner"]), (case["ref"], case["qry"], win)], case["theta_res"])


def test_close_matching_with_the_refinement_behind_it(ctx):
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "match_close12.npz"))
    cm = ScanMatcher(ctx, d["ranges_ref"].shape[1], float(d["angle_min"]), float(d["angle_inc"]), float(d["max_range"]))
    par = RefineParams()
    n_found = 0
    for p in range(4):
        scans = [(d["ranges_ref"][p], np.zeros(3))]
        f0, t0 = cm.closeScanMatchingVSet(scans, 0, d["ranges_qry"][p], d["guess"][p])
        f1, t1, ref = cm.closeScanMatchingVSet(scans, 0, d["ranges_qry"][p], d["guess"][p], refine=par)
        assert f0 == f1 == bool(d["found"][p])
        if not f0:
            assert t1 is None and ref["status"] == 2 and ref["search"] is None
            continue
        n_found += 1
        assert t0.tobytes() == ref["search"].tobytes() == d["xyt"][p].tobytes()          # the search is the plain call's, bit for bit
        assert ref["status"] == 0 and ref["cost"] <= ref["cost0"] and np.array_equal(t1, ref["pose"])
        step = np.array([float(np.float32(cm.cfg.resolution))] * 2 + [cm.cfg.theta_res])
        assert np.all(np.abs(t1 - t0) <= par.bound_steps * step)
        # the same points through the generic call (the laser sits at the robot's origin: the transform is exact)
        assert not any(cm.cfg.laser_pose[k] for k in range(3))
        refp = cm.transformPointsFromVSet(scans, 0)
        qry = cm.subsample(cm.cartesian(d["ranges_qry"][p]), cm.cfg.subsample_res)
        g = cm.matchRefine(refp, qry, cm.cfg.theta_res, [t0[0], t0[1], t0[2], 0.0], par)
        print(f"pair {p}: {ref['n_iters']} moves, stop {ref['stop']}, cost {ref['cost0']:.6g} -> {ref['cost']:.6g}, "
              f"gap to the generic call {np.max(np.abs(g['pose'] - t1)):.3e}")
        assert np.array_equal(g["pose"], t1) and g["cost"] == ref["cost"] and g["n_iters"] == ref["n_iters"]
        # with the response as well: both as their own calls give them
        f2, t2, info, resp, ref2 = cm.closeScanMatchingVSet(scans, 0, d["ranges_qry"][p], d["guess"][p], covariance_T=0.01, refine=par)
        _, _, info0, _ = cm.closeScanMatchingVSet(scans, 0, d["ranges_qry"][p], d["guess"][p], covariance_T=0.01)
        assert f2 and np.array_equal(t2, t1) and np.array_equal(info, info0) and resp["status"] == 0 and ref2["stop"] == ref["stop"]
    assert n_found >= 2
    f, t, ref = cm.closeScanMatchingVSet([(d["ranges_ref"][0], np.zeros(3))], 0, d["ranges_qry"][0], d["guess"][0], maxScore=1e-9, refine=par)
    assert not f and t is None and ref["status"] == 2 and ref["cost"] == 0 and not ref["hessian"].any()


def _run(ctx, tr, **kw):
    la = (tr["n_beams"], tr["angle_min"], tr["angle_inc"], tr["max_range"])
    slam = GraphSLAMDriver(ctx, ScanMatcher(ctx, *la), LCScanMatcher(ctx, *la), **kw)
    run_srslam(slam, tr["odom"], tr["scans"], linearUpdate=0.5)
    return slam


def test_driver_puts_the_refined_pose_on_scan_match_edges(ctx):
    tr = synth.make_trajectory(16, laps=0.04)                    # the smallest run with three scan-match edges
    plain = _run(ctx, tr)                                         # never names the option
    none = _run(ctx, tr, sm_refine=None)
    assert plain.sm_refine is None and none.edge_kind == plain.edge_kind and plain.edge_kind.count("sm") >= 3
    for k in ("ids", "poses", "fixed", "edge_from", "edge_to", "meas", "info"):
        assert getattr(none.g, k).tobytes() == getattr(plain.g, k).tobytes(), k
    assert not [l for l in none.log if l[0] == "sm_refine"]
    b = _run(ctx, tr, sm_refine=RefineParams())
    sm = [k for k, kind in enumerate(b.edge_kind) if kind == "sm"]
    logged = [l for l in b.log if l[0] == "sm_refine"]
    assert len(sm) == len(logged) >= 3
    moved = 0
    for k, l in zip(sm, logged):
        _, vid, status, stop, moves, r = l
        assert int(b.g.ids[b.g.edge_to[k]]) == vid and (status, stop, moves) == (r["status"], r["stop"], r["n_iters"])
        expect = r["pose"] if status == 0 else r["search"]
        assert np.array_equal(b.g.meas[k], expect) and r["cost"] <= r["cost0"]
        assert np.array_equal(b.g.info[k], SM_INFO)                                     # (sm_information is untouched: the constant)
        moved += int(status == 0 and moves > 0)
    assert moved >= 1
    with pytest.raises(ValueError):
        GraphSLAMDriver(ctx, None, None, sm_refine=0.5)
