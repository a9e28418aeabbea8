"""Dogleg on the device (cgmr_dl_optimize, Context.dl_optimize, GraphSLAM(algorithm="dl"), RobotGraph.set_algorithm("dl"))
against the float64 reference of the contract, tests/ref_dogleg.py."""
import numpy as np
import pytest

import ref_dogleg
import ref_numpy as R
import ref_robust as RR
import reference_cases as C
from switch_contexts import assert_launch_shape, context_under
from test_dogleg_cpu import FIXED, EF, ET, INFO, MEAS
from test_lm_cpu import EXTRA_CASES
from test_lm_gpu import rounding_floor

pytestmark = pytest.mark.gpu

U = np.finfo(np.float64).eps / 2
ITERS = 5
RTOL = 1e-9
SMALL_DELTA = ("pg2500", "c2", "lat80", "wrap", "illcond")


def _cases():
    out = {name: (builder, ITERS) for name, (builder, _) in C.CASES.items()}
    out.update({k: v for k, v in EXTRA_CASES.items() if k != "no_fixed"})
    return out


CASES = _cases()
_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = (EXTRA_CASES[name][0] if name in EXTRA_CASES else C.CASES[name][0])()
    return _GRAPHS[name]


DRIFT_RTOL = 1e-4   # after a step that carries the Gauss-Newton step (GN, or DL through beta hgn): far from the optimum such a step
                    # amplifies the factorisation's rounding (another elimination order than SuperLU's) by cond(H), and every
                    # later iterate inherits it -- tests/test_gn_gpu.py measures 6.3e-7 on C2 for plain Gauss-Newton; here the
                    # largest seen is 2.6e-5 (illcond, whose H is ill-conditioned on purpose, with initial_delta = 1)
ILL_DRIFT_RTOL = 1e-2   # the same for illcond with the defaults: full GN steps on its H (measured 1.1e-3)
VARIANT_RTOL = 1e-6  # two launch variants of the same device code: the bar of tests/test_gn_gpu.py (CHI_RTOL)


def tolerances(ref, drift=DRIFT_RTOL):
    """Per iteration, the relative tolerance of its delta and of the chi2 after it: RTOL up to and including the first
    iteration whose accepted step carries hgn (GN or DL), ``drift`` after it.  An SD step is alpha b, which only sums."""
    tol = np.full(max(ref["iters_done"], 1) + 1, RTOL)
    for t in ref["trace"]:
        if t["accept"] and t["step"] != ref_dogleg.STEP_SD:
            tol[t["iteration"] + 1:] = drift
            break
    return tol


def compared_iterations(ref, floor=0.0, drift=DRIFT_RTOL):
    """Iterations of the reference decided by more than rounding: up to (excluding) the first with a trial where
    |currentChi - tempChi| is within 1e3 u (or ten times the iteration's tolerance) of currentChi, or currentChi <= floor
    (rho is rounding there), or where |hgn| or |hsd| lies within the tolerance of delta (the step's kind is rounding
    there); everything after it may differ."""
    tol = tolerances(ref, drift)
    for t in ref["trace"]:
        r = tol[t["iteration"]]
        near = [abs(n - t["delta"]) <= max(1e-9, r) * t["delta"] for n in (t["hgn_norm"], t["hsd_norm"]) if np.isfinite(n)]
        if abs(t["current"] - t["temp"]) <= max(1e3 * U, 10 * r) * abs(t["current"]) or abs(t["current"]) <= floor or any(near):
            return t["iteration"], False
    return ref["iters_done"], True


def check_trace(name, ref, chi, dlt, tri, stp, done, floor=0.0):
    drift = ILL_DRIFT_RTOL if name == "illcond" else DRIFT_RTOL
    k, whole = compared_iterations(ref, floor, drift)
    tol = tolerances(ref, drift)
    floor = max(floor, 1e3 * U * abs(ref["chi2"][0]))         # (a chi2 below 1e3 u of the starting one is rounding)
    assert np.array_equal(tri[:k], ref["trials"][:k]), (name, tri[:k], ref["trials"][:k])
    assert np.array_equal(stp[:k], ref["steps"][:k]), (name, stp[:k], ref["steps"][:k])
    rel = np.abs(dlt[:k] - ref["deltas"][:k]) / np.abs(ref["deltas"][:k])
    assert np.all(rel <= tol[:k]), (name, rel, tol[:k])
    if abs(ref["chi2"][0]) > floor:
        err = np.abs(chi[:k + 1] - ref["chi2"][:k + 1])
        assert np.all(err <= tol[:k + 1] * np.abs(ref["chi2"][:k + 1]) + floor), (name, err / np.abs(ref["chi2"][:k + 1]), tol[:k + 1])
    if whole:
        assert done == ref["iters_done"], (name, done, ref["iters_done"])
        assert np.all(tri[done:] == 0) and np.all(stp[done:] == 0) and np.all(dlt[done:] == 0)
        assert np.allclose(chi, ref["chi2"], rtol=tol[-1], atol=floor)
    return k


@pytest.fixture(scope="module")
def ctx():
    from cg_mrslam_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(CASES))
def test_trace_matches_reference(ctx, name):
    g, iters = graph(name), CASES[name][1]
    ref = ref_dogleg.dl_optimize(*C.args(g), iters)
    rc, poses, chi, dlt, tri, stp, done = ctx.dl_optimize(*C.args(g), iters)
    assert rc == 0
    k = check_trace(name, ref, chi, dlt, tri, stp, done, rounding_floor(g))
    assert k >= 1 or name in ("v2e1", "v5e4", "chain3000"), (name, "nothing compared")
    assert abs(chi[-1] - R.chi2(poses, *C.args(g)[2:])) <= RTOL * chi[-1] + rounding_floor(g)   # its own estimate's chi2
    fx = R.active_fixed(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    assert np.array_equal(poses[fx != 0], g["poses"][fx != 0])
    if name == "bad_start":
        assert np.all(np.diff(chi) <= 0) and tri[0] > 1
    if name == "indefinite":
        assert ref["lambdas"].size > 3 and ctx.dl_last_stats()["factorisations"] == ref["lambdas"].size


@pytest.mark.parametrize("name", SMALL_DELTA)
def test_small_initial_delta_takes_sd_and_dl_steps(ctx, name):
    g = graph(name)
    ref = ref_dogleg.dl_optimize(*C.args(g), ITERS, initial_delta=1.0)
    rc, poses, chi, dlt, tri, stp, done = ctx.dl_optimize(*C.args(g), ITERS, initial_delta=1.0)
    assert rc == 0
    k = check_trace(name, ref, chi, dlt, tri, stp, done, rounding_floor(g))
    assert k >= 2
    assert abs(chi[-1] - R.chi2(poses, *C.args(g)[2:])) <= RTOL * chi[-1] + rounding_floor(g)
    assert ref_dogleg.STEP_SD in stp[:k].tolist() or ref_dogleg.STEP_DL in stp[:k].tolist()


def test_small_delta_cases_cover_both_kinds(ctx):
    kinds = set()
    for name in SMALL_DELTA:
        kinds.update(ctx.dl_optimize(*C.args(graph(name)), ITERS, initial_delta=1.0)[5].tolist())
    assert {ref_dogleg.STEP_SD, ref_dogleg.STEP_DL} <= kinds


def test_no_fixed_vertex_stays_finite_and_never_rises(ctx):
    g = EXTRA_CASES["no_fixed"][0]()
    rc, poses, chi, dlt, tri, stp, done = ctx.dl_optimize(*C.args(g), 10, raise_on_fail=False)
    assert rc == 0 or rc <= -100
    assert np.all(np.isfinite(poses)) and np.all(np.isfinite(chi))
    assert np.all(np.diff(chi) <= 0)


@pytest.mark.parametrize("name", ["pg2500", "c2", "wrap"])
def test_dogleg_steps_have_length_delta(ctx, name):
    g = graph(name)
    p, fixed, ef, et, meas, info = C.args(g)
    t = ref_dogleg.dl_optimize(p, fixed, ef, et, meas, info, 1)["trace"][0]
    d = 0.5 * (t["hsd_norm"] + t["hgn_norm"])
    assert t["hsd_norm"] < d < t["hgn_norm"]
    rc, x1, chi, dlt, tri, stp, done = ctx.dl_optimize(p, fixed, ef, et, meas, info, 1, initial_delta=d)
    assert rc == 0 and stp.tolist() == [ref_dogleg.STEP_DL] and tri.tolist() == [1]
    h = x1 - p
    h[:, 2] = R.normalize_theta(h[:, 2])
    assert abs(np.linalg.norm(h) - d) <= 1e-9 * d, (np.linalg.norm(h), d)


def test_rejected_trials_leave_the_poses_bit_identical(ctx):
    g = graph("bad_start")
    ref = ref_dogleg.dl_optimize(*C.args(g), 1)
    assert not ref["trace"][0]["accept"]
    rc, poses, chi, dlt, tri, stp, done = ctx.dl_optimize(*C.args(g), 3, max_trials=1)
    assert rc == 0 and done == 1 and tri.tolist() == [1, 0, 0]
    assert np.array_equal(poses, g["poses"]) and np.all(chi == chi[0])
    assert dlt[0] == 0.5e4


def test_a_rejected_trial_needs_no_factorisation(ctx):
    g = graph("bad_start")
    ref = ref_dogleg.dl_optimize(*C.args(g), 1)
    rc, _, _, _, tri, _, done = ctx.dl_optimize(*C.args(g), 1)
    assert rc == 0 and tri[0] == ref["trials"][0] > 3
    st = ctx.dl_last_stats()
    assert st["factorisations"] == 1 and st["trials"] == tri[0]
    rc, _, _, _, tri, _, done = ctx.dl_optimize(*C.args(g), 10)
    st = ctx.dl_last_stats()
    assert st["factorisations"] <= st["trials"] == int(np.sum(tri)) and st["factorisations"] == done


def test_one_wait_when_every_first_trial_is_accepted(ctx):
    g = graph("c2")
    ref = ref_dogleg.dl_optimize(*C.args(g), 4)
    assert np.all(ref["trials"] == 1)
    rc, _, _, _, tri, _, done = ctx.dl_optimize(*C.args(g), 4)
    assert rc == 0 and done == 4 and np.all(tri == 1)
    assert ctx.dl_last_stats() == dict(host_waits=1, trials=4, factorisations=4)


def test_repeats_are_bit_identical(ctx):
    for name, kw in (("pg2500", dict(initial_delta=1.0)), ("bad_start", {}), ("indefinite", {})):
        g, iters = graph(name), CASES[name][1]
        a = ctx.dl_optimize(*C.args(g), iters, **kw)
        b = ctx.dl_optimize(*C.args(g), iters, **kw)
        for u, v in zip(a, b):
            assert np.array_equal(np.asarray(u), np.asarray(v)), name


def test_symbolic_cache_hit_after_gauss_newton(ctx):
    g = graph("pg500")
    ctx.gn_optimize(*C.args(g), 2)
    s0 = ctx.symbolic_cache_stats()
    rc, *_ = ctx.dl_optimize(*C.args(g), 3)
    s1 = ctx.symbolic_cache_stats()
    assert rc == 0 and s1["hits"] == s0["hits"] + 1 and s1["misses"] == s0["misses"] and s1["extended"] == s0["extended"]


def test_edge_cases_as_the_reference(ctx):
    # at the optimum (b = 0 exactly): GN steps of length 0, rho = 0, max_trials of them, Terminate
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    ref = ref_dogleg.dl_optimize(p, FIXED, EF, ET, MEAS, INFO, 4, max_trials=7)
    rc, x, chi, dlt, tri, stp, done = ctx.dl_optimize(p, FIXED, EF, ET, MEAS, INFO, 4, max_trials=7)
    assert rc == 0 and done == ref["iters_done"] == 1 and tri.tolist() == [7, 0, 0, 0] and stp.tolist() == [2, 0, 0, 0]
    assert dlt[0] == ref["deltas"][0] and np.array_equal(x, p) and np.all(chi == 0)
    # nothing free
    both = np.array([1, 1], np.uint8)
    ref = ref_dogleg.dl_optimize(p + 0.5, both, EF, ET, MEAS, INFO, 3)
    rc, x, chi, dlt, tri, stp, done = ctx.dl_optimize(p + 0.5, both, EF, ET, MEAS, INFO, 3)
    assert rc == 0 and done == 1 and tri.tolist() == [100, 0, 0] and dlt[0] == ref["deltas"][0]
    assert np.allclose(chi, ref["chi2"], rtol=1e-14, atol=0)
    # no iterations
    rc, x, chi, dlt, tri, stp, done = ctx.dl_optimize(p + 0.5, FIXED, EF, ET, MEAS, INFO, 0)
    assert rc == 0 and done == 0 and chi.shape == (1,) and np.array_equal(x, p + 0.5)
    # bad parameters: refused before anything runs
    from cg_mrslam_amd._lib import CgmrError
    with pytest.raises(CgmrError):
        ctx.dl_optimize(p, FIXED, EF, ET, MEAS, INFO, 1, lambda_factor=0.5)


def test_fail_past_the_largest_lambda(ctx):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = dict(graph("indefinite"))
    info = g["info"].copy()
    info[40] = [-1e5, 0, 0, info[40][3], 0, info[40][5]]
    g["info"] = info
    ref = ref_dogleg.dl_optimize(*C.args(g), 3)
    assert ref["failed"] == 0
    rc, poses, chi, dlt, tri, stp, done = ctx.dl_optimize(*C.args(g), 3, raise_on_fail=False)
    assert rc == -100 and done == 0 and np.all(tri == 0)
    assert np.array_equal(poses, g["poses"]) and np.allclose(chi, ref["chi2"], rtol=RTOL, atol=0)
    assert ctx.dl_last_stats()["factorisations"] == ref["lambdas"].size
    s = GraphSLAM(PoseGraph.from_synth(g), ctx, algorithm="dl")
    s.optimize(3)
    assert s.last_status == -100 and s.last_iterations == 0 and np.array_equal(s.graph.poses, g["poses"])


def test_graph_slam_dogleg(ctx):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = graph("bad_start")
    s = GraphSLAM(PoseGraph.from_synth(g), ctx, algorithm="dl")
    assert s.trustRegion() == 1e4 and s.lastStep() == 0
    s.optimize(10)
    ref = ref_dogleg.dl_optimize(*C.args(g), 10)
    assert s.last_status == 0 and s.last_iterations == ref["iters_done"]
    assert s.trustRegion() == pytest.approx(ref["deltas"][-1], rel=RTOL)
    assert s.lastStep() == ref["steps"][-1]
    assert np.allclose(s.last_chi2, ref["chi2"], rtol=RTOL, atol=0)


@pytest.mark.parametrize("name", ["pg2500", "outlier"])
def test_robust_dogleg_matches_reference(ctx, name):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = RR.outlier_graph()[0] if name == "outlier" else graph(name)
    a = C.args(g)
    ref = ref_dogleg.dl_optimize(*a, 6, kind=3, delta=3.0)
    rc, p, chi, dlt, tri, stp, done, e2, w = ctx.dl_optimize(*a, 6, kind="cauchy", delta=3.0)
    assert rc == 0
    k = check_trace(name, ref, chi, dlt, tri, stp, done, rounding_floor(g))
    assert k >= 2
    np.testing.assert_allclose(w, RR.rho(3, 3.0, e2)[1], rtol=1e-12, atol=1e-300)
    s = GraphSLAM(PoseGraph.from_synth(g), ctx, algorithm="dl")
    s.setRobustKernel("Cauchy", 3.0)
    s.optimize(6)
    assert s.last_status == 0 and np.allclose(s.last_chi2, chi, rtol=RTOL, atol=0)
    assert np.allclose(s.graph.poses, p, rtol=0, atol=1e-9) and np.allclose(s.edgeWeights(), w, rtol=1e-9, atol=1e-300)


LEVELWISE = {"CGMR_FWD_MERGE": "0", "CGMR_BWD_CHAIN": "0"}


def test_one_launch_per_level_gives_the_same_trace(ctx):
    runs = [("pg2500", dict(initial_delta=1.0)), ("pg9000", {}), ("lat80", dict(initial_delta=1.0)), ("hub100", {}),
            ("bad_start", {})]
    z = {}
    with context_under(LEVELWISE) as c:
        assert_launch_shape(c, LEVELWISE, C.args(graph(runs[0][0])))
        for name, kw in runs:
            rc, _, chi, dlt, tri, stp, done = c.dl_optimize(*C.args(graph(name)), ITERS, **kw)
            z.update({name + "_chi": chi, name + "_dlt": dlt, name + "_tri": tri, name + "_stp": stp, name + "_done": np.array([done, rc])})
    for name, kw in runs:
        g = graph(name)
        rc, _, chi, dlt, tri, stp, done = ctx.dl_optimize(*C.args(g), ITERS, **kw)
        # (the iterations the reference decides by more than rounding: after them the variants may part, as two GPUs may)
        k, whole = compared_iterations(ref_dogleg.dl_optimize(*C.args(g), ITERS, **kw), rounding_floor(g))
        if whole:
            assert z[name + "_done"].tolist() == [done, rc], name
        assert np.array_equal(z[name + "_tri"][:k], tri[:k]) and np.array_equal(z[name + "_stp"][:k], stp[:k]), name
        assert np.allclose(z[name + "_dlt"][:k], dlt[:k], rtol=VARIANT_RTOL, atol=0), name
        assert np.allclose(z[name + "_chi"][:k + 1], chi[:k + 1], rtol=VARIANT_RTOL, atol=1e3 * U * chi[0]), name


def test_a_timed_out_head_is_repeated_one_launch_per_level():
    """A bounded device-side wait that runs out in a head (forced: CGMR_BWD_SPIN_LIMIT=1, one poll per wait) is no verdict:
    the call goes on with one launch per kernel and level and gives the plain call's trace; the context counts the event
    and the next call runs the merged and chained launches again (on this context their waits run out again, and that call
    recovers the same way).  The switch belongs to the context: the plain call has a context of its own.  bad_start: trials
    are rejected and the plain call takes several rounds, so the repeated call passes through every part of the round loop."""
    from cg_mrslam_amd import Context
    name = "bad_start"
    g, iters = graph(name), CASES[name][1]
    ref = ref_dogleg.dl_optimize(*C.args(g), iters)
    c0 = Context(0)
    try:
        first = c0.dl_optimize(*C.args(g), iters)
        plain = c0.dl_last_stats()
        assert first[0] == 0 and c0.gn_timeouts() == 0
    finally:
        c0.close()
    assert plain["host_waits"] > 1 and any(t > 1 for t in first[4]), (name, plain, "the case rejects nothing")
    with context_under({"CGMR_BWD_SPIN_LIMIT": "1"}) as c:
        rc, _, chi, dlt, tri, stp, done = c.dl_optimize(*C.args(g), iters)
        print(name, "plain", plain, "forced", c.dl_last_stats(), "timeouts", c.gn_timeouts(), "trials", tri, first[4], "steps", stp, first[5])
        print(name, "chi", np.abs(chi - first[2]) / np.abs(first[2]), "delta", np.abs(dlt - first[3]) / np.maximum(first[3], 1e-300))
        assert rc == 0
        assert c.gn_timeouts() >= 1, "the forced time-out did not happen: the test checks nothing"
        assert done == first[6] and np.array_equal(tri, first[4]) and np.array_equal(stp, first[5]), (tri, first[4], stp, first[5])
        # (as test_one_launch_per_level_gives_the_same_trace compares the two variants)
        k, _ = compared_iterations(ref, rounding_floor(g))
        assert np.allclose(dlt[:k], first[3][:k], rtol=VARIANT_RTOL, atol=0)
        assert np.allclose(chi[:k + 1], first[2][:k + 1], rtol=VARIANT_RTOL, atol=1e3 * U * chi[0])
        assert check_trace(name, ref, chi, dlt, tri, stp, done, rounding_floor(g)) >= 1
        t1 = c.gn_timeouts()
        rc, _, chi, dlt, tri, stp, done = c.dl_optimize(*C.args(g), iters)
        assert rc == 0 and c.gn_timeouts() > t1
        assert done == first[6] and np.array_equal(tri, first[4]) and np.array_equal(stp, first[5]), (tri, first[4], stp, first[5])
        assert np.allclose(dlt[:k], first[3][:k], rtol=VARIANT_RTOL, atol=0)
        assert np.allclose(chi[:k + 1], first[2][:k + 1], rtol=VARIANT_RTOL, atol=1e3 * U * chi[0])


def test_robot_graph_dogleg_matches_reference():
    from cg_mrslam_amd import Context
    from robot_sequences import make_robot_rounds, solved_system
    from cg_mrslam_amd.mrslam import LoopbackExchange
    ctxs = [Context(0) for _ in range(2)]
    rounds = make_robot_rounds(ctxs, 1200, 4000, 44, 60)
    try:
        ex = LoopbackExchange([rr.g for rr in rounds])
        n_rounds, checked = 6, 0
        for t in range(n_rounds):
            for rr in rounds:
                rr.grow()
                g = rr.g
                if t == n_rounds - 1 and g.counts()["received_edges"] > 0:
                    sysm = solved_system(g)
                    p0 = g.poses()
                    g.set_algorithm("dl", initial_delta=1.0)
                    rc, chi = g.optimize(5)
                    g.set_algorithm("gn")
                    dlt, tri, stp = g.dl_last()
                    assert rc == 0
                    ref = ref_dogleg.dl_optimize(p0, sysm["fixed"], sysm["ef"], sysm["et"], sysm["meas"], sysm["info"], 5,
                                                 initial_delta=1.0)
                    full = [np.zeros(5), np.zeros(5, np.int32), np.zeros(5, np.int32)]
                    for f, v in zip(full, (dlt, tri, stp)):
                        f[:len(v)] = v
                    k = check_trace("robot %d" % g.robot, ref, chi, *full, len(dlt))
                    assert k >= 1
                    checked += 1
                else:
                    rc, _ = g.optimize(5)
                    assert rc == 0
            ex.finish_all()
            for rr in rounds:
                rr.condense()
            ex.start_all()
        ex.finish_all()
        assert checked >= 1
    finally:
        for rr in rounds:
            rr.g.close()
        for c in ctxs:
            c.close()
