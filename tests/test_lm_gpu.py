"""Levenberg-Marquardt on the device (cgmr_lm_optimize, Context.lm_optimize, GraphSLAM(algorithm="levenberg"),
RobotGraph.set_algorithm) against the float64 reference of the contract, tests/ref_lm.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import ref_lm
import ref_numpy as R
import reference_cases as C
from switch_contexts import assert_launch_shape, context_under
from test_lm_cpu import EXTRA_CASES

pytestmark = pytest.mark.gpu

U = np.finfo(np.float64).eps / 2
ITERS = 5
RTOL = 1e-9


def _cases():
    out = {name: (builder, ITERS) for name, (builder, _) in C.CASES.items()}
    out.update(EXTRA_CASES)
    return out


CASES = _cases()
_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = CASES[name][0]()
    return _GRAPHS[name]


def rounding_floor(g):
    """A chi2 made of rounded residuals only: nE max(Omega) (1e3 u max |x|)^2 (chain3000 starts at its optimum, 2e-24)."""
    return len(g["edge_from"]) * float(np.max(np.abs(g["info"]))) * (1e3 * U * (float(np.max(np.abs(g["poses"]))) + 1.0)) ** 2


def compared_iterations(ref, floor=0.0):
    """Iterations of the reference whose trials are all decided by more than rounding: up to (excluding) the first with a
    trial where |currentChi - tempChi| <= 1e3 u currentChi, or currentChi <= floor (rho is rounding there, and everything
    after it may differ)."""
    for t in ref["trace"]:
        if not t["failed"] and (abs(t["current"] - t["temp"]) <= 1e3 * U * abs(t["current"]) or abs(t["current"]) <= floor):
            return t["iteration"], False
    return ref["iters_done"], True


CHI_AGREE = 1e-12   # relative agreement assumed of the two chi2 sums at the same poses (summation order, rounded steps)


def lambda_rtol(ref, k):
    """RTOL, widened by what rho's rounding does to lambda: an accepted trial scales lambda by 1 - (2 rho - 1)^3 inside
    [1/3, 2/3], whose relative change is at most 18 times rho's, and rho's relative error is about
    CHI_AGREE currentChi / |currentChi - tempChi| -- near the optimum that exceeds 1e-9 long before the 1e3 u exemption."""
    tol = np.full(k, RTOL)
    acc = 0.0
    for t in ref["trace"]:
        if t["iteration"] >= k:
            break
        if t["accept"]:
            acc += 18 * CHI_AGREE * abs(t["current"]) / abs(t["current"] - t["temp"])
        tol[t["iteration"]] = RTOL + acc
    return tol


def check_trace(name, ref, chi, lam, tri, done, floor=0.0):
    k, whole = compared_iterations(ref, floor)
    assert np.array_equal(tri[:k], ref["trials"][:k]), (name, tri[:k], ref["trials"][:k])
    rel = np.abs(lam[:k] - ref["lambdas"][:k]) / np.abs(ref["lambdas"][:k])
    assert np.all(rel <= lambda_rtol(ref, k)), (name, rel, lambda_rtol(ref, k))
    if abs(ref["chi2"][0]) > floor:
        assert np.allclose(chi[:k + 1], ref["chi2"][:k + 1], rtol=RTOL, atol=0), (name, chi[:k + 1], ref["chi2"][:k + 1])
    if whole:
        assert done == ref["iters_done"], (name, done, ref["iters_done"])
        assert np.array_equal(tri[:done], ref["trials"]) and np.all(tri[done:] == 0) and np.all(lam[done:] == 0)
        assert np.allclose(chi, ref["chi2"], rtol=RTOL, atol=0)
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
    ref = ref_lm.lm_optimize(*C.args(g), iters)
    rc, poses, chi, lam, tri, done = ctx.lm_optimize(*C.args(g), iters)
    assert rc == 0
    k = check_trace(name, ref, chi, lam, tri, done, rounding_floor(g))
    # (v2e1, v5e4 and chain3000 start at their optimum to rounding: nothing there is decided by more than rounding)
    assert k >= 1 or name in ("v2e1", "v5e4", "chain3000"), (name, "nothing compared")
    fx = R.active_fixed(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    assert np.array_equal(poses[fx != 0], g["poses"][fx != 0])          # fixed and inactive vertices: untouched
    if name == "bad_start":
        assert np.all(np.diff(chi) <= 0) and any(t > 1 for t in tri)
    if name == "indefinite":
        assert any(t["failed"] for t in ref["trace"]) and tri[0] == 4


@pytest.mark.parametrize("name", ["v5e4", "chain3000", "pg500", "pg2500", "hub40", "lat40", "fixed_dup_iso", "wrap", "c2",
                                  "bad_start", "indefinite", "no_fixed"])
def test_accepted_steps_are_backward_stable_solves_of_the_damped_system(ctx, name):
    """Chained one-iteration calls, each started at the lambda the previous one ended with (initial_lambda): the same
    iterations as one call, bit for bit, and every accepted step solves (H + lambda I) dx = b within OMEGA_MAX, lambda
    = the start value times nu's growth over the rejected trials (2, 4, 8, ...: exact)."""
    g = graph(name)
    p, fixed, ef, et, meas, info = C.args(g)
    fx = R.active_fixed(len(p), fixed, ef, et)
    H0, _, _ = R.build_system(p, fx, ef, et, meas, info)
    lam0 = 1e-5 * float(np.max(np.abs(H0.diagonal())))
    x, lam, n_run = p.copy(), lam0, 0
    for it in range(3):
        rc, x1, chi, lo, tri, done = ctx.lm_optimize(x, fixed, ef, et, meas, info, 1, initial_lambda=lam)
        assert rc == 0 and done == 1
        if np.array_equal(x1, x):                            # no trial accepted (the trial limit): nothing to check
            break
        r = int(tri[0]) - 1                                  # rejected trials before the accepted one
        used = lam * 2.0 ** (r * (r + 1) // 2)
        H, b, _ = R.build_system(x, fx, ef, et, meas, info)
        Hd = H + used * sp.identity(H.shape[0], format="csc")
        om = R.step_backward_error(x, x1, fixed, ef, et, meas, info, H=Hd, b=b)
        assert om <= C.OMEGA_MAX, (name, it, om / U)
        x, lam, n_run = x1, float(lo[0]), it + 1
    assert n_run >= 1
    rc, xs, _, lams, _, done = ctx.lm_optimize(p, fixed, ef, et, meas, info, n_run, initial_lambda=lam0)
    assert np.array_equal(xs, x) and lams[n_run - 1] == lam


def test_rejected_trials_leave_the_poses_bit_identical(ctx):
    # a failed factorisation twice, then the trial limit: the call terminates with the poses as they came
    g = graph("indefinite")
    rc, poses, chi, lam, tri, done = ctx.lm_optimize(*C.args(g), 3, max_trials=2)
    assert rc == 0 and done == 1 and tri.tolist() == [2, 0, 0]
    assert np.array_equal(poses, g["poses"]) and np.all(chi == chi[0])
    # a rejected step that was solved and applied (rho < 0): the first iteration of bad_start whose first trial is rejected
    g = graph("bad_start")
    ref = ref_lm.lm_optimize(*C.args(g), 10)
    k = next(t["iteration"] for t in ref["trace"] if t["trial"] == 1)
    assert not ref["trace"][[t["iteration"] for t in ref["trace"]].index(k)]["failed"]
    p, fixed, ef, et, meas, info = C.args(g)
    fx = R.active_fixed(len(p), fixed, ef, et)
    lam_k = 1e-5 * float(np.max(np.abs(R.build_system(p, fx, ef, et, meas, info)[0].diagonal())))
    xk = p
    if k:
        _, xk, _, lams, _, _ = ctx.lm_optimize(p, fixed, ef, et, meas, info, k, initial_lambda=lam_k)
        lam_k = float(lams[k - 1])
    rc, x1, chi, lam, tri, done = ctx.lm_optimize(xk, fixed, ef, et, meas, info, 1, initial_lambda=lam_k, max_trials=1)
    assert rc == 0 and done == 1 and tri.tolist() == [1] and lam[0] == 2 * lam_k
    assert np.array_equal(x1, xk) and chi[1] == chi[0]


def test_repeats_are_bit_identical(ctx):
    for name in ("pg2500", "bad_start", "indefinite"):
        g, iters = graph(name), CASES[name][1]
        a = ctx.lm_optimize(*C.args(g), iters)
        b = ctx.lm_optimize(*C.args(g), iters)
        for u, v in zip(a, b):
            assert np.array_equal(np.asarray(u), np.asarray(v)), name


def test_symbolic_cache_hit_after_gauss_newton(ctx):
    g = graph("pg500")
    ctx.gn_optimize(*C.args(g), 2)
    s0 = ctx.symbolic_cache_stats()
    rc, *_ = ctx.lm_optimize(*C.args(g), 3)
    s1 = ctx.symbolic_cache_stats()
    assert rc == 0 and s1["hits"] == s0["hits"] + 1 and s1["misses"] == s0["misses"] and s1["extended"] == s0["extended"]
    st = ctx.lm_last_stats()
    assert st["trials"] >= 3 and st["host_waits"] >= 1


def test_one_wait_when_every_first_trial_is_accepted(ctx):
    g = graph("c2")
    rc, _, _, _, tri, done = ctx.lm_optimize(*C.args(g), 4)
    assert rc == 0 and done == 4 and np.all(tri == 1)
    assert ctx.lm_last_stats() == dict(host_waits=1, trials=4)


def test_graph_slam_levenberg(ctx):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = graph("bad_start")
    pg = PoseGraph.from_synth(g)
    s = GraphSLAM(pg, ctx, algorithm="levenberg")
    s.optimize(10)
    ref = ref_lm.lm_optimize(*C.args(g), 10)
    assert s.last_status == 0 and s.last_iterations == ref["iters_done"]
    assert s.currentLambda() == pytest.approx(ref["lambdas"][-1], rel=RTOL)
    assert s.levenbergIterations() == ref["trials"][-1]
    assert np.allclose(s.last_chi2, ref["chi2"], rtol=RTOL, atol=0)


LEVELWISE = {"CGMR_FWD_MERGE": "0", "CGMR_BWD_CHAIN": "0"}


def test_one_launch_per_level_gives_the_same_trace(ctx):
    names = ["pg2500", "pg9000", "lat80", "hub100", "bad_start"]
    z = {}
    with context_under(LEVELWISE) as c:
        assert_launch_shape(c, LEVELWISE, C.args(graph(names[0])))
        for name in names:
            z[name] = c.lm_optimize(*C.args(graph(name)), CASES[name][1])
    for name in names:
        g, iters = graph(name), CASES[name][1]
        rc, _, chi, lam, tri, done = ctx.lm_optimize(*C.args(g), iters)
        z_rc, _, z_chi, z_lam, z_tri, z_done = z[name]
        assert [z_done, z_rc] == [done, rc] and np.array_equal(z_tri, tri), name
        assert np.allclose(z_lam, lam, rtol=RTOL, atol=0) and np.allclose(z_chi, chi, rtol=RTOL, atol=0), name


def test_a_timed_out_trial_is_repeated_one_launch_per_level():
    """A bounded device-side wait that runs out in a trial (forced: CGMR_BWD_SPIN_LIMIT=1, one poll per wait) is no verdict:
    the call goes on with one launch per kernel and level and gives the plain call's trace; the context counts the event
    and the next call runs the merged and chained launches again (on this context their waits run out again, and that call
    recovers the same way).  The switch belongs to the context: the plain call has a context of its own.  bad_start: trials
    are rejected and the plain call takes several rounds, so the repeated call passes through every part of the round loop."""
    from cg_mrslam_amd import Context
    name = "bad_start"
    g, iters = graph(name), CASES[name][1]
    ref = ref_lm.lm_optimize(*C.args(g), iters)
    c0 = Context(0)
    try:
        first = c0.lm_optimize(*C.args(g), iters)
        plain = c0.lm_last_stats()
        assert first[0] == 0 and c0.gn_timeouts() == 0
    finally:
        c0.close()
    assert plain["host_waits"] > 1 and any(t > 1 for t in first[4]), (name, plain, "the case rejects nothing")
    with context_under({"CGMR_BWD_SPIN_LIMIT": "1"}) as c:
        rc, _, chi, lam, tri, done = c.lm_optimize(*C.args(g), iters)
        print(name, "plain", plain, "forced", c.lm_last_stats(), "timeouts", c.gn_timeouts(), "trials", tri, first[4])
        print(name, "chi", np.abs(chi - first[2]) / np.abs(first[2]), "lambda", np.abs(lam - first[3]) / np.maximum(first[3], 1e-300))
        assert rc == 0
        assert c.gn_timeouts() >= 1, "the forced time-out did not happen: the test checks nothing"
        assert done == first[5] and np.array_equal(tri, first[4]), (tri, first[4])
        assert np.allclose(lam, first[3], rtol=RTOL, atol=0) and np.allclose(chi, first[2], rtol=RTOL, atol=0)
        assert check_trace(name, ref, chi, lam, tri, done, rounding_floor(g)) >= 1
        t1 = c.gn_timeouts()
        rc, _, chi, lam, tri, done = c.lm_optimize(*C.args(g), iters)
        assert rc == 0 and c.gn_timeouts() > t1
        assert done == first[5] and np.array_equal(tri, first[4]), (tri, first[4])
        assert np.allclose(lam, first[3], rtol=RTOL, atol=0) and np.allclose(chi, first[2], rtol=RTOL, atol=0)


def test_robot_graph_levenberg_matches_reference():
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
                    g.set_algorithm("levenberg")
                    rc, chi = g.optimize(5)
                    g.set_algorithm("gn")
                    lam, tri = g.lm_last()
                    assert rc == 0
                    ref = ref_lm.lm_optimize(p0, sysm["fixed"], sysm["ef"], sysm["et"], sysm["meas"], sysm["info"], 5)
                    lam_full, tri_full = np.zeros(5), np.zeros(5, np.int32)
                    lam_full[:len(lam)], tri_full[:len(tri)] = lam, tri
                    check_trace("robot %d" % g.robot, ref, chi, lam_full, tri_full, len(lam))
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
