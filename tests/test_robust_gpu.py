"""Robust kernels on the device (include/cgmr.h: cgmr_robust) against the float64 contract of tests/ref_robust.py."""
import numpy as np
import pytest

import ref_numpy as R
import ref_robust as RR
import reference_cases as C
from switch_contexts import assert_launch_shape, context_under
from test_reference_gpu import VARIANTS

pytestmark = pytest.mark.gpu

OMEGA_MAX = C.OMEGA_MAX
# robust chi2 per iteration against the reference: the GPU's and SciPy's iterates differ by the steps' forward errors (cond(H)
# times rounding), so the chi2 values agree to what the plain path's tests allow (test_lm_gpu.RTOL)
CHI_RTOL = 1e-9
STAT_RTOL = 1e-12         # e2 / weights at the same poses: one evaluation, rounding only
# e2 of an edge near its optimum is the square of a difference of poses: the device's and numpy's e carry cancellation errors
# of a few u times the pose magnitudes, whatever e2 is (measured: 2.3e-28 absolute at e2 ~ 1e-29 on chain3000, 9.4e-12 relative
# at e2 = 0.45 on the outlier graph).  e2 is checked to STAT_RTOL plus the error such a perturbation of e produces; the
# weights are checked to STAT_RTOL against rho1 of the device's own e2 (the kernel formulas, not the cancellation).
def e2_bound(poses, info, e2):
    d = 64 * R.U * (1.0 + float(np.abs(poses).max()))
    om = 3 * np.abs(np.asarray(info)).max(axis=1)
    return STAT_RTOL * np.abs(e2) + 2 * np.sqrt(np.abs(e2) * om) * d + om * d * d


def check_stats(poses, ef, et, meas, info, kind, delta, e2, w):
    ref = RR.edge_chi2(poses, ef, et, meas, info)
    bound = e2_bound(poses, info, ref)
    assert np.all(np.abs(e2 - ref) <= bound), float(np.max(np.abs(e2 - ref) / np.maximum(bound, 1e-300)))
    np.testing.assert_allclose(w, RR.rho(kind, delta, e2)[1], rtol=STAT_RTOL, atol=1e-300)


def check_chi2(chi, poses, ef, et, meas, info, kind, delta):
    """The robust chi2 the device reports at ``poses`` against numpy's, to CHI_RTOL plus the e2 bound summed over the edges."""
    r0 = RR.rho(kind, delta, RR.edge_chi2(poses, ef, et, meas, info))[0]
    tol = CHI_RTOL * abs(float(r0.sum())) + float(e2_bound(poses, info, RR.edge_chi2(poses, ef, et, meas, info)).sum())
    assert abs(chi - float(r0.sum())) <= tol, (chi, float(r0.sum()), tol)


KIND_DELTA = {"huber": (1, 1.0), "pseudohuber": (2, 1.0), "cauchy": (3, 3.0), "welsch": (4, 5.0), "tukey": (5, 8.0),
              "saturated": (6, 8.0), "dcs": (7, 5.0)}
REF_CASES = ("v5e4", "pg500", "pg2500", "hub40", "lat40", "fixed_dup_iso", "wrap")


@pytest.fixture(scope="module")
def ctx():
    from cg_mrslam_amd import Context
    c = Context(0)
    yield c
    c.close()


_OUTLIER = {}


def outlier():
    if not _OUTLIER:
        g, bad, closure = RR.outlier_graph()
        _OUTLIER.update(g=g, bad=bad, closure=closure, clean=RR.clean_optimum(g, bad))
    return _OUTLIER


def graph(name):
    return outlier()["g"] if name == "outlier" else C.CASES[name][0]()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(C.CASES))
def test_all_none_is_bit_identical_to_the_plain_calls(ctx, name):
    g = graph(name)
    a = C.args(g)
    nE = len(g["edge_from"])
    rc0, p0, chi0 = ctx.gn_optimize(*a, 3, raise_on_cholesky=False)
    for kind in ("none", np.zeros(nE, dtype=np.uint8)):
        rc, p, chi, e2, w = ctx.gn_optimize_robust(*a, 3, kind=kind, delta=1.0, raise_on_cholesky=False)
        assert rc == rc0 and np.array_equal(p, p0) and np.array_equal(chi, chi0), name
        check_stats(p, *C.args(g)[2:6], 0, 1.0, e2, w)
        assert np.all(w == 1.0)
    if name in ("c2", "pg2500", "wrap"):
        l0 = ctx.lm_optimize(*a, 3)
        l1 = ctx.lm_optimize_robust(*a, 3, kind="none")
        for u, v in zip(l0, l1[:6]):
            assert np.array_equal(u, v), name
        # device entry points
        import torch
        for lm in (False, True):
            dp, dm, di = _dev(g["poses"]), _dev(g["meas"]), _dev(g["info"])
            dk = _dev(np.zeros(nE, dtype=np.uint8))
            dd = _dev(np.ones(nE))
            args = (dp.data_ptr(), len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"], dm.data_ptr(), di.data_ptr(), 3)
            if lm:
                r = ctx.lm_optimize_robust_dev(*args, d_kind_ptr=dk.data_ptr(), d_delta_ptr=dd.data_ptr())
                assert np.array_equal(r[1], l0[2])
            else:
                r = ctx.gn_optimize_robust_dev(*args, d_kind_ptr=dk.data_ptr(), d_delta_ptr=dd.data_ptr())
                assert r[0] == rc0 and np.array_equal(r[1], chi0)
            torch.cuda.synchronize()
            assert np.array_equal(dp.cpu().numpy(), l0[1] if lm else p0)


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kname", sorted(KIND_DELTA))
@pytest.mark.parametrize("name", REF_CASES + ("outlier",))
def test_contract_per_kind(ctx, name, kname):
    kind, delta = KIND_DELTA[kname]
    g = graph(name)
    a = C.args(g)
    ef, et, meas, info = a[2:6]
    iters = 3
    p, ps = g["poses"], [g["poses"]]
    chis = []
    for it in range(iters):
        rc, p, chi, e2, w = ctx.gn_optimize_robust(p, *a[1:], 1, kind=kind, delta=delta, raise_on_cholesky=False)
        if rc != 0:
            # a zero weight can leave a vertex with no weighted edge: the reference's factorisation fails there too
            x, _, _, failed = RR.gn_optimize(ps[-1], g["fixed"], ef, et, meas, info, kind, delta, 1)
            assert failed == 0, (name, kname, it, rc)
            break
        chis.append(chi[0])
        ps.append(p)
    for i in range(len(ps) - 1):
        check_chi2(chis[i], ps[i], ef, et, meas, info, kind, delta)
        Ws = RR.scaled_info(ps[i], ef, et, meas, info, kind, delta)
        om = R.step_backward_error(ps[i], ps[i + 1], g["fixed"], ef, et, meas, Ws)
        assert om <= OMEGA_MAX, (name, kname, i, om / R.U)
    if len(ps) > 1:
        # the final statistics: at the estimate returned
        check_stats(ps[-1], ef, et, meas, info, kind, delta, e2, w)


# ------------------------------------------------------------------------------------------------------------------- 3
def test_outlier_recovery_through_graphslam(ctx):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    o = outlier()
    g, bad, clean = o["g"], o["bad"], o["clean"]
    plain = GraphSLAM(PoseGraph.from_synth(g), ctx=ctx)
    plain.optimize(10)
    assert plain.last_status == 0 and plain.edgeWeights() is None
    assert RR.rms(plain.graph.poses, clean) > 2.0
    gs = GraphSLAM(PoseGraph.from_synth(g), ctx=ctx)
    gs.setRobustKernel("Cauchy", 3.0)
    gs.optimize(10)
    assert gs.last_status == 0
    err = RR.rms(gs.graph.poses, clean)
    w = gs.edgeWeights()
    good = np.ones(len(w), dtype=bool)
    good[bad] = False
    print(f"outlier graph: plain {RR.rms(plain.graph.poses, clean):.3f} m, Cauchy(3) {err:.4f} m, corrupted w <= "
          f"{w[bad].max():.3g}, clean w > 0.5: {(w[good] > 0.5).mean():.4f}")
    assert err < 0.2
    assert w[bad].max() < 1e-3
    assert (w[good] > 0.5).mean() >= 0.95
    # chi2() stays plain, robustChi2() is the robust one
    ef, et, meas, info = gs.graph.level0()
    np.testing.assert_allclose(gs.chi2(), R.chi2(gs.graph.poses, ef, et, meas, info), rtol=1e-9)
    np.testing.assert_allclose(gs.robustChi2(), RR.robust_chi2(gs.graph.poses, ef, et, meas, info, 3, 3.0), rtol=1e-9)
    # and with Levenberg-Marquardt
    lm = GraphSLAM(PoseGraph.from_synth(g), ctx=ctx, algorithm="levenberg")
    lm.setRobustKernel("Cauchy", 3.0)
    lm.optimize(10)
    assert lm.last_status == 0 and lm.edgeWeights() is not None


# ------------------------------------------------------------------------------------------------------------------- 4
def test_mixed_settings_and_device_variants(ctx):
    import torch
    o = outlier()
    g, closure = o["g"], o["closure"]
    a = C.args(g)
    nE = len(g["edge_from"])
    kind = np.where(closure, 1, 0).astype(np.uint8)
    delta = np.where(closure, 0.5 + (np.arange(nE) % 7) * 0.25, 1.0)
    rc, p, chi, e2, w = ctx.gn_optimize_robust(*a, 4, kind=kind, delta=delta)
    assert rc == 0
    check_chi2(chi[0], g["poses"], *a[2:6], kind, delta)
    check_chi2(chi[-1], p, *a[2:6], kind, delta)
    assert np.all(w[~closure] == 1.0)
    check_stats(p, *a[2:6], kind, delta, e2, w)
    lm = ctx.lm_optimize_robust(*a, 4, kind=kind, delta=delta)
    for lmode in (False, True):
        dp, dm, di, dk, dd = _dev(g["poses"]), _dev(g["meas"]), _dev(g["info"]), _dev(kind), _dev(delta)
        args = (dp.data_ptr(), len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"], dm.data_ptr(), di.data_ptr(), 4)
        if lmode:
            r = ctx.lm_optimize_robust_dev(*args, d_kind_ptr=dk.data_ptr(), d_delta_ptr=dd.data_ptr())
            for u, v in zip(r, (lm[0],) + tuple(lm[2:])):
                assert np.array_equal(u, v)
        else:
            r = ctx.gn_optimize_robust_dev(*args, d_kind_ptr=dk.data_ptr(), d_delta_ptr=dd.data_ptr())
            for u, v in zip(r, (rc, chi, e2, w)):
                assert np.array_equal(u, v)
        torch.cuda.synchronize()
        assert np.array_equal(dp.cpu().numpy(), lm[1] if lmode else p)
    # a bad device delta is caught before anything runs
    from cg_mrslam_amd._lib import CgmrError
    dd = _dev(np.where(closure, -1.0, 1.0))
    dp, dm, di, dk = _dev(g["poses"]), _dev(g["meas"]), _dev(g["info"]), _dev(kind)
    with pytest.raises(CgmrError):
        ctx.gn_optimize_robust_dev(dp.data_ptr(), len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"], dm.data_ptr(),
                                   di.data_ptr(), 2, d_kind_ptr=dk.data_ptr(), d_delta_ptr=dd.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy(), g["poses"])


# ------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name,kname", [("pg500", "huber"), ("pg2500", "cauchy"), ("wrap", "tukey"), ("outlier", "cauchy"),
                                        ("outlier", "dcs")])
def test_levenberg_matches_reference(ctx, name, kname):
    kind, delta = KIND_DELTA[kname]
    g = graph(name)
    a = C.args(g)
    rc, p, chi, lam, tri, done, e2, w = ctx.lm_optimize_robust(*a, 6, kind=kind, delta=delta)
    ref = RR.lm_optimize(*a, kind, delta, 6)
    assert rc == 0 and done == ref["iters_done"], (name, done, ref["iters_done"])
    assert np.array_equal(tri[:done], ref["trials"])
    np.testing.assert_allclose(lam[:done], ref["lambdas"], rtol=1e-6)
    np.testing.assert_allclose(chi, ref["chi2"], rtol=CHI_RTOL)
    check_stats(p, *a[2:6], kind, delta, e2, w)


def test_levenberg_rejected_trial_restores_the_poses(ctx):
    g = graph("pg500")
    a = C.args(g)
    # a huge initial step scale: lambda tiny, the first trial from a poor start is rejected under Tukey
    p_bad = g["poses"] + np.random.default_rng(3).normal(0, 0.5, g["poses"].shape) * (g["fixed"] == 0)[:, None]
    ref = RR.lm_optimize(p_bad, *a[1:], 5, 2.0, 1, max_trials=1)
    rc, p, chi, lam, tri, done, e2, w = ctx.lm_optimize_robust(p_bad, *a[1:], 1, kind="tukey", delta=2.0, max_trials=1)
    assert rc == 0 and done == ref["iters_done"]
    if not ref["trace"][0]["accept"]:
        assert np.array_equal(p, p_bad)
    # the statistics are those of the committed poses
    check_stats(p, *a[2:6], 5, 2.0, e2, w)


# ------------------------------------------------------------------------------------------------------------------- 6
def test_zero_weights_fail_cleanly(ctx):
    """Vertex 2 hangs on one edge far beyond Tukey's delta: its weight is 0, its block of H singular."""
    poses = np.array([[0.0, 0, 0], [1.0, 0, 0], [50.0, 0, 0]])
    fixed = np.array([1, 0, 0], dtype=np.uint8)
    ef, et = np.array([0, 1], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    meas = np.array([[1.0, 0, 0], [1.0, 0, 0]])
    info = np.tile([1.0, 0, 0, 1.0, 0, 1.0], (2, 1))
    rc, p, chi, e2, w = ctx.gn_optimize_robust(poses, fixed, ef, et, meas, info, 3, kind="tukey", delta=2.0,
                                               raise_on_cholesky=False)
    assert rc == -100                                            # CGMR_E_CHOLESKY_BASE - 0
    assert np.all(np.isfinite(p)) and np.array_equal(p, poses)
    assert w[1] == 0.0 and w[0] == 1.0
    rc, p, chi, lam, tri, done, e2, w = ctx.lm_optimize_robust(poses, fixed, ef, et, meas, info, 3, kind="tukey", delta=2.0)
    assert rc == 0 and np.all(np.isfinite(p)) and np.all(np.isfinite(chi))


# ------------------------------------------------------------------------------------------------------------------- 7
def test_robot_graph_robust_round():
    from cg_mrslam_amd import Context
    from cg_mrslam_amd.mrslam import LoopbackExchange
    from robot_sequences import debug_edges, make_robot_rounds, solved_system
    ctxs = [Context(0) for _ in range(2)]
    rounds = make_robot_rounds(ctxs, 1200, 4000, 44, 60)
    try:
        ex = LoopbackExchange([rr.g for rr in rounds])
        n_rounds, checked = 5, 0
        for t in range(n_rounds):
            for rr in rounds:
                rr.grow()
                g = rr.g
                if t == n_rounds - 1 and g.counts()["received_edges"] > 0:
                    # one corrupted own closure, Huber on every own closure and on the received edges
                    _, oef, oet, _, _ = g.own_system()
                    id_of = {v: k for k, v in g.index.items()}
                    g.add_edges([id_of[int(oef[3])]], [id_of[int(oet[len(oet) // 2])]], np.array([[7.0, -4.0, 2.0]]),
                                np.array([[100.0, 0, 0, 100.0, 0, 1000.0]]))
                    fixed, oef, oet, _, _ = g.own_system()
                    closure = np.abs(oet.astype(np.int64) - oef.astype(np.int64)) != 1
                    kind = np.where(closure, 1, 0).astype(np.uint8)
                    g.set_edge_robust(kind, 1.0)
                    g.set_received_robust("huber", 2.0)
                    sysm = solved_system(g)
                    nA = sysm["n_own"]
                    kk = np.concatenate([kind, np.full(len(sysm["ef"]) - nA, 1)])
                    dd = np.concatenate([np.ones(nA), np.full(len(sysm["ef"]) - nA, 2.0)])
                    p = g.poses()
                    for it in range(3):
                        rc, chi = g.optimize(1)
                        assert rc == 0
                        p1 = g.poses()
                        ws = RR.scaled_info(p, sysm["ef"], sysm["et"], sysm["meas"], sysm["info"], kk, dd)
                        om = R.step_backward_error(p, p1, sysm["fixed"], sysm["ef"], sysm["et"], sysm["meas"], ws)
                        assert om <= OMEGA_MAX, (it, om / R.U)
                        check_chi2(chi[0], p, sysm["ef"], sysm["et"], sysm["meas"], sysm["info"], kk, dd)
                        p = p1
                    e2, w = g.edge_stats()
                    ef, et, n_own = debug_edges(g)
                    assert len(e2) == len(ef) and n_own == nA
                    check_stats(p, ef, et, sysm["meas"], sysm["info"], kk, dd, e2, w)
                    assert w[nA - 1] < 0.05                             # the corrupted closure
                    # the condensed graphs do not see the kernels
                    got = {}
                    for peer in range(g.n_robots):
                        if peer != g.robot and g.computeCondensedGraph(peer) > 0:
                            got[peer] = [np.array(v).tobytes() for v in g.condensed(peer)]
                    g.set_edge_robust(np.zeros(nA, np.uint8), 1.0)
                    g.set_received_robust("none")
                    for peer, want in got.items():
                        assert g.computeCondensedGraph(peer) > 0
                        assert [np.array(v).tobytes() for v in g.condensed(peer)] == want
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


# ------------------------------------------------------------------------------------------------------------------- 8
def test_launch_variants_backward_error():
    g = outlier()["g"]
    a = C.args(g)
    ef, et, meas, info = a[2:6]
    for vname, env in VARIANTS:
        with context_under(env) as c:
            assert_launch_shape(c, env, a)
            ps = [g["poses"]]
            for it in range(3):
                rc, p, _, _, _ = c.gn_optimize_robust(ps[-1], *a[1:], 1, kind="huber", delta=1.0)
                assert rc == 0, (vname, it, rc)
                ps.append(p)
            assert c.gn_timeouts() == 0, vname
        for i in range(len(ps) - 1):
            ws = RR.scaled_info(ps[i], ef, et, meas, info, 1, 1.0)
            om = R.step_backward_error(ps[i], ps[i + 1], g["fixed"], ef, et, meas, ws)
            assert om <= OMEGA_MAX, (vname, i, om / R.U)
