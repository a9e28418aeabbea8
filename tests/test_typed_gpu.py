"""Typed factors on the GPU (cgmr_*_typed): point landmarks (EDGE_SE2_XY), pose priors (EDGE_PRIOR_SE2) and position priors
(EDGE_PRIOR_SE2_XY) against the true-dimension float64 reference (tests/ref_typed.py) on the cases of tests/typed_cases.py.
The bars are those of the untyped tests: reference_cases.OMEGA_MAX for a step's backward error, tests/test_gn_gpu.py's CHI_RTOL
for chi2, the trace checks of tests/test_lm_gpu.py / tests/test_dogleg_gpu.py, tests/test_robust_gpu.py's statistics bounds,
tests/test_reference_gpu.py's MARG_TAU."""
import numpy as np
import pytest

import ref_numpy as R
import ref_typed as T
import reference_cases as C
import typed_cases as TC
from cg_mrslam_amd._lib import CgmrError

pytestmark = pytest.mark.gpu


def _a(g):
    return TC.args(g)


def _kw(g):
    return dict(vertex_kind=g["vk"], edge_kind=g["ek"])


def test_all_zero_kinds_are_the_plain_call_bit_for_bit(ctx):
    g = C.CASES["pg500"][0]()
    a = C.args(g)
    z = dict(vertex_kind=np.zeros(len(g["poses"]), np.uint8), edge_kind=np.zeros(len(g["edge_from"]), np.uint8))
    for plain, typed in ((ctx.gn_optimize(*a, 5), ctx.gn_optimize_typed(*a, 5, **z)),
                         (ctx.gn_optimize(*a, 5), ctx.gn_optimize_typed(*a, 5)),
                         (ctx.lm_optimize(*a, 5), ctx.lm_optimize_typed(*a, 5, **z)),
                         (ctx.dl_optimize(*a, 5), ctx.dl_optimize_typed(*a, 5, **z))):
        assert len(plain) == len(typed)
        for u, v in zip(plain, typed):
            assert np.array_equal(np.asarray(u), np.asarray(v))
    fx = g["fixed"]
    assert np.array_equal(ctx.marginals(g["poses"], fx, *a[2:], [3, 77]), ctx.marginals_typed(g["poses"], fx, *a[2:], [3, 77], **z))


def test_known_answer_landmark(ctx):
    g = TC.landmark_answer()
    rc, p, chi = ctx.gn_optimize_typed(*_a(g), 1, **_kw(g))
    assert rc == 0
    assert np.abs(p[1, :2] - g["answer"]).max() <= 1e-12 and p[1, 2] == 0.0
    assert np.array_equal(p[0], g["poses"][0])
    assert chi[1] <= 1e-20 and chi[0] == pytest.approx(T.chi2(g["poses"], *_a(g)[2:], g["ek"]), rel=1e-12)


@pytest.mark.parametrize("wrap", [False, True])
def test_known_answer_prior(ctx, wrap):
    g = TC.prior_answer(wrap)
    rc, p, chi = ctx.gn_optimize_typed(*_a(g), 1, **_kw(g))
    assert rc == 0
    assert np.abs(p[0, :2] - g["answer"][:2]).max() <= 1e-12
    assert abs(float(R.normalize_theta(p[0, 2] - g["answer"][2]))) <= 1e-12
    assert chi[0] == pytest.approx(T.chi2(g["poses"], *_a(g)[2:], g["ek"]), rel=1e-12) and chi[1] <= 1e-20


def _launches(c, g):
    c.set_profiling(True)
    try:
        rc, _, _ = c.gn_optimize_typed(*_a(g), 1, **_kw(g))
        assert rc == 0
        t = c.gn_kernel_times()
    finally:
        c.set_profiling(False)
    return {k: v[1] for k, v in t.items()}


@pytest.mark.parametrize("name", list(TC.CASES))
def test_gn_against_reference(ctx, name):
    """chi2 before each of 10 iterations against the reference's; one step from the initial guess and one from the GPU's own
    3rd iterate within the backward-error bar; a point's third component stays 0.0; fixed and untouched vertices keep their bits."""
    _, why, reach = TC.CASES[name]
    g = TC.case(name)
    assert reach(g), why
    vk, ek = TC.kinds(g)
    a = _a(g)
    if name == "tree600":
        from cg_mrslam_amd._lib import gn_symbolic_info
        n = _launches(ctx, g)
        info = gn_symbolic_info(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
        assert n["front_level"] > 0 and n["solve_bwd"] < info["launch_levels"]      # merged levels, a chained backward solve
    rc, p10, chi = ctx.gn_optimize_typed(*a, 10, **_kw(g))
    assert rc == 0
    _, chi_ref, _ = T.gn_optimize(*a, 10, vk, ek)
    rel = np.abs(chi - chi_ref) / np.maximum(np.abs(chi_ref), 1e-300)
    print(f"{name}: chi2 {chi[0]:.6g} -> {chi[-1]:.6g}, largest relative difference to the reference {rel.max():.2e}")
    np.testing.assert_allclose(chi, chi_ref, rtol=TC.CHI_RTOL, atol=1e-18)
    fx = T.active_fixed(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    worst = 0.0
    for start in (0, 3):
        p0 = g["poses"]
        if start:
            rc, p0, _ = ctx.gn_optimize_typed(*a, start, **_kw(g))
            assert rc == 0
        rc, p1, _ = ctx.gn_optimize_typed(p0, *a[1:], 1, **_kw(g))
        assert rc == 0
        for p in (p0, p1):
            assert np.all(p[vk == 1, 2] == 0.0)
            assert np.array_equal(p[fx != 0], g["poses"][fx != 0])
        w = T.step_backward_error(p0, p1, *a[1:], vk, ek)
        worst = max(worst, w)
        assert w <= TC.OMEGA_MAX, (name, start, w / T.U)
    print(f"{name}: largest omega {worst / T.U:.1f} u")
    assert np.all(p10[vk == 1, 2] == 0.0) and np.array_equal(p10[fx != 0], g["poses"][fx != 0])
    if name == "leaf_and_hub":
        assert p10[g["lone"]].tobytes() == g["poses"][g["lone"]].tobytes()
        assert p10[g["fixed_point"]].tobytes() == g["poses"][g["fixed_point"]].tobytes()
    if name == "prior_only_vertex":
        v = g["alone"]
        assert np.abs(p10[v] - g["truth"][v]).max() < 0.1 and np.abs(p10[v] - g["poses"][v]).max() > 0


def test_without_its_prior_the_gauge_case_fails_to_factor(ctx):
    g = TC.case("prior_gauge")
    keep = g["ek"] != 3
    a = (g["poses"], g["fixed"], g["edge_from"][keep], g["edge_to"][keep], g["meas"][keep], g["info"][keep])
    rc, p, _ = ctx.gn_optimize_typed(*a, 1, vertex_kind=g["vk"], edge_kind=g["ek"][keep], raise_on_cholesky=False)
    assert rc == -100                                            # CGMR_E_CHOLESKY_BASE - 0: no fixed vertex, nothing holds the gauge
    assert np.array_equal(p, g["poses"])
    rc, _, _ = ctx.gn_optimize_typed(*_a(g), 1, **_kw(g), raise_on_cholesky=False)
    assert rc == 0


@pytest.mark.parametrize("name", ["mixed257", "prior_gauge"])
def test_lm_trace_matches_reference(ctx, name):
    """Trials, termination, lambda and chi2 at the bars of tests/test_lm_gpu.py (check_trace).  lambda's trace at 1e-9 from the
    first iteration on holds the initial lambda tau * max |H_jj| to the true-dimension system's: the dummy pivots do not enter."""
    import test_lm_gpu as LM
    g = TC.case(name)
    vk, ek = TC.kinds(g)
    ref = T.lm_optimize(*_a(g), LM.ITERS, vk, ek)
    rc, poses, chi, lam, tri, done = ctx.lm_optimize_typed(*_a(g), LM.ITERS, **_kw(g))
    assert rc == 0
    k = LM.check_trace(name, ref, chi, lam, tri, done, LM.rounding_floor(g))
    assert k >= 1, "nothing compared"
    assert np.all(poses[vk == 1, 2] == 0.0)
    # the first trial alone, lambda given: the same trial as with lambda = tau max |H_jj| of the reference's H
    lam0 = ref["trace"][0]["lambda"]
    fx = T.active_fixed(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    H, _, _ = T.build_system(g["poses"], fx, *_a(g)[2:], vk, ek)
    assert lam0 == 1e-5 * H.diagonal().max()
    one = ctx.lm_optimize_typed(*_a(g), 1, **_kw(g))
    given = ctx.lm_optimize_typed(*_a(g), 1, **_kw(g), initial_lambda=lam0)
    assert one[5] == given[5] == 1 and np.array_equal(one[4], given[4])
    np.testing.assert_allclose(one[3], given[3], rtol=LM.RTOL)
    np.testing.assert_allclose(one[2], given[2], rtol=LM.RTOL)


@pytest.mark.parametrize("name", ["mixed257", "prior_gauge"])
def test_dogleg_trace_matches_reference(ctx, name):
    """Trials, step kinds, termination, delta and chi2 at the bars of tests/test_dogleg_gpu.py (check_trace)."""
    import test_dogleg_gpu as DL
    g = TC.case(name)
    vk, ek = TC.kinds(g)
    for params in ({}, dict(initial_delta=0.5)):
        ref = T.dl_optimize(*_a(g), DL.ITERS, vk, ek, **params)
        rc, poses, chi, dlt, tri, stp, done = ctx.dl_optimize_typed(*_a(g), DL.ITERS, **_kw(g), **params)
        assert rc == 0
        k = DL.check_trace(name, ref, chi, dlt, tri, stp, done, DL.rounding_floor(g))
        assert k >= 1, "nothing compared"
        assert np.all(poses[vk == 1, 2] == 0.0)


def test_robust_cauchy_on_corrupted_landmark_observations(ctx):
    """Cauchy on mixed257 with three corrupted landmark observations: e2 / weights / robust chi2 at the bars of
    tests/test_robust_gpu.py, the weight from e^T Omega e of the factor's own dimension."""
    import test_robust_gpu as RG
    g = dict(TC.case("mixed257"))
    vk, ek = TC.kinds(g)
    meas = g["meas"].copy()
    bad = np.flatnonzero(ek == 1)[[4, 40, 90]]
    meas[bad, :2] += np.array([[2.0, -1.5], [-1.0, 2.5], [3.0, 1.0]])
    a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], meas, g["info"])
    kind, delta = 3, 3.0
    # statistics and chi2 at the starting point (no iteration), then after five iterations
    for iters in (0, 5):
        rc, p, chi, e2, w = ctx.gn_optimize_typed(*a, iters, **_kw(g), kind="cauchy", delta=delta)
        assert rc == 0
        ref_e2 = T.edge_chi2(p, *a[2:], ek)
        info3 = np.abs(T.info_typed(g["info"], ek)).reshape(len(ek), 9)[:, [0, 1, 2, 4, 5, 8]]
        bound = RG.e2_bound(p, info3, ref_e2)
        assert np.all(np.abs(e2 - ref_e2) <= bound)
        np.testing.assert_allclose(w, T.ref_robust.rho(kind, delta, e2)[1], rtol=RG.STAT_RTOL, atol=1e-300)
        r0 = float(T.ref_robust.rho(kind, delta, ref_e2)[0].sum())
        assert abs(chi[-1] - r0) <= RG.CHI_RTOL * abs(r0) + float(bound.sum())
    _, chi_ref, _ = T.gn_optimize(*a, 5, vk, ek, kind, delta)
    np.testing.assert_allclose(chi, chi_ref, rtol=RG.CHI_RTOL)
    assert w[bad].max() < 0.05 and np.median(np.delete(w, bad)) > 0.7
    # the steps themselves: the robust system's backward error
    rc, p1, _, _, _ = ctx.gn_optimize_typed(*a, 1, **_kw(g), kind="cauchy", delta=delta)
    assert T.step_backward_error(g["poses"], p1, *a[1:], vk, ek, kind, delta) <= TC.OMEGA_MAX


def test_typed_robust_call_then_batched_robust_condensed_graphs(ctx):
    """The two robust linearisations side by side in one process: a typed Cauchy call on mixed257 (robust + typed, one job), then
    a robot graph's robust condensed graphs for two peers in one batch (robust, batched -- a robot graph is never typed).  The
    batch is held to the single calls on the same edges, gauge and query, at tests/test_robust_marginals_gpu.py's bars."""
    from cg_mrslam_amd import synth
    from cg_mrslam_amd.condensed import RobotGraph
    from ref_condensed import select_gauge_centroid
    from reference_cases import EST_ATOL, INFO_RTOL
    g = TC.case("mixed257")
    rc, _, chi, e2, w = ctx.gn_optimize_typed(*_a(g), 2, **_kw(g), kind="cauchy", delta=3.0)
    assert rc == 0 and np.all(np.isfinite(chi)) and np.all(np.isfinite(e2)) and np.all((w > 0) & (w <= 1))
    V = 300
    h = synth.make_pose_graph(V, 900, seed=23, id_base=0)
    ids = h["ids"].astype(np.int64)
    e = (h["edge_from"], h["edge_to"], h["meas"], h["info"])
    rg = RobotGraph(ctx, 0, 3)
    try:
        rg.add_vertices(ids, h["poses"], h["fixed"])
        rg.add_edges(ids[e[0]], ids[e[1]], e[2], e[3])
        rg.set_edge_robust("cauchy", 1.0)
        assert rg.optimize(4)[0] == 0
        want = {p: np.sort(np.random.default_rng(5 + p).choice(V, 6 + 2 * p, replace=False)).astype(np.int32) for p in (1, 2)}
        for p, idx in want.items():
            rg.insertOutClosure(p, ids[idx])
        rg.set_condensed_robust(True)
        assert rg.computeCondensedGraph(-1) == 2
        poses = rg.poses()
        for p, idx in want.items():
            gid, to, est, iu = rg.condensed(p)
            gauge = int(idx[select_gauge_centroid(poses[idx, :2])])
            assert gid == ids[gauge]
            to1, est1, iu1, _, _, _ = ctx.condense_robust(poses, *e, gauge, idx, "cauchy", 1.0)
            assert np.array_equal(to, ids[to1])
            d = est - est1
            d[:, 2] = synth.normalize_theta(d[:, 2])
            assert np.abs(d).max() <= EST_ATOL
            for k in range(len(to)):
                assert np.linalg.norm(iu[k] - iu1[k]) <= INFO_RTOL * np.linalg.norm(iu1[k]), (p, int(to[k]))
    finally:
        rg.close()


@pytest.mark.parametrize("name", ["mixed257", "leaf_and_hub"])
def test_marginals_against_reference(ctx, name):
    g = TC.case(name)
    vk, ek = TC.kinds(g)
    a = _a(g)
    rc, p, _ = ctx.gn_optimize_typed(*a, 3, **_kw(g))
    assert rc == 0
    nV, ef, et = len(p), g["edge_from"], g["edge_to"]
    want, want_x, err = T.marginal_blocks(p, *a[1:], vk, ek, pairs=list(zip(ef, et)))
    assert err <= TC.REF_ERR_MAX, "the reference itself is not accurate enough here"
    query = np.arange(nV, dtype=np.int32)
    cov_q = ctx.marginals_typed(p, *a[1:], query, **_kw(g))
    cov_a, cross = ctx.marginals_all_typed(p, *a[1:], cross=True, **_kw(g))
    fx = T.active_fixed(nV, g["fixed"], ef, et)
    worst = 0.0
    for cov in (cov_q, cov_a):
        for v in range(nV):
            if fx[v]:
                assert np.all(cov[v] == 0), v
                continue
            if vk[v] == 1:
                assert np.all(cov[v][2, :] == 0) and np.all(cov[v][:, 2] == 0), v
            e = np.linalg.norm(cov[v] - want[v]) / np.linalg.norm(want[v])
            worst = max(worst, e)
            assert e <= TC.MARG_TAU, (v, e)
    for v in range(nV):                                           # the two calls agree with each other
        assert np.linalg.norm(cov_q[v] - cov_a[v]) <= TC.MARG_TAU * max(np.linalg.norm(want[v]), 1e-300), v
    for k in range(len(ef)):
        if ef[k] == et[k]:
            continue                                              # (a prior's "cross" block is its vertex's diagonal block)
        if fx[ef[k]] or fx[et[k]]:
            assert np.all(cross[k] == 0), k
            continue
        if ek[k] == 1:
            assert np.all(cross[k][:, 2] == 0), k
        scale = np.sqrt(np.linalg.norm(want[ef[k]]) * np.linalg.norm(want[et[k]]))
        assert np.linalg.norm(cross[k] - want_x[k]) <= TC.MARG_TAU * scale, k
    print(f"{name}: largest relative block error {worst:.2e}")


def test_invalid_combinations_are_rejected(ctx):
    g = TC.case("mixed255")
    vk, ek = TC.kinds(g)
    ef, et = g["edge_from"], g["edge_to"]
    k0 = int(np.flatnonzero((ek == 0) & (ef != et))[0])
    k1 = int(np.flatnonzero(ek == 1)[0])
    k3 = int(np.flatnonzero(ek == 3)[0])
    k4 = int(np.flatnonzero(ek == 4)[0])
    pt = int(np.flatnonzero(vk == 1)[0])

    def variant(edge, kind=None, frm=None, to=None, vkind=None):
        e2, f2, t2, v2 = ek.copy(), ef.copy(), et.copy(), vk.copy()
        if kind is not None:
            e2[edge] = kind
        if frm is not None:
            f2[edge] = frm
        if to is not None:
            t2[edge] = to
        if vkind is not None:
            v2[vkind[0]] = vkind[1]
        return edge, (g["poses"], g["fixed"], f2, t2, g["meas"], g["info"]), dict(vertex_kind=v2, edge_kind=e2)

    bad = [variant(k1, frm=pt),                    # a landmark observation from a point
           variant(k1, to=int(ef[k1])),            # ... to a pose
           variant(k0, to=pt),                     # an EDGE_SE2 that touches a point
           variant(k3, frm=pt, to=pt),             # a pose prior on a point
           variant(k4, frm=pt, to=pt),             # a position prior on a point
           variant(k3, to=int(ef[k0]) if ef[k0] != ef[k3] else int(et[k0])),      # a prior with from != to
           variant(k0, kind=2), variant(k0, kind=5), variant(k4, kind=200)]      # reserved / unknown kinds
    calls = (lambda a, kw: ctx.gn_optimize_typed(*a, 2, **kw), lambda a, kw: ctx.lm_optimize_typed(*a, 2, **kw),
             lambda a, kw: ctx.dl_optimize_typed(*a, 2, **kw), lambda a, kw: ctx.marginals_typed(*a, [0, 1], **kw),
             lambda a, kw: ctx.marginals_all_typed(*a, **kw))
    for edge, a, kw in bad:
        for call in calls:
            with pytest.raises(CgmrError) as ei:
                call(a, kw)
            assert ei.value.code == -1 and f"edge {edge} " in str(ei.value), (edge, str(ei.value))
    # the context is as good as before
    rc, _, _ = ctx.gn_optimize_typed(*_a(g), 1, **_kw(g))
    assert rc == 0


def test_graph_slam_routes_typed_graphs(ctx, tmp_path):
    """GraphSLAM on a graph with landmarks and priors: optimize, chi2, robustChi2, computeMarginals and the .g2o round trip."""
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    c = TC.case("mixed256")
    vk, ek = TC.kinds(c)
    g = PoseGraph(np.arange(len(c["poses"])), c["poses"], c["fixed"], c["edge_from"], c["edge_to"], c["meas"], c["info"],
                  vertex_kind=vk, edge_kind=ek)
    g.save_g2o(str(tmp_path / "m.g2o"), precision=17)
    s = GraphSLAM(PoseGraph.load_g2o(str(tmp_path / "m.g2o")), ctx)
    assert s.chi2() == pytest.approx(T.chi2(c["poses"], *_a(c)[2:], ek), rel=1e-9)
    s.optimize(5)
    _, chi_ref, _ = T.gn_optimize(*_a(c), 5, vk, ek)
    assert s.last_status == 0 and s.last_iterations == 5
    np.testing.assert_allclose(s.last_chi2, chi_ref, rtol=TC.CHI_RTOL)
    assert s.chi2() == pytest.approx(chi_ref[-1], rel=TC.CHI_RTOL)
    cov = s.computeMarginals()
    assert cov.shape == (len(vk), 3, 3) and np.all(cov[vk == 1][:, 2, :] == 0) and np.all(cov[vk == 0][:, 2, 2] > 0)
    s.setRobustKernel("Cauchy", 3.0)
    assert s.robustChi2() == pytest.approx(T.chi2(s.graph.poses, *_a(c)[2:], ek, 3, 3.0), rel=1e-9)
    for alg in ("levenberg", "dl"):
        t = GraphSLAM(PoseGraph.load_g2o(str(tmp_path / "m.g2o")), ctx, algorithm=alg)
        t.optimize(5)
        assert t.last_status == 0 and t.last_chi2[-1] == pytest.approx(chi_ref[-1], rel=1e-3)
