"""Graduated non-convexity on the device (include/cgmr.h: cgmr_gnc_optimize) against the float64 contract of tests/ref_gnc.py,
on the cases of tests/gnc_cases.py (whose reach predicates tests/test_gnc_cpu.py proves on the reference alone)."""
import numpy as np
import pytest

import gnc_cases as GC
import ref_numpy as R
import ref_typed
import typed_cases
from test_robust_gpu import STAT_RTOL, e2_bound

pytestmark = pytest.mark.gpu

CHI_RTOL = typed_cases.CHI_RTOL      # 1e-6: cost records against the reference, per entry
POS_TOL, ANG_TOL = 1e-6, 1e-7        # SURVEY section 8(d)'s parity bar: metres, radians
COMPARED = ("hand", "og60", "og300", "mixed255", "mixed256", "mixed257", "tree600x")


@pytest.fixture(scope="module")
def ctx():
    from cg_mrslam_amd import Context
    c = Context(0)
    yield c
    c.close()


def run(ctx, name, loss, **kw):
    g = GC.case(name)
    kw.setdefault("inner_iters", g["inner_iters"])
    return ctx.gnc_optimize(*GC.args(g), loss=loss, barc_sq=g["barc_sq"], known_inliers=g["known"], vertex_kind=g["vk"],
                            edge_kind=g["ek"], **kw)


def check_poses(g, p, ref):
    d = p - ref
    assert float(np.abs(d[:, :2]).max()) <= POS_TOL, float(np.abs(d[:, :2]).max())
    assert float(np.abs(R.normalize_theta(d[:, 2])).max()) <= ANG_TOL
    if g["vk"] is not None:
        assert np.all(p[g["vk"] == 1, 2] == 0.0)                                 # a point's third component: untouched
    touched = np.zeros(len(p), bool)
    touched[g["edge_from"]] = touched[g["edge_to"]] = True
    still = (g["fixed"] != 0) | ~touched
    assert np.array_equal(p[still], g["poses"][still])                           # fixed and untouched vertices: bit for bit


def check_edge_chi2(g, p, e2):
    ref = ref_typed.edge_chi2(p, g["edge_from"], g["edge_to"], g["meas"], g["info"], ref_typed._kinds(p, g["edge_from"], g["vk"], g["ek"])[1])
    bound = e2_bound(p, g["info"], ref)
    assert np.all(np.abs(e2 - ref) <= bound), float(np.max(np.abs(e2 - ref) / np.maximum(bound, 1e-300)))


def check_against(g, out, ref, loss):
    n = ref["outer_done"]
    assert out["status"] == 0 and out["outer_done"] == n
    assert np.array_equal(out["partial"], ref["partial"])
    np.testing.assert_allclose(out["mu"], ref["mu"], rtol=STAT_RTOL, atol=0)
    np.testing.assert_allclose(out["cost"], ref["cost"], rtol=CHI_RTOL, atol=0)
    check_poses(g, out["poses"], ref["poses"])
    if loss == "tls":
        assert np.array_equal(out["weights"], ref["weights"])
    else:
        assert float(np.abs(out["weights"] - ref["weights"]).max()) <= 2 * CHI_RTOL
    check_edge_chi2(g, out["poses"], out["edge_chi2"])


# ------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("loss", ["tls", "gm"])
@pytest.mark.parametrize("name", COMPARED)
def test_contract_per_case(ctx, name, loss):
    g = GC.case(name)
    out = run(ctx, name, loss)
    check_against(g, out, GC.reference(name, loss), loss)
    if loss == "tls":
        assert np.array_equal(np.flatnonzero(out["weights"] == 0.0), g["bad"])
    st = ctx.gnc_last_stats()
    assert st["inner_iterations"] == out["outer_done"] * g["inner_iters"]
    assert st["host_waits"] == -(-out["outer_done"] // 8)                        # outer_per_wait = 8: one wait per round


def test_hand_worked_literals(ctx):
    g = GC.case("hand")
    out = run(ctx, "hand", "tls", max_outer=1)
    assert out["mu"][0] == pytest.approx(g["mu0"], rel=1e-15) and out["partial"].tolist() == [1] and out["outer_done"] == 1
    np.testing.assert_allclose(out["weights"], g["w_first"], rtol=1e-14, atol=0)
    out = run(ctx, "hand", "tls")
    assert out["weights"].tolist() == g["w_final"].tolist()
    np.testing.assert_allclose(out["poses"][1], [1.0, 0.0, 0.0], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("loss", ["tls", "gm"])
@pytest.mark.parametrize("name", ["clean", "clean_typed"])
def test_nothing_to_reject_is_the_plain_call_bit_for_bit(ctx, name, loss):
    g = GC.case(name)
    out = run(ctx, name, loss)
    if g["vk"] is None:
        rc, p, chi = ctx.gn_optimize(*GC.args(g), g["inner_iters"])
    else:
        rc, p, chi = ctx.gn_optimize_typed(*GC.args(g), g["inner_iters"], vertex_kind=g["vk"], edge_kind=g["ek"])
    assert out["status"] == rc == 0 and np.array_equal(out["poses"], p)
    assert out["outer_done"] == 1 and out["mu"][0] == 0.0 and out["partial"][0] == 0 and np.all(out["weights"] == 1.0)
    assert out["cost"][0] == chi[0]                                              # every weight 1: the plain chi2, the same sum
    check_edge_chi2(g, out["poses"], out["edge_chi2"])


# ------------------------------------------------------------------------------------------------------------------- 3
def test_three_inner_iterations(ctx):
    g = GC.case("og60")
    out = run(ctx, "og60", "tls", inner_iters=3)
    check_against(g, out, GC.reference("og60", "tls", inner_iters=3), "tls")
    assert ctx.gnc_last_stats()["inner_iterations"] == 3 * out["outer_done"]


def test_max_outer_cuts_the_call(ctx):
    g = GC.case("og60")
    out = run(ctx, "og60", "tls", max_outer=5)
    ref = GC.reference("og60", "tls", max_outer=5)
    assert out["outer_done"] == 5 and out["partial"][4] > 0
    np.testing.assert_allclose(out["mu"], ref["mu"], rtol=STAT_RTOL, atol=0)
    np.testing.assert_allclose(out["cost"], ref["cost"], rtol=CHI_RTOL, atol=0)
    assert np.array_equal(out["partial"], ref["partial"])
    np.testing.assert_allclose(out["weights"], ref["weights"], rtol=0, atol=2 * CHI_RTOL)     # (partial weights: as GM's)
    check_poses(g, out["poses"], ref["poses"])


@pytest.mark.parametrize("name,loss", [("og60", "tls"), ("mixed257", "gm")])
def test_result_does_not_depend_on_outer_per_wait(ctx, name, loss):
    outs = [run(ctx, name, loss, outer_per_wait=n) for n in (1, 8, 100)]
    waits = []
    for n, o in zip((1, 8, 100), outs):
        for key in ("poses", "weights", "edge_chi2", "mu", "cost", "partial"):
            assert np.array_equal(o[key], outs[1][key]), (n, key)
        assert o["outer_done"] == outs[1]["outer_done"]
        waits.append(-(-o["outer_done"] // n))
    run(ctx, name, loss, outer_per_wait=1)
    assert ctx.gnc_last_stats()["host_waits"] == waits[0]


@pytest.mark.parametrize("name,loss", [("og60", "tls"), ("mixed257", "tls"), ("og60", "gm")])
def test_device_entry_point_is_bit_identical(ctx, name, loss):
    import torch
    g = GC.case(name)
    host = run(ctx, name, loss)
    dp, dm, di = (torch.from_numpy(np.ascontiguousarray(g[k], dtype=np.float64)).to("cuda:0") for k in ("poses", "meas", "info"))
    dev = ctx.gnc_optimize_dev(dp.data_ptr(), len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"], dm.data_ptr(), di.data_ptr(),
                               loss=loss, barc_sq=g["barc_sq"], known_inliers=g["known"], vertex_kind=g["vk"], edge_kind=g["ek"])
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy(), host["poses"])
    for key in ("weights", "edge_chi2", "mu", "cost", "partial"):
        assert np.array_equal(dev[key], host[key]), key
    assert dev["outer_done"] == host["outer_done"] and dev["status"] == 0


# ------------------------------------------------------------------------------------------------------------------- 4
def test_starved_vertex_returns_a_cholesky_code(ctx):
    from cg_mrslam_amd._lib import CGMR_E_CHOLESKY_BASE, CgmrError
    g = GC.case("starved")
    ref = GC.reference("starved", "tls")
    out = run(ctx, "starved", "tls", raise_on_cholesky=False)
    assert out["status"] == CGMR_E_CHOLESKY_BASE - ref["failed"] == CGMR_E_CHOLESKY_BASE - 3
    assert out["outer_done"] == ref["outer_done"] and np.all(np.isfinite(out["poses"]))
    check_poses(g, out["poses"], ref["poses"])                                   # the last good update
    # (the call ends inside the band: the other free edges carry partial weights, compared as GM's are)
    assert float(np.abs(out["weights"] - ref["weights"]).max()) <= 2 * CHI_RTOL and out["weights"][g["bad"]].tolist() == [0.0, 0.0]
    assert np.array_equal(out["weights"] == 0.0, ref["weights"] == 0.0) and np.array_equal(out["partial"], ref["partial"])
    check_edge_chi2(g, out["poses"], out["edge_chi2"])
    with pytest.raises(CgmrError):
        run(ctx, "starved", "tls")
    # the context is as good as new: a plain typed call on the same graph
    rc, p, chi = ctx.gn_optimize_typed(*GC.args(g), 2, vertex_kind=g["vk"], edge_kind=g["ek"])
    want, _, _ = ref_typed.gn_optimize(*GC.args(g), 2, g["vk"], g["ek"])
    assert rc == 0 and float(np.abs(p - want).max()) <= POS_TOL


def test_invalid_parameters_are_refused(ctx):
    from cg_mrslam_amd._lib import CgmrError
    g = GC.case("hand")
    a = GC.args(g)
    nE = len(g["edge_from"])
    bad_c = np.ones(nE)
    for kw in (dict(loss=2), dict(loss=-1), dict(mu_factor=1.0), dict(mu_factor=0.5), dict(mu_factor=float("nan")),
               dict(mu_factor=float("inf")), dict(max_outer=0), dict(inner_iters=0), dict(outer_per_wait=0), dict(barc_sq=0.0),
               dict(barc_sq=-1.0), dict(barc_sq=float("nan")), dict(barc_sq=float("inf")),
               dict(barc_sq=np.where(np.arange(nE) == 1, 0.0, bad_c)), dict(barc_sq=np.where(np.arange(nE) == 2, np.nan, bad_c)),
               dict(barc_sq=np.where(np.arange(nE) == 0, np.inf, bad_c)), dict(barc_sq=np.where(np.arange(nE) == 0, -2.0, bad_c)),
               dict(vertex_kind=np.array([0, 2], np.uint8)), dict(edge_kind=np.array([0, 0, 5], np.uint8)),
               dict(edge_kind=np.array([0, 1, 0], np.uint8)), dict(edge_kind=np.array([3, 0, 0], np.uint8))):
        with pytest.raises(CgmrError) as e:
            ctx.gnc_optimize(*a, **kw)
        assert e.value.code == -1, kw
    with pytest.raises(ValueError):
        ctx.gnc_optimize(*a, loss="huber")
    with pytest.raises(TypeError):
        ctx.gnc_optimize(*a, kind="cauchy")                                      # not combined with the robust kernels
    # ... and the call still works afterwards
    assert ctx.gnc_optimize(*a, barc_sq=1.0, known_inliers=g["known"])["weights"].tolist() == [1.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", ["og60", "mixed257"])
def test_graph_slam_optimize_gnc(ctx, name):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = GC.case(name)
    pg = PoseGraph(np.arange(len(g["poses"])), g["poses"].copy(), g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"],
                   vertex_kind=g["vk"], edge_kind=g["ek"])
    s = GraphSLAM(pg, ctx=ctx)
    s.optimizeGNC(barc_sq=g["barc_sq"], known_inliers=np.flatnonzero(g["known"]))
    ref = GC.reference(name, "tls")
    assert np.array_equal(s.rejectedEdges(), g["bad"]) and s.last_status == 0 and s.last_iterations == ref["outer_done"]
    assert len(s.last_mu) == ref["outer_done"] and len(s.last_chi2) == ref["outer_done"] + 1
    assert np.array_equal(s.last_weights, ref["weights"]) and len(s.last_edge_chi2) == len(g["edge_from"])
    check_poses(g, pg.poses, ref["poses"])
    # optimize() behaves as before: the plain (typed) call from the same estimates
    before = pg.poses.copy()
    s.optimize(2)
    if g["vk"] is None:
        rc, p, chi = ctx.gn_optimize(before, *GC.args(g)[1:], 2)
    else:
        rc, p, chi = ctx.gn_optimize_typed(before, *GC.args(g)[1:], 2, vertex_kind=g["vk"], edge_kind=g["ek"])
    assert s.last_status == rc == 0 and np.array_equal(pg.poses, p) and np.array_equal(s.last_chi2, chi)
    assert s.last_weights is None and s.last_iterations == 2


def test_no_state_leaks_into_the_plain_call(ctx):
    g = GC.case("og300")
    a = GC.args(g)
    rc0, p0, chi0 = ctx.gn_optimize(*a, 3)
    run(ctx, "og300", "tls")
    rc1, p1, chi1 = ctx.gn_optimize(*a, 3)
    run(ctx, "mixed256", "gm")
    rc2, p2, chi2 = ctx.gn_optimize(*a, 3)
    assert rc0 == rc1 == rc2 == 0
    assert np.array_equal(p0, p1) and np.array_equal(chi0, chi1) and np.array_equal(p0, p2) and np.array_equal(chi0, chi2)
