"""Max-mixture edges on the device (include/cgmr.h: cgmr_mixture) against the float64 contract of tests/ref_mixture.py, on the
cases of tests/mixture_cases.py (whose reach predicates tests/test_mixture_cpu.py proves on the reference alone)."""
import numpy as np
import pytest

import mixture_cases as MC
import ref_numpy as R
import ref_robust
import typed_cases
from test_dogleg_gpu import check_trace as dl_check_trace
from test_lm_gpu import check_trace as lm_check_trace
from test_lm_gpu import rounding_floor

pytestmark = pytest.mark.gpu

CHI_RTOL = typed_cases.CHI_RTOL      # 1e-6: chi2 before every iteration against the reference, per entry
POS_TOL, ANG_TOL = 1e-6, 1e-7        # the device-to-reference bars of tests/test_chordal_gpu.py: metres, radians


@pytest.fixture(scope="module")
def ctx():
    from cg_mrslam_amd import Context
    c = Context(0)
    yield c
    c.close()


def kinds(g):
    return {} if g["vk"] is None else dict(vertex_kind=g["vk"], edge_kind=g["ek"])


def check_poses(g, p, ref):
    d = p - ref
    assert float(np.abs(d[:, :2]).max()) <= POS_TOL, float(np.abs(d[:, :2]).max())
    assert float(np.abs(R.normalize_theta(d[:, 2])).max()) <= ANG_TOL
    assert np.array_equal(p[g["fixed"] != 0], g["poses"][g["fixed"] != 0])


# ------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(MC.CASES))
def test_gauss_newton_per_case(ctx, name):
    g, ref = MC.case(name), MC.reference(name)
    rc, p, chi, sel = ctx.gn_optimize_mixture(*MC.args(g), g["iters"], g["mix"], **kinds(g))
    assert rc == 0
    np.testing.assert_allclose(chi, ref["chi2"], rtol=CHI_RTOL, atol=0)
    check_poses(g, p, ref["poses"])
    assert np.array_equal(sel, ref["selected"])


@pytest.mark.parametrize("name", ["g60_k2_last", "g300_k5_random", "switching"])
def test_ends_at_the_clean_optimum_where_the_plain_path_does_not(ctx, name):
    g = MC.case(name)
    clean = MC.clean_optimum(name)
    p = ctx.gn_optimize_mixture(*MC.args(g), g["iters"], g["mix"])[1]
    plain = ctx.gn_optimize(*MC.args(g), g["iters"])[1]
    assert ref_robust.rms(p, clean) <= POS_TOL and ref_robust.rms(plain, clean) > 1.0


def test_tie_goes_to_the_lowest_index(ctx):
    g = MC.case("tie")
    sel = ctx.gn_optimize_mixture(*MC.args(g), g["iters"], g["mix"])[3]
    assert sel[g["exempt"][0]] == 0
    assert ctx.mixture_select(*MC.args(g), g["mix"])[1][g["exempt"][0]] == 0


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", MC.TRUST_REGION)
def test_levenberg_against_the_reference_policy(ctx, name):
    g, ref = MC.case(name), MC.reference(name, "lm")
    rc, p, chi, lam, tri, done, sel = ctx.lm_optimize_mixture(*MC.args(g), MC.TR_ITERS, g["mix"])
    assert rc == 0
    k = lm_check_trace(name, ref["out"], chi, lam, tri, done, rounding_floor(g))
    assert k >= 1
    np.testing.assert_allclose(chi, ref["chi2"], rtol=CHI_RTOL, atol=0)
    check_poses(g, p, ref["poses"])
    assert np.array_equal(sel, ref["selected"])


@pytest.mark.parametrize("name", MC.TRUST_REGION)
def test_dogleg_against_the_reference_policy(ctx, name):
    g, ref = MC.case(name), MC.reference(name, "dl")
    rc, p, chi, dlt, tri, stp, done, sel = ctx.dl_optimize_mixture(*MC.args(g), MC.TR_ITERS, g["mix"])
    assert rc == 0
    k = dl_check_trace(name, ref["out"], chi, dlt, tri, stp, done, rounding_floor(g))
    assert k >= 1
    check_poses(g, p, ref["poses"])
    assert np.array_equal(sel, ref["selected"])


# ------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["g60_k5_random", "typed"])
def test_device_entry_points_bit_for_bit(ctx, name):
    import torch
    g = MC.case(name)
    kw = kinds(g)
    dev = torch.device("cuda:0")
    d_m = torch.tensor(g["meas"], dtype=torch.float64, device=dev).contiguous()
    d_i = torch.tensor(g["info"], dtype=torch.float64, device=dev).contiguous()
    nV = len(g["poses"])
    s = (g["fixed"], g["edge_from"], g["edge_to"])
    for alg, iters in (("gn", g["iters"]), ("lm", 4), ("dl", 4)):
        host = getattr(ctx, alg + "_optimize_mixture")(*MC.args(g), iters, g["mix"], **kw)
        d_p = torch.tensor(g["poses"], dtype=torch.float64, device=dev).contiguous()
        torch.cuda.synchronize()
        out = getattr(ctx, alg + "_optimize_mixture_dev")(d_p.data_ptr(), nV, *s, d_m.data_ptr(), d_i.data_ptr(), iters, g["mix"], **kw)
        assert out[0] == host[0] == 0
        np.testing.assert_array_equal(d_p.cpu().numpy(), host[1])
        for a, b in zip(out[1:], host[2:]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["g60_k2_last", "typed"])
def test_one_component_everywhere_is_the_plain_call_bit_for_bit(ctx, name):
    g = MC.case(name)
    n = len(g["edge_from"])
    one = (np.arange(n + 1, dtype=np.int32), g["meas"], g["info"], np.full(n, 0.25))
    kw = kinds(g)
    typed = g["vk"] is not None
    for alg, iters in (("gn", 5), ("lm", 4), ("dl", 4)):
        plain = getattr(ctx, alg + ("_optimize_typed" if typed else "_optimize"))(*MC.args(g), iters, **kw)
        for mix in (one, None):
            out = getattr(ctx, alg + "_optimize_mixture")(*MC.args(g), iters, mix, **kw)
            assert not out[-1].any()
            for a, b in zip(out[:-1], plain):
                np.testing.assert_array_equal(a, b)
    chi, sel = ctx.mixture_select(*MC.args(g), one, **kw)
    assert chi == plain_chi2(ctx, g, kw) and not sel.any()


def plain_chi2(ctx, g, kw):
    if kw:
        return float(ctx.gn_optimize_typed(*MC.args(g), 0, **kw)[2][0])
    return float(ctx.gn_optimize(*MC.args(g), 0)[2][0])


@pytest.mark.parametrize("name", ["anchor_hi", "switching", "typed", "b257"])
def test_mixture_select_is_the_optimise_calls_first_and_last_chi2(ctx, name):
    g, ref = MC.case(name), MC.reference(name)
    kw = kinds(g)
    rc, p, chi, sel = ctx.gn_optimize_mixture(*MC.args(g), g["iters"], g["mix"], **kw)
    c0, s0 = ctx.mixture_select(*MC.args(g), g["mix"], **kw)
    c1, s1 = ctx.mixture_select(p, *MC.args(g)[1:], g["mix"], **kw)
    assert c0 == chi[0] and c1 == chi[-1]
    assert np.array_equal(s0, ref["sels"][0]) and np.array_equal(s1, sel)


@pytest.mark.parametrize("name", ["switching", "typed"])
def test_two_runs_are_bit_identical(ctx, name):
    g = MC.case(name)
    kw = kinds(g)
    for alg, iters in (("gn", g["iters"]), ("lm", 4), ("dl", 4)):
        a = getattr(ctx, alg + "_optimize_mixture")(*MC.args(g), iters, g["mix"], **kw)
        b = getattr(ctx, alg + "_optimize_mixture")(*MC.args(g), iters, g["mix"], **kw)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------- 4
def _bad_mixtures(g):
    """(label, mixture, the edge its message must name) for every CGMR_E_INVALID case of the header."""
    ptr, cm, ci, cw = g["mix"]
    k = int(g["multi"][2])
    p = int(ptr[k])
    out = []
    q = ptr.copy(); q[0] = 1
    out.append(("comp_ptr does not start at 0", (q, cm, ci, cw), 0))
    q = ptr.copy(); q[k + 1:] -= 2                                       # (edge k loses both components)
    out.append(("an edge without a component", (q, cm, ci, cw), k))
    q = ptr.copy(); q[k + 1] = q[k] - 1
    out.append(("comp_ptr decreases", (q, cm, ci, cw), k))
    for label, w in (("weight 0", 0.0), ("negative weight", -1.0), ("weight inf", np.inf), ("weight nan", np.nan)):
        v = cw.copy(); v[p + 1] = w
        out.append((label, (ptr, cm, ci, v), k))
    neg = [-1.0, 0.0, 0.0, 1.0, 0.0, 1.0]                                 # (negative in one, two and three dimensions)
    for label, u6 in (("det 0", 0.0 * ci[p]), ("det negative", neg), ("det inf", np.full(6, np.inf)), ("det nan", np.full(6, np.nan))):
        u = ci.copy(); u[p] = u6
        out.append((label, (ptr, cm, u, cw), k))
    return out


@pytest.mark.parametrize("name", ["g60_k2_last", "typed"])
def test_invalid_mixtures_are_refused_before_the_device_is_touched(ctx, name):
    from cg_mrslam_amd._lib import CgmrError
    g = MC.case(name)
    kw = kinds(g)
    ctx.gn_optimize_mixture(*MC.args(g), 1, g["mix"], **kw)
    before = ctx.symbolic_cache_stats()
    for label, mix, edge in _bad_mixtures(g):
        for call in (lambda m: ctx.gn_optimize_mixture(*MC.args(g), 2, m, **kw), lambda m: ctx.lm_optimize_mixture(*MC.args(g), 2, m, **kw),
                     lambda m: ctx.dl_optimize_mixture(*MC.args(g), 2, m, **kw), lambda m: ctx.mixture_select(*MC.args(g), m, **kw)):
            with pytest.raises(CgmrError) as e:
                call(mix)
            assert e.value.code == -1 and f"edge {edge}" in str(e.value), (label, str(e.value))
    assert ctx.symbolic_cache_stats() == before                          # no call reached the structure, let alone a launch


def test_one_component_edges_are_not_checked(ctx):
    """K = 1: the plain chi2 -- Omega may be singular and the weight anything."""
    g = MC.case("g60_k2_last")
    ptr, cm, ci, cw = (a.copy() for a in g["mix"])
    single = np.flatnonzero(np.diff(ptr) == 1)
    cw[ptr[single]] = -3.0
    ci[ptr[single[5]]] = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]                  # (singular)
    info = g["info"].copy()
    info[single[5]] = ci[ptr[single[5]]]
    a = MC.args(g)[:5] + (info,)
    chi, sel = ctx.mixture_select(*a, (ptr, cm, ci, cw))
    ref = MC.RM.chi2(g["poses"], g["edge_from"], g["edge_to"], (ptr, cm, ci, np.abs(cw)))
    assert chi == pytest.approx(ref, rel=CHI_RTOL)


# ------------------------------------------------------------------------------------------------------------------- 5
def _slam(ctx, name, algorithm="gn"):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = MC.case(name)
    pg = PoseGraph(np.arange(len(g["poses"])), g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"],
                   vertex_kind=g["vk"], edge_kind=g["ek"])
    ptr, cm, ci, cw = g["mix"]
    for k in g["multi"]:
        pg.set_edge_mixture(int(k), [(cw[p], cm[p], ci[p]) for p in range(ptr[k], ptr[k + 1])])
    return g, GraphSLAM(pg, ctx=ctx, algorithm=algorithm)


@pytest.mark.parametrize("algorithm", ["gn", "levenberg", "dl"])
def test_graphslam_routes_to_the_mixture_path(ctx, algorithm):
    g, slam = _slam(ctx, "g60_k5_random", algorithm)
    ref = MC.reference("g60_k5_random")
    plain0 = slam.chi2()
    assert plain0 == plain_chi2(ctx, g, {})                              # chi2(): the plain one of the components 0, as ever
    assert slam.mixtureChi2() == pytest.approx(ref["chi2"][0], rel=CHI_RTOL)
    slam.optimize(g["iters"])
    assert slam.last_status == 0 and np.array_equal(slam.last_selected, ref["selected"])
    assert np.array_equal(slam.selectedComponents(), ref["selected"])
    assert ref_robust.rms(slam.graph.poses, MC.clean_optimum("g60_k5_random")) <= POS_TOL
    assert slam.mixtureChi2() == pytest.approx(ref["chi2"][-1], rel=CHI_RTOL)
    flat = slam.collapseMixtures()
    assert not flat.has_mixtures and np.array_equal(flat.meas, g["clean"]["meas"])
    from cg_mrslam_amd.graph import GraphSLAM
    assert GraphSLAM(flat, ctx=ctx).chi2() == pytest.approx(ref["chi2"][-1], rel=CHI_RTOL)
    cov = GraphSLAM(flat, ctx=ctx).computeMarginals()                    # the supported route to the marginals
    assert cov.shape == (len(g["poses"]), 3, 3) and np.all(np.isfinite(cov))


def test_graphslam_null_hypothesis(ctx):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g, ref = MC.case("null"), MC.reference("null")
    pg = PoseGraph(np.arange(len(g["poses"])), g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
    slam = GraphSLAM(pg, ctx=ctx)
    slam.addNullHypothesis(g["closure"], weight=1.0, scale=MC.NULL_SCALE)
    slam.optimize(g["iters"])
    np.testing.assert_allclose(slam.last_chi2, ref["chi2"], rtol=CHI_RTOL, atol=0)
    assert np.array_equal(slam.last_selected, ref["selected"]) and np.all(slam.last_selected[g["bad"]] == 1)
