"""Chordal initialisation on the device against tests/ref_chordal.py from the same start: every stage combination, the counts,
the chi2 outputs, the device-resident entry points, a system without a gauge, the end-to-end recovery from scrambled
estimates, and the spanning-tree guess against the oracle's.  Bars: tests/chordal_cases.py (tests/test_gn_gpu.py's for one
solve through the same factorisation)."""
import numpy as np
import pytest

import chordal_cases as CC
import ref_chordal as RC
import ref_numpy as R
import ref_assoc as RA
from cg_mrslam_amd import synth
from cg_mrslam_amd.graph import GraphSLAM, PoseGraph

pytestmark = pytest.mark.gpu


def _chi2(g, poses):
    a = CC.args(g)[2:]
    return RA.chi2(poses, *a, g["ek"]) if "ek" in g else R.chi2(poses, *a)      # (ref_typed's, plus the bearings)


def _check(name, stages, out):
    g, ref = CC.case(name), CC.reference(name, stages)
    dp, da = RC.differences(out["poses"], ref["poses"])
    print(f"{name} stages {stages}: status {out['status']} position {dp:.3e} heading {da:.3e} counts {out['counts'].tolist()} "
          f"chi2 {out['chi2'].tolist()}")
    assert out["status"] == 0
    assert out["counts"].tolist() == ref["counts"].tolist()
    assert dp <= CC.POS_ATOL and da <= CC.ANG_ATOL
    if not stages & 1:
        np.testing.assert_array_equal(out["poses"][:, 2], g["poses"][:, 2])      # the translation stage's dummy step is exactly 0
    if not stages & 2:
        np.testing.assert_array_equal(out["poses"][:, :2], g["poses"][:, :2])
    np.testing.assert_array_equal(out["poses"][g["fixed"] != 0], g["poses"][g["fixed"] != 0])
    np.testing.assert_allclose(out["chi2"][0], _chi2(g, g["poses"]), rtol=CC.CHI_RTOL, atol=1e-18)
    np.testing.assert_allclose(out["chi2"][1], _chi2(g, out["poses"]), rtol=CC.CHI_RTOL, atol=1e-18)


@pytest.mark.parametrize("stages", [1, 2, 3])
@pytest.mark.parametrize("name", list(CC.PLAIN))
def test_plain_matches_reference(ctx, name, stages):
    _check(name, stages, ctx.chordal_initialize(*CC.args(CC.case(name)), stages))


@pytest.mark.parametrize("stages", [1, 2, 3])
@pytest.mark.parametrize("name", list(CC.TYPED))
def test_typed_matches_reference(ctx, name, stages):
    g = CC.case(name)
    _check(name, stages, ctx.chordal_initialize(*CC.args(g), stages, **CC.kinds(g)))


def test_left_out_vertices_come_back_untouched(ctx):
    """A bearing-only point, leaf_and_hub's point that no edge touches, the isolated vertices of fixed_dup_iso: bit for bit."""
    g = CC.case("bearing_lone")
    out = ctx.chordal_initialize(*CC.args(g), 3, **CC.kinds(g))
    v = g["lone_bearing_point"]
    np.testing.assert_array_equal(out["poses"][v], g["poses"][v])
    assert out["counts"].tolist() == [12, 13, 0]
    g = CC.case("leaf_and_hub")
    out = ctx.chordal_initialize(*CC.args(g), 3, **CC.kinds(g))
    np.testing.assert_array_equal(out["poses"][[g["lone"], g["fixed_point"]]], g["poses"][[g["lone"], g["fixed_point"]]])
    g = CC.case("fixed_dup_iso")
    out = ctx.chordal_initialize(*CC.args(g), 3)
    np.testing.assert_array_equal(out["poses"][-2:], g["poses"][-2:])


def test_result_does_not_depend_on_the_start(ctx):
    g = CC.case("pg300_scrambled")
    a = CC.args(g)
    one = ctx.chordal_initialize(*a, 3)
    two = ctx.chordal_initialize(g["start"], *a[1:], 3)
    dp, da = RC.differences(one["poses"], two["poses"])
    print(f"two starts: position {dp:.3e} heading {da:.3e}")
    assert dp <= CC.POS_ATOL and da <= CC.ANG_ATOL


@pytest.mark.parametrize("name", ["pg300_scrambled", "tree600"])
def test_device_entry_points_bit_for_bit(ctx, name):
    import torch
    g = CC.case(name)
    kw = CC.kinds(g)
    dev = torch.device("cuda:0")
    d_m = torch.tensor(g["meas"], dtype=torch.float64, device=dev).contiguous()
    d_i = torch.tensor(g["info"], dtype=torch.float64, device=dev).contiguous()
    for stages in (1, 2, 3):
        host = ctx.chordal_initialize(*CC.args(g), stages, **kw)
        d_p = torch.tensor(g["poses"], dtype=torch.float64, device=dev).contiguous()
        torch.cuda.synchronize()
        out = ctx.chordal_initialize_dev(d_p.data_ptr(), len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"], d_m.data_ptr(),
                                         d_i.data_ptr(), stages, **kw)
        assert out["status"] == 0 and "poses" not in out
        np.testing.assert_array_equal(d_p.cpu().numpy(), host["poses"])
        np.testing.assert_array_equal(out["chi2"], host["chi2"])
        np.testing.assert_array_equal(out["counts"], host["counts"])


@pytest.mark.parametrize("stages", [1, 2, 3])
def test_no_gauge_returns_a_cholesky_code(ctx, stages):
    """No fixed vertex and no prior: the first requested stage meets a zero pivot (exactly zero: chordal_cases.singular_pair),
    the call returns Gauss-Newton's code for its first iteration and the estimates are unchanged."""
    from cg_mrslam_amd._lib import CGMR_E_CHOLESKY_BASE, CgmrError
    g = CC.singular_pair()
    out = ctx.chordal_initialize(*CC.args(g), stages, raise_on_cholesky=False)
    assert out["status"] == CGMR_E_CHOLESKY_BASE
    np.testing.assert_array_equal(out["poses"], g["poses"])
    assert out["counts"].tolist() == [0, 0, 0]
    np.testing.assert_allclose(out["chi2"], R.chi2(g["poses"], *CC.args(g)[2:]), rtol=CC.CHI_RTOL)
    with pytest.raises(CgmrError):
        ctx.chordal_initialize(*CC.args(g), stages)
    gs = GraphSLAM(PoseGraph(np.arange(2), *CC.args(g)), ctx=ctx)
    gs.initializeChordal()                                       # must not raise
    assert gs.last_status == CGMR_E_CHOLESKY_BASE
    np.testing.assert_array_equal(gs.graph.poses, g["poses"])


def test_bad_stages_are_refused(ctx):
    from cg_mrslam_amd._lib import CgmrError
    import ctypes as C
    g = CC.case("v2e1")
    for bad in (0, 4):
        with pytest.raises(ValueError):
            ctx.chordal_initialize(*CC.args(g), bad)
    nV, p, (poses, fixed, nE, ef, et, meas, info), _keep = ctx._problem(*CC.args(g))
    rc = ctx.lib.cgmr_chordal_initialize(ctx.h, C.c_int(nV), poses, fixed, nE, ef, et, meas, info, C.c_int(0), None, None)
    assert rc == -1
    with pytest.raises(CgmrError):
        ctx._check(rc)


@pytest.mark.parametrize("name", list(CC.SCRAMBLES))
def test_graphslam_recovers_from_a_scramble(ctx, name):
    """initializeChordal() then optimize(5) ends at the chi2 of Gauss-Newton started from the truth; optimize(10) alone from
    the same scramble ends above 100 times that."""
    g = CC.case(name)
    a = CC.args(g)

    def slam(poses):
        pg = PoseGraph.from_synth(g)
        pg.poses[:] = poses
        return GraphSLAM(pg, ctx=ctx)

    best = slam(g["truth"])
    best.optimize(10)
    chi_opt = best.last_chi2[-1]
    gs = slam(g["poses"])
    gs.initializeChordal()
    assert gs.last_status == 0 and len(gs.last_chi2) == 2
    assert gs.last_init_counts.tolist() == CC.reference(name, 3)["counts"].tolist()
    np.testing.assert_allclose(gs.last_chi2, [R.chi2(g["poses"], *a[2:]), R.chi2(gs.graph.poses, *a[2:])], rtol=CC.CHI_RTOL)
    chi_init = gs.last_chi2[1]
    gs.optimize(5)
    alone = slam(g["poses"])
    alone.optimize(10)
    print(f"{name}: optimum {chi_opt:.9g}, chordal {chi_init:.6g}, chordal + 5 GN {gs.last_chi2[-1]:.9g}, 10 GN alone {alone.last_chi2[-1]:.3e}")
    assert gs.last_status == 0
    np.testing.assert_allclose(gs.last_chi2[-1], chi_opt, rtol=CC.CHI_FINAL_RTOL)
    assert not alone.last_chi2[-1] <= 100 * chi_opt


def test_graphslam_typed_graph_goes_through_its_kinds(ctx):
    g = CC.case("mixed257")
    pg = PoseGraph(np.arange(len(g["poses"])), *CC.args(g), vertex_kind=g["vk"], edge_kind=g["ek"])
    gs = GraphSLAM(pg, ctx=ctx)
    gs.initializeChordal("rt")
    ref = CC.reference("mixed257", 3)
    dp, da = RC.differences(gs.graph.poses, ref["poses"])
    assert gs.last_status == 0 and dp <= CC.POS_ATOL and da <= CC.ANG_ATOL
    assert gs.last_init_counts.tolist() == ref["counts"].tolist()


def test_initial_guess_equals_the_oracle(ctx, oracle):
    """Context.initial_guess and GraphSLAM.computeInitialGuess: the oracle's spanning-tree guess, bit for bit."""
    g = synth.make_pose_graph(300, 1000, seed=11)
    start = CC.case("pg300_scrambled")["poses"]
    want = oracle.initial_guess(start, g["fixed"], g["edge_from"], g["edge_to"], g["meas"])
    got = ctx.initial_guess(start, g["fixed"], g["edge_from"], g["edge_to"], g["meas"])
    np.testing.assert_array_equal(got, want)
    pg = PoseGraph.from_synth(g)
    pg.poses[:] = start
    gs = GraphSLAM(pg, ctx=ctx)
    gs.computeInitialGuess()
    np.testing.assert_array_equal(gs.graph.poses, want)
