"""The graduated non-convexity contract (tests/ref_gnc.py) pinned without a GPU: a hand-worked answer, the weights at the ends
of the TLS band, "nothing to reject", the reach predicates of every case of tests/gnc_cases.py -- the reference ALONE must
reject exactly the corrupted edges and stay clear of every branch -- and the interface."""
import math
import re

import numpy as np
import pytest

import gnc_cases as GC
import ref_gnc
import ref_typed
from cg_mrslam_amd import _lib
from cg_mrslam_amd.graph import GraphSLAM


# ------------------------------------------------------------------------------------------------ the hand-worked answer
def test_hand_worked_answer():
    g = GC.case("hand")
    assert g["mu0"] == 1.0 / 17.0 and g["w_first"][2] == pytest.approx((math.sqrt(2.0) - 1.0) / 17.0, rel=1e-15)
    res = GC.reference("hand", "tls")
    assert res["mu"][0] == pytest.approx(g["mu0"], rel=1e-15)
    np.testing.assert_allclose(res["trace"][0]["r"], [0.0, 0.0, 9.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(res["trace"][0]["w"], g["w_first"], rtol=1e-14, atol=0)
    assert res["weights"].tolist() == g["w_final"].tolist()
    assert res["partial"][res["outer_done"] - 1] == 0 and res["partial"][0] == 1
    np.testing.assert_allclose(res["poses"][1], [1.0, 0.0, 0.0], rtol=0, atol=1e-12)
    # mu grows by the factor, one multiplication per step
    mu = res["mu"][:res["outer_done"]]
    assert all(mu[k + 1] == mu[k] * 1.4 for k in range(len(mu) - 1))
    # behind outer_done: zeros, the cost repeats sum w r at the end
    assert np.all(res["mu"][res["outer_done"]:] == 0) and np.all(res["partial"][res["outer_done"]:] == 0)
    assert np.all(res["cost"][res["outer_done"]:] == float(np.sum(res["weights"] * res["edge_chi2"])))


# ------------------------------------------------------------------------------------------------ the ends of the band
@pytest.mark.parametrize("mu", [1.0 / 17.0, 0.5, 1.0, 3.7, 1e3])
@pytest.mark.parametrize("c", [1.0, 9.21034037197618, 21.1])
def test_band_edge_weights(mu, c):
    lo, up = ref_gnc.band(ref_gnc.TLS, mu, np.array([c]))
    known = np.zeros(1, np.uint8)
    assert ref_gnc.weights(ref_gnc.TLS, mu, np.array([c]), lo, known)[0] == 1.0
    assert ref_gnc.weights(ref_gnc.TLS, mu, np.array([c]), up, known)[0] == 0.0
    assert ref_gnc.weights(ref_gnc.TLS, mu, np.array([c]), np.array([0.0]), known)[0] == 1.0
    mid = ref_gnc.weights(ref_gnc.TLS, mu, np.array([c]), 0.5 * (lo + up), known)[0]
    assert 0.0 < mid < 1.0
    # just inside the band the formula joins the ends: w(lo) = 1 and w(up) = 0 up to rounding
    assert math.sqrt(c * mu * (mu + 1.0) / lo[0]) - mu == pytest.approx(1.0, abs=1e-12 * (1 + mu))
    assert math.sqrt(c * mu * (mu + 1.0) / up[0]) - mu == pytest.approx(0.0, abs=1e-12 * (1 + mu))
    # a known inlier: 1 whatever r
    assert ref_gnc.weights(ref_gnc.TLS, mu, np.array([c]), 10 * up, np.ones(1, np.uint8))[0] == 1.0


def test_gm_weight_at_mu_one():
    c = np.array([4.0, 4.0, 4.0])
    w = ref_gnc.weights(ref_gnc.GM, 1.0, c, np.array([0.0, 4.0, 12.0]), np.zeros(3, np.uint8))
    assert w.tolist() == [1.0, 0.25, 0.0625]                     # (c / (r + c))^2


def test_start_values():
    c, known = np.array([2.0, 2.0, 2.0]), np.array([0, 0, 1], np.uint8)
    assert ref_gnc.mu_start(ref_gnc.TLS, c, np.array([0.9, 5.0, 100.0]), known) == (2.0 / 8.0, False)   # (the known edge does not count)
    assert ref_gnc.mu_start(ref_gnc.TLS, c, np.array([0.9, 1.0, 100.0]), known) == (0.0, True)          # 2 r - c <= 0 everywhere
    assert ref_gnc.mu_start(ref_gnc.GM, c, np.array([0.9, 5.0, 100.0]), known) == (5.0, False)
    assert ref_gnc.mu_start(ref_gnc.GM, c, np.array([0.9, 1.0, 100.0]), known) == (0.0, True)           # mu0 = 1: nothing
    assert ref_gnc.mu_start(ref_gnc.GM, c, np.array([9.0, 9.0, 9.0]), np.ones(3, np.uint8)) == (0.0, True)   # F empty
    assert ref_gnc.default_barc_sq(np.array([0, 1, 2, 3, 4]), 5).tolist() == [11.344866730144373, 9.21034037197618, 6.634896601021213,
                                                                             11.344866730144373, 9.21034037197618]


# ------------------------------------------------------------------------------------------------ nothing to reject
@pytest.mark.parametrize("name", ["clean", "clean_typed"])
@pytest.mark.parametrize("loss", ["tls", "gm"])
def test_nothing_to_reject_is_plain_gauss_newton(name, loss):
    g = GC.case(name)
    res = GC.reference(name, loss)
    assert res["nothing"] and res["outer_done"] == 1 and res["mu"][0] == 0.0 and res["partial"][0] == 0
    assert np.all(res["weights"] == 1.0)
    p, _, _ = ref_typed.gn_optimize(*GC.args(g), g["inner_iters"], g["vk"], g["ek"])
    assert np.array_equal(res["poses"], p)


# ------------------------------------------------------------------------------------------------ reach predicates
@pytest.mark.parametrize("name", GC.REJECTING)
def test_tls_rejects_exactly_the_corrupted_edges_clear_of_every_branch(name):
    g = GC.case(name)
    res = GC.reference(name, "tls")
    assert res["failed"] is None and res["outer_done"] < 100
    assert np.array_equal(np.flatnonzero(res["weights"] == 0.0), g["bad"]), name
    assert np.all(res["weights"][np.setdiff1d(np.arange(len(res["weights"])), g["bad"])] == 1.0)
    assert ref_gnc.margins(res) > GC.MARGIN, (name, ref_gnc.margins(res))
    assert res["partial"][res["outer_done"] - 1] == 0 and np.all(res["partial"][:res["outer_done"] - 1] > 0)


@pytest.mark.parametrize("name", GC.GM_CASES)
def test_gm_leaves_the_corrupted_edges_no_weight(name):
    g = GC.case(name)
    res = GC.reference(name, "gm")
    assert res["failed"] is None and res["mu"][res["outer_done"] - 1] == 1.0
    assert float(res["weights"][g["bad"]].max()) < 1e-3, name


def test_issue_table():
    """The two cases the recipe was first run on: the iteration counts it reported."""
    assert (GC.reference("og60", "tls")["outer_done"], GC.reference("og60", "gm")["outer_done"]) == (29, 31)
    assert (GC.reference("og300", "tls")["outer_done"], GC.reference("og300", "gm")["outer_done"]) == (32, 32)
    assert (len(GC.case("og60")["bad"]), len(GC.case("og300")["bad"])) == (24, 143)
    assert (len(GC.case("og300")["edge_from"]) + 255) // 256 == 4              # mu0 folds across four workgroups


@pytest.mark.parametrize("name", GC.BOUNDARY)
def test_the_extreme_of_mu0_is_on_the_last_edge(name):
    g = GC.case(name)
    nE = len(g["ek"])
    assert nE == int(name[5:]) and g["bad"][-1] == nE - 1 and g["known"][-1] == 0 and g["ek"][-1] == 1
    r0 = GC.reference(name, "tls")["trace"][0]["r"]
    free = g["known"] == 0
    assert int(np.flatnonzero(free)[np.argmax(r0[free])]) == nE - 1
    c = GC.reference(name, "tls")["barc_sq"]
    assert GC.reference(name, "tls")["mu"][0] == c[-1] / (2.0 * r0[-1] - c[-1])
    assert GC.reference(name, "gm")["mu"][0] == 2.0 * r0[-1] / c[-1]
    assert len(g["bad"]) == int(np.sum(g["ek"] == 1)) // 10
    assert np.all(g["known"][g["ek"] != 1] == 1)                                 # priors and odometry: known inliers


def test_tree600x_reaches_the_deep_tree():
    g = GC.case("tree600x")
    info = _lib.gn_symbolic_info(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    assert len(g["ek"]) == 2500 and len(g["bad"]) == 90 and info["launch_levels"] >= 4


def test_starved_ends_singular():
    g = GC.case("starved")
    res = GC.reference("starved", "tls")
    # both observations of the lone landmark reach weight 0 together, at t = 3 (gnc_cases.starved's arithmetic)
    assert res["failed"] == 3 and res["outer_done"] == 4 and res["inner_total"] == 3
    assert res["weights"][g["bad"]].tolist() == [0.0, 0.0]
    touching = np.flatnonzero((g["edge_to"] == g["lone"]) | (g["edge_from"] == g["lone"]))
    assert np.array_equal(touching, g["bad"]) and np.all(g["known"][touching] == 0)
    assert np.array_equal(res["poses"], res["trace"][3]["x0"]) and np.all(np.isfinite(res["poses"]))
    assert ref_gnc.margins(res) > GC.MARGIN


def test_inner_iterations_keep_the_weights_frozen():
    res = GC.reference("og60", "tls", inner_iters=3)
    g = GC.case("og60")
    assert np.array_equal(np.flatnonzero(res["weights"] == 0.0), g["bad"]) and ref_gnc.margins(res) > GC.MARGIN
    assert res["inner_total"] == 3 * res["outer_done"]


def test_max_outer_cuts_the_records():
    full, cut = GC.reference("og60", "tls"), GC.reference("og60", "tls", max_outer=5)
    assert cut["outer_done"] == 5 and np.array_equal(cut["mu"], full["mu"][:5]) and np.array_equal(cut["partial"], full["partial"][:5])
    assert np.array_equal(cut["cost"][:5], full["cost"][:5]) and cut["partial"][4] > 0


# ------------------------------------------------------------------------------------------------ the interface
def _prototype(name):
    txt = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "cgmr.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_header_declares_the_gnc_entry_points():
    for name in ("cgmr_gnc_optimize", "cgmr_gnc_optimize_dev"):
        a = _prototype(name)
        assert len(a) == 15, a
        assert a[9].startswith("const cgmr_factor_types*") and a[10].startswith("const cgmr_gnc_params*")
        assert a[11].startswith("double*") and a[12].startswith("double*") and a[13].startswith("int32_t*") and a[14].startswith("int32_t*")
    assert len(_prototype("cgmr_gnc_last_stats")) == 2
    decl = _lib.declared_symbols()
    for name in ("cgmr_gnc_params_default", "cgmr_gnc_optimize", "cgmr_gnc_optimize_dev", "cgmr_gnc_last_stats"):
        assert name in decl and name in _lib._SYMBOLS, name


def test_library_exports_the_gnc_entry_points_and_keeps_version_105():
    lib = _lib.load_library()
    for name in ("cgmr_gnc_params_default", "cgmr_gnc_optimize", "cgmr_gnc_optimize_dev", "cgmr_gnc_last_stats"):
        assert hasattr(lib, name), name
    assert lib.cgmr_version() == 105
    lib.cgmr_gnc_params_default.restype = _lib.GncParams
    p = lib.cgmr_gnc_params_default()
    assert (p.loss, p.mu_factor, p.max_outer, p.inner_iters, p.outer_per_wait) == (0, 1.4, 100, 1, 8)
    assert p.barc_sq is None and p.known_inlier is None and p.weight_out is None and p.edge_chi2_out is None and p.default_barc_sq <= 0


def test_python_layers_expose_gnc():
    for name in ("gnc_optimize", "gnc_optimize_dev", "gnc_last_stats"):
        assert callable(getattr(_lib.Context, name, None)), name
    assert callable(getattr(GraphSLAM, "optimizeGNC", None)) and callable(getattr(GraphSLAM, "rejectedEdges", None))
    assert _lib.gnc_loss_code("TLS") == 0 and _lib.gnc_loss_code("gm") == 1
    with pytest.raises(ValueError):
        _lib.gnc_loss_code("huber")
    assert _lib.gnc_known_mask([0, 2], 4).tolist() == [1, 0, 1, 0]
    assert _lib.gnc_known_mask(np.array([True, False, False]), 3).tolist() == [1, 0, 0]
    assert _lib.gnc_known_mask(None, 2).tolist() == [0, 0]
