"""Dogleg (cgmr_dl_optimize): the float64 reference of the contract (tests/ref_dogleg.py) on hand-derived and calibrated
cases, and the entry points as the header, the library and the Python layers declare them; no GPU needed.
tests/test_dogleg_gpu.py checks the device against the same reference."""
import os
import re

import numpy as np
import pytest

import ref_dogleg
from cg_mrslam_amd import _lib
from cg_mrslam_amd.condensed import RobotGraph
from cg_mrslam_amd.graph import GraphSLAM
from test_lm_cpu import args, indefinite_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# v0 fixed at the origin, v1 free, z = (1, 0, 0): the error is e = x1 - z exactly, Jj = I, H = Omega, b = -Omega e
W = np.array([4.0, 9.0, 25.0])
POSES = np.array([[0.0, 0.0, 0.0], [1.5, 0.2, 0.1]])
FIXED = np.array([1, 0], np.uint8)
EF, ET = np.array([0]), np.array([1])
MEAS = np.array([[1.0, 0.0, 0.0]])
INFO = np.array([[W[0], 0, 0, W[1], 0, W[2]]])
E = POSES[1] - MEAS[0]
B = -W * E
HGN = -E                                                     # H hgn = b
ALPHA = float(B @ B) / float(B @ (W * B))
HSD = ALPHA * B


def two(iters=1, **kw):
    return ref_dogleg.dl_optimize(POSES, FIXED, EF, ET, MEAS, INFO, iters, **kw)


# ---------------------------------------------------------------------------------------------- hand-derived
def test_alpha_by_hand():
    r = two()
    t = r["trace"][0]
    assert t["alpha"] == pytest.approx(ALPHA, rel=1e-15)
    assert ALPHA == pytest.approx(float(np.sum(B * B)) / float(np.sum(W * B * B)), rel=1e-15)
    assert t["hsd_norm"] == pytest.approx(float(np.linalg.norm(HSD)), rel=1e-15)
    assert t["hgn_norm"] == pytest.approx(float(np.linalg.norm(E)), rel=1e-15)


def test_default_delta_takes_the_gauss_newton_step():
    r = two()
    t = r["trace"][0]
    assert t["step"] == ref_dogleg.STEP_GN and t["accept"]
    assert t["rho"] == pytest.approx(1.0, rel=1e-12)            # a linear error: the model is exact
    assert r["deltas"].tolist() == [1e4]                     # rho > 0.75: max(delta, 3 |h|) = delta
    assert r["steps"].tolist() == [ref_dogleg.STEP_GN] and r["trials"].tolist() == [1]
    assert np.allclose(r["poses"][1], MEAS[0], rtol=0, atol=1e-15)
    assert r["chi2"][1] <= 1e-28 and r["iters_done"] == 1 and not r["terminated"]


def test_small_delta_takes_a_steepest_descent_step_of_length_delta():
    d = 0.5 * float(np.linalg.norm(HSD))
    r = two(initial_delta=d)
    t = r["trace"][0]
    assert t["step"] == ref_dogleg.STEP_SD and t["h_norm"] == pytest.approx(d, rel=1e-14)
    h = r["poses"][1] - POSES[1]
    assert np.allclose(h, d * B / np.linalg.norm(B), rtol=0, atol=1e-14)   # along b
    lin = -float(h @ (W * h)) + 2 * float(B @ h)
    assert t["lin_gain"] == pytest.approx(lin, rel=1e-12)
    assert t["rho"] == pytest.approx(1.0, rel=1e-12) and r["deltas"][0] == pytest.approx(max(d, 3 * d), rel=1e-14)


def test_delta_between_the_norms_takes_a_dogleg_step_of_length_delta():
    nsd, ngn = float(np.linalg.norm(HSD)), float(np.linalg.norm(HGN))
    assert nsd < ngn
    d = 0.5 * (nsd + ngn)
    r = two(initial_delta=d)
    t = r["trace"][0]
    assert t["step"] == ref_dogleg.STEP_DL
    a = HGN - HSD
    c = float(HSD @ a)
    beta = (-c + np.sqrt(c * c + (a @ a) * (d * d - HSD @ HSD))) / (a @ a) if c <= 0 else \
        (d * d - HSD @ HSD) / (c + np.sqrt(c * c + (a @ a) * (d * d - HSD @ HSD)))
    assert 0 < beta < 1
    h = r["poses"][1] - POSES[1]
    assert np.allclose(h, HSD + beta * a, rtol=0, atol=1e-14)
    assert float(np.linalg.norm(h)) == pytest.approx(d, rel=1e-12) and t["h_norm"] == pytest.approx(d, rel=1e-12)


# ---------------------------------------------------------------------------------------------- damping, Fail
def test_indefinite_graph_runs_the_damping_loop():
    g = indefinite_graph()
    r = ref_dogleg.dl_optimize(*args(g), 3)
    assert r["failed"] is None and r["iters_done"] == 3 and not r["terminated"]
    # iteration 0: the undamped factorisation fails, then H + lambda I for 1e-6 .. 1e1 fails, 1e2 works (-> 1e2 / 5);
    # iteration 1: 20 fails, 200 works (-> 40); iteration 2: 40 fails, 400 works (-> 80)
    want = [1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e0, 1e1, 1e2, 2e1, 2e2, 4e1, 4e2, 8e1]
    assert np.allclose(r["lambdas"], want, rtol=1e-12, atol=0)
    assert np.all(np.diff(r["chi2"]) < 0)


def test_indefinite_past_the_largest_lambda_fails():
    g = indefinite_graph()
    info = g["info"].copy()
    info[40] = [-1e5, 0, 0, info[40][3], 0, info[40][5]]
    r = ref_dogleg.dl_optimize(g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], info, 3)
    assert r["failed"] == 0 and r["iters_done"] == 0 and r["lambdas"][-1] == 1e3
    # 1e-6 .. 1e3 all fail; 1e4 is above the largest lambda: clamped to 1e3, Fail
    assert np.allclose(r["lambdas"], [10.0 ** k for k in range(-6, 4)] + [1e3], rtol=1e-12, atol=0)
    assert np.array_equal(r["poses"], g["poses"]) and np.all(r["chi2"] == r["chi2"][0])


# ---------------------------------------------------------------------------------------------- termination
def test_an_accepted_step_on_the_last_allowed_trial_still_terminates():
    # g2o's quirk: numTries == max_trials terminates even after a good step.  With max_trials = 1 the GN step is accepted on
    # the only trial of iteration 0, and the call ends there.
    r = two(iters=3, max_trials=1)
    assert r["trace"][0]["accept"] and r["trials"].tolist() == [1]
    assert r["iters_done"] == 1 and r["terminated"]
    assert np.allclose(r["poses"][1], MEAS[0], rtol=0, atol=1e-15)
    assert r["chi2"][1] == r["chi2"][2] == r["chi2"][3]


def test_graph_at_its_optimum():
    p = POSES.copy()
    p[1] = MEAS[0]                                           # e = 0 exactly: b = 0, alpha = 0/0
    r = ref_dogleg.dl_optimize(p, FIXED, EF, ET, MEAS, INFO, 4, max_trials=7)
    assert np.isnan(r["trace"][0]["alpha"]) and np.isnan(r["trace"][0]["hsd_norm"])
    assert all(t["step"] == ref_dogleg.STEP_GN and t["rho"] == 0 and not t["accept"] for t in r["trace"])
    assert r["iters_done"] == 1 and r["terminated"] and r["trials"].tolist() == [7]
    assert r["deltas"].tolist() == [1e4 * 0.5 ** 7]
    assert np.array_equal(r["poses"], p) and np.all(r["chi2"] == 0)


def test_nothing_free_and_no_iterations():
    r = ref_dogleg.dl_optimize(POSES, np.array([1, 1], np.uint8), EF, ET, MEAS, INFO, 3)
    assert r["iters_done"] == 1 and r["terminated"] and r["trials"].tolist() == [100] and r["steps"].tolist() == [2]
    assert r["deltas"].tolist() == [1e4 * 0.5 ** 100] and np.all(r["chi2"] == r["chi2"][0])
    r = two(iters=0)
    assert r["iters_done"] == 0 and len(r["chi2"]) == 1 and not r["terminated"]


def test_bad_start_never_rises():
    from test_lm_cpu import bad_start_graph
    g = bad_start_graph()
    r = ref_dogleg.dl_optimize(*args(g), 10)
    assert r["iters_done"] == 10 and np.all(np.diff(r["chi2"]) <= 0)
    assert r["trials"][0] > 1 and any(not t["accept"] for t in r["trace"])


# ---------------------------------------------------------------------------------------------- declarations
def _prototype(name):
    txt = open(os.path.join(ROOT, "include", "cgmr.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/cgmr.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_dogleg_entry_points():
    for name in ("cgmr_dl_optimize", "cgmr_dl_optimize_dev"):
        a = _prototype(name)
        assert len(a) == 17, a
        assert a[10].startswith("const cgmr_dl_params*") and a[11].startswith("double*") and a[12].startswith("double*")
        assert a[13].startswith("int32_t*") and a[14].startswith("int32_t*") and a[15].startswith("int32_t*")
        assert a[16].startswith("const cgmr_robust*")
    assert _prototype("cgmr_dl_last_stats") == ["const cgmr_ctx* ctx", "int64_t out[3]"]
    assert len(_prototype("cgmr_graph_set_dogleg_params")) == 2
    assert len(_prototype("cgmr_graph_dl_last")) == 5
    txt = open(os.path.join(ROOT, "include", "cgmr.h")).read()
    assert re.search(r"#define\s+CGMR_ALG_DOGLEG\s+2\b", txt)
    for k, v in (("SD", 1), ("GN", 2), ("DL", 3)):
        assert re.search(r"#define\s+CGMR_DL_STEP_%s\s+%d\b" % (k, v), txt)
    m = re.search(r"typedef struct cgmr_dl_params \{([^}]*)\}", txt)
    fields = re.findall(r"(\w+)\s*;", m.group(1))
    assert fields == [f for f, _ in _lib.DlParams._fields_]
    assert "g2o-recalled" in txt[txt.index("Dogleg optimisation"):txt.index("typedef struct cgmr_dl_params")]


def test_library_exports_the_dogleg_entry_points_and_keeps_version_105():
    lib = _lib.load_library()
    for name in ("cgmr_dl_optimize", "cgmr_dl_optimize_dev", "cgmr_dl_last_stats", "cgmr_graph_set_dogleg_params",
                 "cgmr_graph_dl_last"):
        assert hasattr(lib, name), name
    assert lib.cgmr_version() == 105


def test_python_layers_expose_dogleg_and_reject_bad_parameters():
    for name in ("dl_optimize", "dl_optimize_dev", "dl_last_stats"):
        assert callable(getattr(_lib.Context, name, None)), name
    assert callable(getattr(RobotGraph, "dl_last", None))
    assert callable(getattr(GraphSLAM, "trustRegion", None)) and callable(getattr(GraphSLAM, "lastStep", None))
    p = _lib.dl_params(max_trials=3)
    assert (p.initial_delta, p.max_trials, p.initial_lambda, p.lambda_factor) == (1e4, 3, 1e-7, 10.0)
    with pytest.raises(TypeError):
        _lib.dl_params(radius=1.0)
    for bad in (dict(max_trials=0), dict(initial_delta=0.0), dict(initial_delta=float("inf")), dict(initial_lambda=-1.0),
                dict(lambda_factor=1.0), dict(lambda_factor=float("nan"))):
        with pytest.raises(ValueError):
            _lib.dl_params_checked(bad)
        with pytest.raises(ValueError):
            GraphSLAM(None, None, algorithm="dl", dl_params=bad)
    with pytest.raises(TypeError):
        GraphSLAM(None, None, algorithm="dl", dl_params=dict(radius=1.0))
    with pytest.raises(ValueError):
        GraphSLAM(None, None, algorithm="dogleg")               # g2o's factory prefix only
