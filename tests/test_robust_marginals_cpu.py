"""Robust kernels in the marginals and the condensed graphs, without a GPU: the declarations and exports, the argument checks
before any device call, and the float64 contract of tests/ref_robust_marginals.py (a hand-derived case, the outlier recipe)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import ref_numpy as R
import ref_robust as RR
import ref_robust_marginals as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cgmr_marginals_robust": 13, "cgmr_marginals_all_robust": 12, "cgmr_covariance_estimate_robust": 13,
       "cgmr_condense_robust": 16, "cgmr_graph_set_condensed_robust": 2}


def _prototype_args(txt, fn):
    m = re.search(r"\bint " + fn + r"\(([^;]*)\);", txt)
    assert m, fn
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_entry_points_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "cgmr.h")).read()
    for fn, n in NEW.items():
        assert _prototype_args(txt, fn) == n, fn
        assert txt.count("int " + fn + "(") == 1, fn
    for fn in ("marginals", "marginals_all", "covariance_estimate", "condense"):      # each: the plain prototype + the cgmr_robust
        assert _prototype_args(txt, f"cgmr_{fn}_robust") == _prototype_args(txt, f"cgmr_{fn}") + 1
        assert re.search(r"const cgmr_robust\* rk\);", re.search(r"\bint cgmr_" + fn + r"_robust\([^;]*;", txt).group(0))
    assert "Out of scope: the marginals" not in txt
    from cg_mrslam_amd import _lib
    lib = _lib.load_library()
    assert lib.cgmr_version() == 105
    for fn in NEW:
        assert hasattr(lib, fn), fn
    from cg_mrslam_amd.condensed import RobotGraph
    from cg_mrslam_amd.graph import GraphSLAM
    assert "robust" in inspect.signature(GraphSLAM.computeMarginals).parameters
    assert inspect.signature(GraphSLAM.computeMarginals).parameters["robust"].default is False
    assert callable(getattr(RobotGraph, "set_condensed_robust", None))
    for m in ("marginals_robust", "marginals_all_robust", "covariance_estimate_robust", "condense_robust"):
        assert callable(getattr(_lib.Context, m, None)), m


def test_bad_kernels_and_a_missing_context_are_rejected_without_a_device():
    from cg_mrslam_amd import _lib
    lib = _lib.load_library()
    E_INVALID = lib.cgmr_match_last_stats(None, (C.c_int64 * 4)())
    assert E_INVALID < 0
    poses = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    fixed = np.array([1, 0], np.uint8)
    ef, et = np.array([0], np.int32), np.array([1], np.int32)
    meas, info = np.array([[1.0, 0, 0]]), np.array([[1.0, 0, 0, 1, 0, 1]])
    q = np.array([1], np.int32)
    out = np.zeros(64)
    to = np.zeros(4, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)                                          # noqa: E731
    for kind, delta in ((9, 1.0), (1, 0.0), (3, -2.0), (2, float("nan")), (0, 1.0)):
        rk = _lib.Robust(None, None, kind, delta, None, None)
        assert lib.cgmr_marginals_robust(None, 2, p(poses), p(fixed), 1, p(ef), p(et), p(meas), p(info), 1, p(q), p(out),
                                         C.byref(rk)) == E_INVALID
        assert lib.cgmr_marginals_all_robust(None, 2, p(poses), p(fixed), 1, p(ef), p(et), p(meas), p(info), p(out), None,
                                             C.byref(rk)) == E_INVALID
        assert lib.cgmr_covariance_estimate_robust(None, 2, p(poses), 1, p(ef), p(et), p(meas), p(info), 0, 1, p(q), p(out),
                                                   C.byref(rk)) == E_INVALID
        assert lib.cgmr_condense_robust(None, 2, p(poses), 1, p(ef), p(et), p(meas), p(info), 0, 1, p(q), p(to), p(out), p(out),
                                        None, C.byref(rk)) == E_INVALID
    assert lib.cgmr_graph_set_condensed_robust(None, 1) == E_INVALID

    class NoDevice:                                                                 # any library call would fail loudly
        def __getattr__(self, name):
            raise AssertionError(f"device call {name} reached")

    ctx = _lib.Context.__new__(_lib.Context)
    ctx.lib, ctx.h = NoDevice(), None
    for kind, delta in (("Fair", 1.0), ("huber", 0.0), (np.array([1], np.uint8), np.array([np.inf]))):
        with pytest.raises(ValueError):
            ctx.marginals_robust(poses, fixed, ef, et, meas, info, q, kind, delta)
        with pytest.raises(ValueError):
            ctx.marginals_all_robust(poses, fixed, ef, et, meas, info, False, kind, delta)
        with pytest.raises(ValueError):
            ctx.covariance_estimate_robust(poses, ef, et, meas, info, 0, q, kind, delta)
        with pytest.raises(ValueError):
            ctx.condense_robust(poses, ef, et, meas, info, 0, q, kind, delta)


def test_two_vertex_huber_covariance_doubles():
    """x0 fixed, one edge with information diag(4, 9, 16) measuring (1, 0, 0), x1 at (1 + delta, 0, 0): e = (delta, 0, 0) and
    e2 = 4 delta^2, so Huber's weight is delta / sqrt(e2) = 1/2, H halves and the covariance of x1 doubles."""
    delta = 0.75
    poses = np.array([[0.0, 0, 0], [1.0 + delta, 0, 0]])
    fixed = np.array([1, 0], np.uint8)
    ef, et = np.array([0], np.int32), np.array([1], np.int32)
    meas, info = np.array([[1.0, 0, 0]]), np.array([[4.0, 0, 0, 9.0, 0, 16.0]])
    assert RR.edge_chi2(poses, ef, et, meas, info)[0] == pytest.approx(4 * delta * delta, rel=1e-15)
    rob, _, w = RM.marginals(poses, fixed, ef, et, meas, info, 1, delta, [0, 1])
    plain, _, w0 = RM.marginals(poses, fixed, ef, et, meas, info, 0, 1.0, [0, 1])
    assert w[0] == pytest.approx(0.5, rel=1e-15) and w0[0] == 1.0
    assert np.all(rob[0] == 0) and np.all(plain[0] == 0)        # the fixed vertex
    np.testing.assert_allclose(rob[1], 2 * plain[1], rtol=1e-14, atol=0)
    np.testing.assert_allclose(np.diag(plain[1]), [1 / 4.0, 1 / 9.0, 1 / 16.0], rtol=1e-14)   # (J = -I at x0 = 0)


# ---------------------------------------------------------------------------------------------- the outlier recipe
_OUT = {}


def outlier_optimum():
    """ref_robust.outlier_graph at its Cauchy(3) optimum (ten robust Gauss-Newton iterations in numpy)."""
    if not _OUT:
        g, bad, _ = RR.outlier_graph()
        a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
        x, _, _, failed = RR.gn_optimize(*a, 3, 3.0, 10)
        assert failed is None
        _OUT.update(g=g, bad=bad, x=x)
    return _OUT


# Measured in float64 on this recipe (Cauchy, delta 3): the robust marginals of the first ten corrupted closures' end vertices
# have 1.0032 .. 1.0075 times the plain trace; the condensed information across each of the first four corrupted closures
# (gauge vertex 0, both end vertices queried) 0.73 .. 0.936 times the plain trace.  Pinned with margin.
MARG_TRACE_MIN = 1.001
COND_TRACE_MAX = 0.97


def test_outlier_marginals_grow_at_the_corrupted_closures():
    o = outlier_optimum()
    g, bad, x = o["g"], o["bad"], o["x"]
    ef, et = g["edge_from"], g["edge_to"]
    ends = np.unique(np.r_[ef[bad[:10]], et[bad[:10]]])
    rob, err, w = RM.marginals(x, g["fixed"], ef, et, g["meas"], g["info"], 3, 3.0, ends)
    plain, err0, _ = RM.marginals(x, g["fixed"], ef, et, g["meas"], g["info"], 0, 1.0, ends)
    assert err.max() <= 1e-10 and err0.max() <= 1e-10
    assert w[bad].max() < 1e-3                                  # (rejected at the optimum)
    ratio = np.trace(rob, axis1=1, axis2=2) / np.trace(plain, axis1=1, axis2=2)
    print(f"robust / plain marginal trace at the corrupted closures' ends: {ratio.min():.4f} .. {ratio.max():.4f}")
    assert ratio.min() >= MARG_TRACE_MIN


def test_outlier_condensed_information_shrinks_across_the_corrupted_closures():
    """The condensed weights come from the spanning-tree guess from the gauge, not from the optimum: a corrupted closure can be
    a tree edge there (weight 1), yet the edges it bends are down-weighted and the star edge across it still loses information."""
    o = outlier_optimum()
    g, bad, x = o["g"], o["bad"], o["x"]
    ef, et = g["edge_from"], g["edge_to"]
    a = (ef, et, g["meas"], g["info"])
    worst = 0.0
    for b in bad[:4]:
        q = np.array([0, ef[b], et[b]], np.int32)
        rob = RM.condense(x, *a, 3, 3.0, 0, q, RM.guess_bfs)
        plain = RM.condense(x, *a, 0, 1.0, 0, q, RM.guess_bfs)
        assert np.array_equal(rob["to"], plain["to"]) and not rob["not_pd"].any()
        assert rob["cov_err"].max() <= 1e-10
        assert np.sum(rob["weights"] >= 1 - 1e-12) >= len(x) - 1  # (the tree edges, and any other edge the guess closes exactly)
        for k in range(len(rob["to"])):
            r = np.trace(R.info_full(rob["iu"])[k]) / np.trace(R.info_full(plain["iu"])[k])
            worst = max(worst, r)
    print(f"largest robust / plain condensed information trace across a corrupted closure: {worst:.4f}")
    assert worst <= COND_TRACE_MAX
