"""Robust kernels without a GPU: the contract of tests/ref_robust.py (include/cgmr.h, cgmr_robust) against derivatives, hand
values and a hand-derived two-vertex case, the outlier recipe in numpy, the declarations and the Python checks."""
import os
import re

import numpy as np
import pytest

import ref_numpy as R
import ref_robust as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH = {"huber": 1, "pseudohuber": 2, "cauchy": 3, "welsch": 4, "tukey": 5}


@pytest.mark.parametrize("name", sorted(SMOOTH))
def test_rho1_is_the_derivative_of_rho0(name):
    kind, delta = SMOOTH[name], 1.7
    e2 = np.concatenate([np.linspace(0.05, 2.8, 25), np.linspace(3.0, 40.0, 25)])   # (Tukey: both sides of delta^2 = 2.89)
    e2 = e2[np.abs(e2 - delta * delta) > 1e-3]
    h = 1e-6 * np.maximum(e2, 1.0)
    fd = (RR.rho(kind, delta, e2 + h)[0] - RR.rho(kind, delta, e2 - h)[0]) / (2 * h)
    np.testing.assert_allclose(RR.rho(kind, delta, e2)[1], fd, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("name", ["huber", "tukey", "saturated", "dcs"])
def test_rho_is_continuous_at_the_threshold(name):
    kind = RR.KINDS[name]
    delta = 2.5
    t = delta * delta if name != "dcs" else delta            # DCS: s = 1 at e2 = phi
    lo, hi = RR.rho(kind, delta, np.nextafter(t, 0)), RR.rho(kind, delta, np.nextafter(t, np.inf))
    np.testing.assert_allclose(lo[0], hi[0], rtol=1e-12)
    if name in ("huber", "tukey", "dcs"):
        np.testing.assert_allclose(lo[1], hi[1], rtol=1e-12, atol=1e-12)


def test_dcs_and_saturated_hand_values():
    # DCS, phi = 2: e2 = 1 -> s = 4/3 >= 1: (1, 1); e2 = 6 -> s = 0.5: (0.25 * 6, 0.25)
    r0, r1 = RR.rho(7, 2.0, np.array([1.0, 6.0]))
    np.testing.assert_array_equal(r0, [1.0, 1.5])
    np.testing.assert_array_equal(r1, [1.0, 0.25])
    # Saturated, delta = 3: e2 = 4 -> (4, 1); e2 = 16 -> (9, 0)
    r0, r1 = RR.rho(6, 3.0, np.array([4.0, 16.0]))
    np.testing.assert_array_equal(r0, [4.0, 9.0])
    np.testing.assert_array_equal(r1, [1.0, 0.0])
    # none: (e2, 1) whatever delta
    r0, r1 = RR.rho(0, -1.0, np.array([0.0, 7.0]))
    np.testing.assert_array_equal(r0, [0.0, 7.0])
    np.testing.assert_array_equal(r1, [1.0, 1.0])


def test_two_vertex_huber_edge_beyond_delta():
    """x0 fixed at the origin, x1 at (3, 0, 0), one edge measuring (1, 0, 0) with identity information: e = (2, 0, 0),
    e2 = 4 > delta^2 = 1, so the weight is delta / sqrt(e2) = 1/2, H = 1/2 I, b = -(1/2) (2, 0, 0) and the step is -2 in x:
    the full step to the measurement, as for the plain edge (a single edge: the weight cancels)."""
    poses = np.array([[0.0, 0, 0], [3.0, 0, 0]])
    fixed = np.array([1, 0], dtype=np.uint8)
    ef, et = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    meas = np.array([[1.0, 0, 0]])
    info = np.array([[1.0, 0, 0, 1.0, 0, 1.0]])
    w = RR.weights(poses, ef, et, meas, info, 1, 1.0)
    assert w[0] == 0.5
    assert RR.robust_chi2(poses, ef, et, meas, info, 1, 1.0) == 2 * 2 * 1 - 1
    H, b, _ = R.build_system(poses, fixed, ef, et, meas, info * w[:, None])
    np.testing.assert_array_equal(H.toarray(), 0.5 * np.eye(3))
    np.testing.assert_array_equal(b, [-1.0, 0, 0])
    x, chi, _, failed = RR.gn_optimize(poses, fixed, ef, et, meas, info, 1, 1.0, 1)
    assert failed is None
    np.testing.assert_allclose(x[1], [1.0, 0, 0], atol=1e-15)
    assert chi[0] == 3.0 and chi[1] < 1e-28


def test_outlier_recipe_in_numpy():
    """The ordering the robust kernels are for: plain Gauss-Newton is pulled metres away by 1 % corrupted closures, Cauchy(3)
    stays within 0.2 m of the clean optimum and weighs every corrupted closure down.  Measured here: plain 19.2 m, Cauchy
    0.114 m, corrupted weights <= 2.7e-4, 98.1 % of the clean weights > 0.5."""
    g, bad, _ = RR.outlier_graph()
    a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
    clean = RR.clean_optimum(g, bad)
    plain, _ = R.gn_optimize(*a, 10)
    assert RR.rms(plain, clean) > 2.0
    x, chi, _, failed = RR.gn_optimize(*a, 3, 3.0, 10)
    assert failed is None and chi[-1] < chi[0]
    assert RR.rms(x, clean) < 0.2
    w = RR.weights(x, g["edge_from"], g["edge_to"], g["meas"], g["info"], 3, 3.0)
    good = np.ones(len(w), dtype=bool)
    good[bad] = False
    assert w[bad].max() < 1e-3
    assert (w[good] > 0.5).mean() >= 0.95


def test_header_declares_the_robust_abi():
    txt = open(os.path.join(ROOT, "include", "cgmr.h")).read()
    codes = dict(re.findall(r"#define CGMR_RK_([A-Z_]+) (\d+)", txt))
    assert codes == {"NONE": "0", "HUBER": "1", "PSEUDO_HUBER": "2", "CAUCHY": "3", "WELSCH": "4", "TUKEY": "5",
                     "SATURATED": "6", "DCS": "7"}
    for fn in ("cgmr_gn_optimize_robust", "cgmr_gn_optimize_robust_dev", "cgmr_lm_optimize_robust", "cgmr_lm_optimize_robust_dev",
               "cgmr_graph_set_edge_robust", "cgmr_graph_set_received_robust", "cgmr_graph_edge_stats"):
        assert re.search(r"\bint " + fn + r"\(", txt), fn
    assert "typedef struct cgmr_robust" in txt and "Fair" in txt and "GemanMcClure" in txt
    src = open(os.path.join(ROOT, "cg_mrslam_amd", "csrc", "cgmr_api.cpp")).read()
    assert re.search(r"int cgmr_version\(void\) \{ return 105; \}", src)


def test_python_checks_names_and_deltas():
    from cg_mrslam_amd import _lib
    assert _lib.robust_code("Cauchy") == 3 and _lib.robust_code("PseudoHuber") == 2 and _lib.robust_code("RobustKernelDCS") == 7
    assert _lib.robust_code(0) == 0
    for bad in ("GemanMcClure", "Fair", "cauchyy", 8, -1, 2.5, True):
        with pytest.raises(ValueError):
            _lib.robust_code(bad)
    for d in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            _lib.robust_arrays("huber", d, 3)
    _lib.robust_arrays("none", 0.0, 3)                              # (no delta needed)
    with pytest.raises(ValueError):
        _lib.robust_arrays(["huber", "none"], 1.0, 3)               # one kind per edge
    with pytest.raises(ValueError):
        _lib.robust_arrays(np.array([1, 0, 3]), np.array([1.0, 0.0, -2.0]), 3)   # edge 2: Cauchy with delta -2
    codes, deltas, _, _ = _lib.robust_arrays(np.array([1, 0, 3]), np.array([1.0, 0.0, 2.0]), 3)
    assert codes.tolist() == [1, 0, 3] and deltas.tolist() == [1.0, 0.0, 2.0]


def test_graphslam_rejects_bad_kernels_before_the_device():
    from cg_mrslam_amd import synth
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph

    class NoDevice:                                                 # any device call would fail loudly
        def __getattr__(self, name):
            raise AssertionError(f"device call {name} reached")

    gs = GraphSLAM(PoseGraph.from_synth(synth.make_pose_graph(20, 40, seed=3)), ctx=NoDevice())
    with pytest.raises(ValueError):
        gs.setRobustKernel("Fair", 1.0)
    with pytest.raises(ValueError):
        gs.setRobustKernel("Huber", 0.0)
    with pytest.raises(ValueError):
        gs.setRobustKernel("Huber", 1.0, edges=[gs.graph.n_edges])
    gs.setRobustKernel("Huber", 1.0, edges=[0, 5])
    assert gs._rk_kind.tolist().count(1) == 2
    gs.clearRobustKernels()
    assert gs._robust_level0() is None
