"""Chordal initialisation without a GPU: the reference (tests/ref_chordal.py) against answers worked by hand, the conditions the
GPU checks rely on, asserted on every case of tests/chordal_cases.py, and the new entry points' declarations."""
import numpy as np
import pytest

import chordal_cases as CC
import ref_chordal as RC
import ref_numpy as R
from cg_mrslam_amd import synth

INFO = [1000.0, 0.0, 0.0, 1000.0, 0.0, 10000.0]
HOWS = ("lstsq", "cholesky")


def _graph(poses, fixed, edges, ek=None):
    ef, et, meas, info = zip(*edges)
    return (np.array(poses, float), np.array(fixed, np.uint8), np.array(ef, np.int32), np.array(et, np.int32),
            np.array(meas, float).reshape(-1, 3), np.array(info, float).reshape(-1, 6)), ek


def _rot(t):
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


# ------------------------------------------------------------------------------------------------------- hand cases
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("th0,zth", [(0.3, 0.5), (2.9, 0.6), (-3.0, -0.4), (np.pi - 1e-3, 2e-3)])
def test_one_edge_from_a_fixed_pose(th0, zth, how):
    """theta_1 = normalize(theta_0 + z_theta), also beyond pi, and t_1 = t_0 + R(theta_0) z_t, whatever pose 1 starts from."""
    t0, zt = np.array([1.0, -2.0]), np.array([0.7, 0.2])
    a, _ = _graph([[*t0, th0], [9.0, 9.0, -1.0]], [1, 0], [(0, 1, [*zt, zth], INFO)])
    out = RC.initialize(*a, 3, how=how)
    assert out["counts"].tolist() == [1, 1, 0]
    assert abs(RC.wrap(out["poses"][1, 2] - (th0 + zth))) <= 1e-14
    assert -np.pi < out["poses"][1, 2] <= np.pi
    np.testing.assert_allclose(out["poses"][1, :2], t0 + _rot(th0) @ zt, rtol=0, atol=1e-13)
    np.testing.assert_array_equal(out["poses"][0], a[0][0])


@pytest.mark.parametrize("how", HOWS)
def test_two_opposite_edges_cancel(how):
    """Two equal-weight edges 0 -> 1 with z_theta = +-alpha: theta_1 = theta_0."""
    a, _ = _graph([[0.0, 0.0, 0.8], [1.0, 1.0, -2.0]], [1, 0],
                  [(0, 1, [1.0, 0.0, 0.4], INFO), (0, 1, [1.0, 0.0, -0.4], INFO)])
    out = RC.initialize(*a, 1, how=how)
    assert abs(out["poses"][1, 2] - 0.8) <= 1e-14
    np.testing.assert_array_equal(out["poses"][:, :2], a[0][:, :2])     # the rotation stage moves no position


@pytest.mark.parametrize("how", HOWS)
def test_landmark_seen_once(how):
    """A landmark seen once lands at t_i + R_i z."""
    a, _ = _graph([[2.0, 1.0, 0.7], [-5.0, 4.0, 0.0]], [1, 0], [(0, 1, [1.5, -0.5, 5.0], [300.0, 20.0, 7.0, 200.0, -3.0, 11.0])])
    vk, ek = np.array([0, 1], np.uint8), np.array([1], np.uint8)
    out = RC.initialize(*a, 3, vk, ek, how=how)
    assert out["counts"].tolist() == [0, 1, 0]                          # the point is no unknown of the rotation stage
    np.testing.assert_allclose(out["poses"][1, :2], [2.0, 1.0] + _rot(0.7) @ [1.5, -0.5], rtol=0, atol=1e-13)
    assert out["poses"][1, 2] == 0.0


@pytest.mark.parametrize("how", HOWS)
def test_prior_alone_returns_the_prior(how):
    z = [3.0, -1.0, 2.5]
    a, _ = _graph([[0.0, 0.0, -1.0]], [0], [(0, 0, z, [200.0, 30.0, 5.0, 150.0, -4.0, 90.0])])
    out = RC.initialize(*a, 3, np.array([0], np.uint8), np.array([3], np.uint8), how=how)
    assert out["counts"].tolist() == [1, 1, 0]
    np.testing.assert_allclose(out["poses"][0], z, rtol=0, atol=1e-13)


def test_what_a_stage_leaves_out_keeps_its_estimate():
    """A bearing-only point, an isolated vertex and a pose whose heading information is zero."""
    g = CC.case("bearing_lone")
    out = CC.reference("bearing_lone", 3)
    lone = g["lone_bearing_point"]
    np.testing.assert_array_equal(out["poses"][lone], g["poses"][lone])
    poses = np.array([[0.0, 0.0, 0.1], [1.0, 0.0, 0.2], [7.0, 7.0, 0.3], [2.0, 0.0, 0.4]])
    a, _ = _graph(poses, [1, 0, 0, 0], [(0, 1, [1.0, 0.0, 0.05], INFO), (1, 3, [1.0, 0.0, 0.05], [1000.0, 0.0, 0.0, 1000.0, 0.0, 0.0])])
    out = RC.initialize(*a, 3)
    assert out["counts"].tolist() == [1, 2, 0]
    np.testing.assert_array_equal(out["poses"][2], poses[2])            # isolated
    assert out["poses"][3, 2] == poses[3, 2]                            # omega = 0 on its only edge: the heading stays
    np.testing.assert_allclose(out["poses"][3, :2], out["poses"][1, :2] + _rot(out["poses"][1, 2]) @ [1.0, 0.0], atol=1e-12)


def test_no_gauge_is_singular():
    g = CC.singular_pair()
    for stages in (1, 2, 3):
        for how in HOWS:
            with pytest.raises(RC.Singular):
                RC.initialize(*CC.args(g), stages, how=how)


# ----------------------------------------------------------------------------------- independence of the start
@pytest.mark.parametrize("V,E,seed", [(60, 150, 3), (300, 1000, 11)])
def test_result_does_not_depend_on_the_start(V, E, seed):
    g = synth.make_pose_graph(V, E, seed=seed)
    a, b = CC.scrambled(V, E, seed), CC.scrambled(V, E, seed)
    rng = np.random.default_rng(seed + 1000)
    free = g["fixed"] == 0
    b["poses"] = b["poses"].copy()
    b["poses"][free] = np.c_[30.0 * rng.standard_normal((int(free.sum()), 2)), rng.uniform(-np.pi, np.pi, int(free.sum()))]
    ra, rb = RC.initialize(*CC.args(a), 3), RC.initialize(*CC.args(b), 3)
    dp, da = RC.differences(ra["poses"], rb["poses"])
    assert dp <= 1e-12 and da <= 1e-12


# ------------------------------------------------------------------- what the GPU checks rely on, on every case
@pytest.mark.parametrize("name", list(CC.CASES))
def test_reference_solves_agree_and_no_heading_is_degenerate(name):
    """The two solves agree to a tenth of the GPU checks' bars in every stage combination, and no solved (c, s) is zero."""
    for stages in (1, 2, 3):
        a, b = CC.reference(name, stages, "lstsq"), CC.reference(name, stages, "cholesky")
        dp, da = RC.differences(a["poses"], b["poses"])
        print(f"{name} stages {stages}: position {dp:.3e} heading {da:.3e} counts {a['counts'].tolist()}")
        assert dp <= CC.POS_ATOL / 10 and da <= CC.ANG_ATOL / 10
        assert a["counts"].tolist() == b["counts"].tolist() and a["counts"][2] == 0


def test_bearing_only_point_is_uncounted():
    g = CC.case("bearing_lone")
    nV = len(g["poses"])
    # 13 poses (one fixed) in the rotation stage; in the translation stage those, and the observed point
    assert CC.reference("bearing_lone", 3)["counts"].tolist() == [12, 13, 0] and nV == 15


@pytest.mark.parametrize("name", list(CC.SCRAMBLES))
def test_scramble_defeats_gauss_newton_and_chordal_does_not(name):
    """The figures the end-to-end GPU checks rest on: Gauss-Newton from the scramble ends above 100 times the optimum chi2, the
    chordal result is within 2 % of it, and five iterations from there reach it."""
    g = CC.case(name)
    a = CC.args(g)
    _, chi_opt = R.gn_optimize(g["truth"], *a[1:], 10)
    with np.errstate(all="ignore"):
        _, chi_gn = R.gn_optimize(*a, 10)
    init = CC.reference(name, 3)["poses"]
    chi_init = R.chi2(init, *a[2:])
    _, chi_fin = R.gn_optimize(init, *a[1:], 5)
    print(f"{name}: optimum {chi_opt[-1]:.6g}, 10 GN from the scramble {chi_gn[-1]:.3e}, chordal {chi_init:.6g}, + 5 GN {chi_fin[-1]:.9g}")
    assert not chi_gn[-1] <= 100 * chi_opt[-1]
    assert chi_opt[-1] <= chi_init <= 1.02 * chi_opt[-1]
    assert abs(chi_fin[-1] - chi_opt[-1]) <= CC.CHI_FINAL_RTOL * chi_opt[-1]


# --------------------------------------------------------------------------------------------- the entry points
NEW = ("cgmr_chordal_initialize", "cgmr_chordal_initialize_dev", "cgmr_chordal_initialize_typed",
       "cgmr_chordal_initialize_typed_dev", "cgmr_initial_guess")


def test_entry_points_declared_listed_and_exported():
    from cg_mrslam_amd import _lib
    lib = _lib.load_library()
    declared = _lib.declared_symbols()
    for n in NEW:
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    assert lib.cgmr_version() == 105


def test_stage_names():
    from cg_mrslam_amd._lib import chordal_stages
    assert [chordal_stages(s) for s in ("r", "t", "rt", "tr", 1, 2, 3)] == [1, 2, 3, 3, 1, 2, 3]
    for bad in ("", "x", 0, 4, True, 1.0):
        with pytest.raises(ValueError):
            chordal_stages(bad)


def test_initial_guess_needs_no_device():
    """cgmr_initial_guess on host arrays: a chain from a fixed pose composes the measurements; bad indices are refused."""
    from cg_mrslam_amd import _lib
    import ctypes as C
    lib = _lib.load_library()
    p = np.array([[1.0, 2.0, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    fx = np.array([1, 0, 0], np.uint8)
    ef, et = np.array([0, 2], np.int32), np.array([1, 1], np.int32)
    m = np.array([[1.0, 0.0, 0.25], [0.5, 0.0, -0.25]])
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.cgmr_initial_guess(3, ptr(p), ptr(fx), 2, ptr(ef), ptr(et), ptr(m)) == 0
    want1 = synth.se2_compose(p[:1], m[:1])[0]
    np.testing.assert_allclose(p[1], want1, atol=1e-15)
    np.testing.assert_allclose(synth.se2_compose(p[2:3], m[1:2])[0], want1, atol=1e-14)     # x_2 = x_1 * z^-1
    ef[0] = 3
    assert lib.cgmr_initial_guess(3, ptr(p), ptr(fx), 2, ptr(ef), ptr(et), ptr(m)) == -1
