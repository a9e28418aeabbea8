"""CPU-side checks of the scan matcher's sub-cell refinement (include/cgmr.h, "Refining a match below the grid's
resolution"): the float64 yardstick the GPU tests compare with (tests/ref_match_refine.py) on its named cases, and the
entry points' declarations, exports and argument checks that need no device.

The conditions on the yardstick are conditions, not measurements: a case is only a fair comparison for a device in
double when none of its decisions hangs on the sums' rounding (about 1e-14), no point sits on a cell boundary and no
3x3 system is badly conditioned.  Figures seen when the cases were written: decision margins >= 1.9e-10, kink margins
>= 5.7e-7 cells, condition numbers <= 2.3e3.
"""
import ctypes as C

import numpy as np
import pytest

from cg_mrslam_amd import _lib
from cg_mrslam_amd.matcher import MatcherConfig, MatchRefined, RefineJob, RefineParams

import ref_match_refine as RR

NEW = ("cgmr_refine_params_default", "cgmr_match_refine", "cgmr_match_refine_batch", "cgmr_close_scan_matching_refined")
NAMED = ("room", "corridor", "rotated", "clamped", "sparse", "pinned", "dense")


@pytest.fixture(scope="module")
def runs(oracle):
    """name -> (case, the yardstick's result); computed once, never changed."""
    cases = RR.named_cases(oracle)
    assert tuple(cases) == NAMED
    return {n: (c, RR.refine(oracle, c["grid"], c["ref"], c["qry"], c["theta_res"], c["winner"], c["params"])) for n, c in cases.items()}


def test_the_header_declares_and_the_library_exports_the_refinement():
    lib = _lib.load_library()
    declared = _lib.declared_symbols()
    for n in NEW:
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    assert lib.cgmr_version() == 105
    assert C.sizeof(MatchRefined) == 8 * (3 + 4 + 9) + 4 * 6
    p = RefineParams()
    assert (p.max_iters, p.max_halvings, p.ridge, p.step_tol, p.bound_steps) == (10, 4, 1e-6, 1e-6, 1.0)
    assert RefineParams(ridge=1e-3).ridge == 1e-3 and RefineParams(ridge=1e-3).max_iters == 10
    assert dict(RR.DEFAULTS) == {k: getattr(p, k) for k in RR.DEFAULTS}


def test_a_null_context_is_refused_without_a_device():
    """No context can exist without a device: every call turns a missing one down before it looks at anything else and
    leaves the outputs alone."""
    lib = _lib.load_library()
    E_INVALID = lib.cgmr_match_last_stats(None, (C.c_int64 * 4)())    # (the code every entry point returns for a null context)
    assert E_INVALID < 0
    cfg = MatcherConfig()
    lib.cgmr_matcher_config_close(C.byref(cfg), C.c_int(1081), C.c_double(-2.35), C.c_double(0.004), C.c_double(30.0))
    pts = np.zeros((4, 2))
    win = np.zeros(4)
    out = MatchRefined()
    out.status = 77
    for par in (RefineParams(), RefineParams(max_iters=0), RefineParams(ridge=float("nan"))):
        rc = lib.cgmr_match_refine(None, C.byref(cfg), C.c_int(4), C.c_void_p(pts.ctypes.data), C.c_int(4), C.c_void_p(pts.ctypes.data),
                                   C.c_double(0.05), C.c_double(0.05), C.c_double(0.02), C.c_void_p(win.ctypes.data), C.c_int(1),
                                   C.byref(par), C.byref(out))
        assert rc == E_INVALID and out.status == 77
        job = RefineJob(4, pts.ctypes.data, 4, pts.ctypes.data, (C.c_double * 4)(), 1)
        rc = lib.cgmr_match_refine_batch(None, C.byref(cfg), C.c_int(1), C.byref(job), C.c_double(0.05), C.c_double(0.05),
                                         C.c_double(0.02), C.byref(par), C.byref(out))
        assert rc == E_INVALID and out.status == 77
        trel, search, found = (C.c_double * 3)(3.0, 3.0, 3.0), (C.c_double * 3)(4.0, 4.0, 4.0), C.c_int(5)
        rc = lib.cgmr_close_scan_matching_refined(None, C.byref(cfg), None, None, None, C.c_double(0.15), C.byref(par), trel, search,
                                                  C.byref(found), C.byref(out))
        assert rc == E_INVALID and found.value == 5 and trel[0] == 3.0 and search[0] == 4.0 and out.status == 77
    assert lib.cgmr_match_refine(None, None, C.c_int(0), None, C.c_int(0), None, C.c_double(0), C.c_double(0), C.c_double(0), None,
                                 C.c_int(0), None, None) == E_INVALID


@pytest.mark.parametrize("name", NAMED)
def test_the_yardstick_is_a_fair_comparison_on_the_case(runs, name):
    case, r = runs[name]
    d = r["diag"]
    print(f"{name}: decision margin {d['decision']:.3e} kink margin {d['kink']:.3e} cells condition {d['cond']:.3e}")
    assert r["status"] == 0
    assert d["decision"] >= 1e-11
    assert d["kink"] >= 1e-9
    assert d["cond"] <= 1e4


@pytest.mark.parametrize("name", NAMED)
def test_the_yardstick_never_raises_the_cost_and_stays_within_the_bound(runs, name):
    case, r = runs[name]
    assert r["cost"] <= r["cost0"] and np.all(np.isfinite(r["pose"])) and np.all(np.isfinite(r["hessian"]))
    assert np.all(np.abs(r["pose"] - case["winner"][:3]) <= r["bound"] * (1 + 1e-15))
    assert 0 <= r["n_iters"] <= 10 and r["n_active"] == len(case["qry"])
    assert np.array_equal(r["hessian"], r["hessian"].T)


def test_what_the_cases_were_chosen_for(runs):
    for name in ("room", "corridor", "rotated"):
        assert (runs[name][1]["n_iters"], runs[name][1]["stop"]) == (3, 1), name
    assert runs["clamped"][1]["at_bound"] & 3 == 3
    assert runs["sparse"][1]["n_halvings"] >= 1
    assert runs["pinned"][1]["at_bound"] == 7
    assert len(runs["dense"][0]["qry"]) > 512 and len(runs["room"][0]["qry"]) == 160
    assert {r["stop"] for _, r in runs.values()} == {0, 1, 2, 3}
    for name in ("room", "rotated"):
        case, r = runs[name]
        e0 = np.hypot(*(case["winner"][:2] - case["true"][:2]))
        e1 = np.hypot(*(r["pose"][:2] - case["true"][:2]))
        print(f"{name}: translation error {1e3 * e0:.2f} mm -> {1e3 * e1:.2f} mm")
        assert e1 < e0, name


def test_points_off_the_grid_count_the_fill_value_and_nothing_else(oracle, runs):
    case, r = runs["room"]
    off = np.stack([np.full(20, 5.5), np.linspace(-1, 1, 20)], axis=1)
    qry = np.concatenate([case["qry"], off])
    r2 = RR.refine(oracle, case["grid"], case["ref"], qry, case["theta_res"], case["winner"], case["params"])
    assert np.max(np.abs(r2["pose"] - r["pose"])) <= 1e-12
    fill = r["fill"]
    assert fill == 25 / 128
    assert abs((r2["cost"] - r["cost"]) - 20 * fill ** 2) <= 1e-12 and abs((r2["cost0"] - r["cost0"]) - 20 * fill ** 2) <= 1e-12
    assert r2["n_active"] == r["n_active"] and (r2["stop"], r2["n_iters"]) == (r["stop"], r["n_iters"])


def test_the_yardstick_statuses(oracle, runs):
    case, _ = runs["room"]
    a = (oracle, case["grid"], case["ref"])
    r = RR.refine(*a, np.zeros((0, 2)), case["theta_res"], case["winner"])
    assert r["status"] == 1 and np.array_equal(r["pose"], case["winner"][:3]) and r["cost"] == 0 and not r["hessian"].any()
    r = RR.refine(*a, np.full((7, 2), 7.0), case["theta_res"], case["winner"])
    assert r["status"] == 1 and np.array_equal(r["pose"], case["winner"][:3]) and r["cost0"] == 0
    r = RR.refine(*a, case["qry"], case["theta_res"], case["winner"], found=False)
    assert r["status"] == 2 and np.array_equal(r["pose"], case["winner"][:3]) and r["n_active"] == 0
