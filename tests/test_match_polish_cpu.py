"""CPU-side checks of the polished searches (include/cgmr.h, "Polishing a search's results"): the entry points'
declarations, exports and argument checks that need no device, and the float64 yardstick the GPU tests compare with
(tests/ref_match_polish.py) on its two loop-closure cases.

The conditions on the yardstick are those of tests/test_match_refine_cpu.py, and conditions, not measurements: a case is
a fair comparison for a device in double when none of the refinement's decisions hangs on the sums' rounding, no point
sits on a cell boundary and no 3x3 system is badly conditioned.  Figures seen when the cases were written, default
parameters: `lc_room` decision margin 2.9e-9, kink margin 4.9e-6 cells, condition 9.2; `lc_pi` 1.6e-10, 2.0e-4, 9.6.  The
response at T = 0.01 leaves 1.0e-3 (`lc_room`) and 1.2e-3 (`lc_pi`) of its mass on the window's border.
"""
import ctypes as C
import math

import numpy as np
import pytest

from cg_mrslam_amd import _lib
from cg_mrslam_amd.matcher import (POLISH_MAX_WINNERS, MatcherConfig, MatchPolished, MatchRefined, MatchResponse, PolishJob,
                                   PolishParams, RefineParams)

import ref_match_polish as RP

NEW = ("cgmr_match_polish_batch", "cgmr_scan_matching_lc_polished_batch", "cgmr_scan_matching_lc_polished",
       "cgmr_global_matching_polished_batch", "cgmr_global_matching_polished")
CASES = ("lc_room", "lc_pi")


@pytest.fixture(scope="module")
def runs(oracle):
    """name -> (case, the yardstick's polished winner at T = 0.01 with the default refinement); computed once, never changed."""
    cases = RP.lc_cases(oracle)
    assert tuple(cases) == CASES
    return {n: (c, RP.polish(oracle, c["grid"], c["ref"], c["qry"], c["theta_res"], [c["winner"]], T=0.01, refine={})[0])
            for n, c in cases.items()}


def test_the_header_declares_and_the_library_exports_the_polished_calls():
    lib = _lib.load_library()
    declared = _lib.declared_symbols()
    for n in NEW:
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    assert lib.cgmr_version() == 105
    assert C.sizeof(MatchPolished) == C.sizeof(MatchResponse) + C.sizeof(MatchRefined) == 200 + 152
    assert MatchPolished.refined.offset == C.sizeof(MatchResponse)
    assert POLISH_MAX_WINNERS == 4 and C.sizeof(PolishJob) == 5 * 8 + 8 * 4 * POLISH_MAX_WINNERS
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "cgmr.h")).read()
    assert "#define CGMR_POLISH_MAX_WINNERS 4" in hdr


def test_the_parameters():
    p = PolishParams()
    assert p.T is None and p.window == (0.5, 0.5, 0.2) and p.refine is None
    pod = p.pod()
    assert pod.T == 0.0 and list(pod.window) == [0.5, 0.5, 0.2] and pod.refine == 0 and C.sizeof(pod) == 8 + 24 + 8 + 32
    pod = PolishParams(T=0.01, window=(0.2, 0.3, 0.1), refine=RefineParams(ridge=1e-3)).pod()
    assert pod.T == 0.01 and list(pod.window) == [0.2, 0.3, 0.1] and pod.refine == 1
    assert (pod.refine_params.ridge, pod.refine_params.max_iters) == (1e-3, 10)
    with pytest.raises(ValueError):
        PolishParams(refine=0.5)
    with pytest.raises(ValueError):
        PolishParams(window=(0.5, 0.5))


def test_a_null_context_is_refused_without_a_device():
    """Every call turns a missing context down before it looks at anything else and leaves the outputs alone."""
    lib = _lib.load_library()
    E_INVALID = lib.cgmr_match_last_stats(None, (C.c_int64 * 4)())    # (the code every entry point returns for a null context)
    assert E_INVALID < 0
    cfg = MatcherConfig()
    lib.cgmr_matcher_config_close(C.byref(cfg), C.c_int(1081), C.c_double(-2.35), C.c_double(0.004), C.c_double(30.0))
    pts = np.zeros((4, 2))
    for par in (PolishParams(T=0.01, refine=RefineParams()), PolishParams(T=-1.0), PolishParams(window=(0.0, 0.5, 0.2))):
        pod = par.pod()
        out = (MatchPolished * 4)()
        for k in range(4):
            out[k].response.status = out[k].refined.status = 77
        job = PolishJob(4, pts.ctypes.data, 4, pts.ctypes.data, 1)
        rc = lib.cgmr_match_polish_batch(None, C.byref(cfg), C.c_int(1), C.byref(job), C.c_double(0.1), C.c_double(0.1), C.c_double(0.025),
                                         C.byref(pod), out)
        assert rc == E_INVALID and all(out[k].response.status == 77 and out[k].refined.status == 77 for k in range(4))
        trel, n, found = (C.c_double * 6)(*([3.0] * 6)), C.c_int(5), C.c_int(6)
        for fn in (lib.cgmr_scan_matching_lc_polished_batch, lib.cgmr_global_matching_polished_batch):
            rc = fn(None, C.byref(cfg), C.c_int(1), None, None, C.c_double(0.15), C.byref(pod), trel, C.byref(n), out)
            assert rc == E_INVALID and n.value == 5 and trel[0] == 3.0 and out[0].response.status == 77
        rc = lib.cgmr_scan_matching_lc_polished(None, C.byref(cfg), None, None, C.c_double(0.15), C.byref(pod), trel, C.byref(n), out)
        assert rc == E_INVALID and n.value == 5 and trel[0] == 3.0 and out[0].refined.status == 77
        rc = lib.cgmr_global_matching_polished(None, C.byref(cfg), None, None, C.c_double(0.15), C.byref(pod), trel, C.byref(found), out)
        assert rc == E_INVALID and found.value == 6 and trel[0] == 3.0 and out[0].refined.status == 77
    assert lib.cgmr_match_polish_batch(None, None, C.c_int(0), None, C.c_double(0), C.c_double(0), C.c_double(0), None, None) == E_INVALID


def test_the_window_rule():
    w = np.array([0.10000229, -0.20000076, 3.16659255, 0.045])
    reg = RP.window_region(w, (0.5, 0.5, 0.2))
    assert reg.dtype == np.float32 and reg.shape == (6,)
    for q in range(3):
        assert reg[q] == np.float32(w[q] - (0.5, 0.5, 0.2)[q]) and reg[3 + q] == np.float32(w[q] + (0.5, 0.5, 0.2)[q])


@pytest.mark.parametrize("name", CASES)
def test_what_the_cases_were_chosen_for(runs, name):
    case, got = runs[name]
    r = got["refined"]
    e0 = np.hypot(*(case["winner"][:2] - case["true"][:2]))
    e1 = np.hypot(*(r["pose"][:2] - case["true"][:2]))
    print(f"{name}: winner {case['winner']} of {case['n_search']} candidates, translation error {1e3 * e0:.1f} mm -> {1e3 * e1:.1f} mm "
          f"in {r['n_iters']} moves (stop {r['stop']})")
    assert case["n_search"] == 19500                              # scanMatchingLC's region on the loop-closure grid
    centre = (0.1, -0.2, 0.025 + (math.pi if name == "lc_pi" else 0.0))
    assert np.max(np.abs(case["winner"][:3] - centre)) < 1e-5     # the grid cell next to the true pose
    assert e0 > 0.05 and e1 < e0 / 10 and (r["n_iters"], r["stop"]) == (3, 1)
    assert got["response"]["n_candidates"] == 1700 and got["response"]["shape"] == (10, 10, 17)   # one pass of 100 cells per angle
    assert len(case["qry"]) == 160


@pytest.mark.parametrize("name", CASES)
def test_the_yardstick_is_a_fair_comparison_on_the_case(runs, name):
    _, got = runs[name]
    r = got["refined"]
    d = r["diag"]
    print(f"{name}: decision margin {d['decision']:.3e} kink margin {d['kink']:.3e} cells condition {d['cond']:.3e}")
    assert r["status"] == 0 and r["cost"] <= r["cost0"]
    assert d["decision"] >= 1e-11
    assert d["kink"] >= 1e-9
    assert d["cond"] <= 1e4


@pytest.mark.parametrize("name", CASES)
def test_the_response_yardstick(runs, name):
    """Status 0, and the border mass within 20 % of the figure stated for the case (1.0e-3 for `lc_room`, 1.2e-3 for `lc_pi`: the
    figures are given to two digits, and a yardstick that changed would move them by far more)."""
    _, got = runs[name]
    q = got["response"]
    print(f"{name}: status {q['status']} border mass {q['border_mass']:.3e} mass {q['mass']:.6g}")
    assert q["status"] == 0 and np.all(np.isfinite(q["info"])) and np.all(np.linalg.eigvalsh(q["info"]) > 0)
    stated = {"lc_room": 1.0e-3, "lc_pi": 1.2e-3}[name]
    assert abs(q["border_mass"] - stated) <= 0.2 * stated


@pytest.mark.parametrize("window,cells,passes", [(RP.LC_WINDOW, 100, 1), (RP.LC_MID_WINDOW, 196, 1), (RP.LC_BIG_WINDOW, 676, 2)])
def test_the_windows_cover_the_candidate_slots_and_more_than_one_pass(oracle, runs, window, cells, passes):
    """A pass holds at most 576 cells of one angle, 64 lanes x up to 9 slots: 100 cells take 2 slots per lane, 196 take 4, 676 take
    9 and a second pass.  Asserted on the yardstick's own candidate list."""
    case, _ = runs["lc_room"]
    q = RP.polish(oracle, case["grid"], case["ref"], case["qry"], case["theta_res"], [case["winner"]], T=0.01, window=window)[0]["response"]
    nx, ny, nth = q["shape"]
    print(f"window {window}: {nx} x {ny} cells, {nth} angles, border mass {q['border_mass']:.3e}")
    assert nx * ny == cells and -(-cells // RP.PASS_CELLS) == passes and q["n_candidates"] == cells * nth <= 65536 and q["status"] == 0
    assert (-(-min(cells, RP.PASS_CELLS) // 64) <= 2) == (cells == 100) and (-(-cells // 64) <= 4) == (cells <= 196)


def test_the_parts_that_are_not_asked_for(oracle, runs):
    case, _ = runs["lc_room"]
    a = (oracle, case["grid"], case["ref"], case["qry"], case["theta_res"], [case["winner"]])
    r = RP.polish(*a)[0]
    assert r["response"]["status"] == 3 and r["refined"]["status"] == 3
    assert np.array_equal(r["refined"]["pose"], case["winner"][:3]) and r["refined"]["cost0"] == 0 and not r["response"]["info"].any()
    r = RP.polish(*a, T=0.01)[0]
    assert r["response"]["status"] == 0 and r["refined"]["status"] == 3
    r = RP.polish(*a, refine={})[0]
    assert r["response"]["status"] == 3 and r["refined"]["status"] == 0
