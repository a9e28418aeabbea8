"""CPU-side checks of the cases that take the response, the refinement and the polish away from their tests' three grids
(tests/match_config_cases.py): the float64 yardstick is a fair comparison on every case, every case is there for what its
table says, and the response yardstick is finite.  On the yardstick and the CPU oracle alone; no device.

The conditions are those of tests/test_match_refine_cpu.py -- no decision of the refinement hangs on less than 1e-11, no
inside point comes within 1e-9 cells of a cell boundary, no 3x3 system has a condition above 1e4 -- and, set beside the second
for the same reason, no point, inside or outside, comes within 1e-9 cells of the border test (u against 0 and nx - 1, v
against 0 and ny - 1: ``diag["border"]``).  They are conditions, not measurements.  Figures seen when the cases were written:

  family A  decision >= 6.1e-10 (2.3e-11 for `step_2` under bound_steps = 0.25), kink >= 4.7e-6 cells, cond <= 19; border 4.7e-6
            cells on `edge_in` and 2.0e-5 on `edge_out` and `edge_out_k100`, 26 cells or more elsewhere.  (When `edge_in` was
            proposed its border margin was given as 6.3e-3 cells.  The diagnostic here is the minimum over all ten poses the
            run evaluates -- at the winner alone it is 3.7e-2 -- and the point that sets it also sets the kink margin: its u
            lies 4.7e-6 below nx - 1, which is an integer.  The condition of 1e-9 holds with either figure.)
  family B  decision 1.0e-7, kink 1.7e-6, border 204, cond 35
  family C  decision >= 5.2e-9, kink >= 1.2e-6, border >= 2.3, cond <= 75
  family D  decision >= 1.4e-9, kink >= 4.9e-6, border >= 207, cond <= 9.4; on the pair of scans 2.4e-7, 1.6e-5, 149, 94
"""
import numpy as np
import pytest

import match_config_cases as M
import matcher_configs as MC
import ref_match_polish as RP
import ref_match_refine as RR
import ref_match_response as R


@pytest.mark.parametrize("label", list(M.LABELS))
def test_the_yardstick_is_a_fair_comparison_on_the_case(oracle, label):
    _, r, _, _ = M.case(oracle, label)
    runs = [(label, r)]
    if label == "A-step_2":
        runs.append((label + " under bound_steps 0.25", M.family_a(oracle, "step_2")["clipped"]))
    for what, r in runs:
        d = r["diag"]
        print(f"{what}: decision margin {d['decision']:.3e} kink margin {d['kink']:.3e} cells border margin {d['border']:.3e} cells "
              f"condition {d['cond']:.3e}; {r['n_iters']} moves, {r['n_halvings']} halvings, stop {r['stop']}, {r['n_active']} active points")
        assert r["status"] == 0 and r["cost"] <= r["cost0"], what
        assert d["decision"] >= 1e-11, what
        assert d["kink"] >= 1e-9, what
        assert d["border"] >= 1e-9, what
        assert d["cond"] <= 1e4, what


@pytest.mark.parametrize("label", list(M.LABELS))
def test_the_response_yardstick_is_a_fair_comparison_on_the_case(oracle, label):
    _, _, q, n = M.case(oracle, label)
    print(f"{label}: status {q['status']} n {q['n_candidates']} mass {q['mass']:.6g} border mass {q['border_mass']:.3e}")
    assert q["status"] == 0 and np.isfinite(q["mass"]) and q["mass"] > 0
    assert np.all(np.isfinite(q["info"])) and np.all(np.isfinite(q["cov"])) and np.all(np.isfinite(q["mean"]))
    if isinstance(n, tuple):
        assert n[0] <= q["n_candidates"] <= n[1], (label, q["n_candidates"])
    else:
        assert q["n_candidates"] == n, (label, q["n_candidates"])


@pytest.mark.parametrize("name", list(M.A_CASES))
def test_what_the_cases_of_the_room_scene_are_there_for(oracle, name):
    c, spec = M.family_a(oracle, name), M.A_CASES[name]
    fld = RR.field(oracle, c["grid"], c["ref"])
    assert fld[0].shape == spec["cells"], (name, fld[0].shape)
    assert len(c["cands"]) == spec["n_cands"] and len(c["qry"]) == 160
    assert c["refine"]["stop"] == spec["stop"], (name, c["refine"]["stop"])
    res32 = float(np.float32(c["grid"][2]))
    if name == "unsym_odd":
        assert all(n & 7 for n in fld[0].shape) and fld[0].shape[0] != fld[0].shape[1]
        assert any(float(np.float32(v)) != v for v in c["grid"][0] + c["grid"][1])
    if name == "radius_10":
        assert int(c["grid"][3] / c["grid"][2]) == 10 and fld[4] == 64 / 128
    if name == "kscale_100":
        assert fld[4] == 20 / 100
    if name == "edge_out_k100":
        assert fld[4] == 20 / 100 and c["grid"][:4] == M.A_CASES["edge_out"]["grid"][:4]
    if name in ("edge_in", "edge_out", "edge_out_k100"):
        at = M.border_census(oracle, c["grid"], c["ref"], c["qry"], c["winner"])
        print(f"{name}: at the winner {at}, {c['refine']['n_active']} active points at the refined pose")
        assert max(at["last_x"], at["last_y"]) >= 15 and at["beyond_x"] + at["beyond_y"] >= 1
        if name == "edge_in":
            assert at["last_x"] >= 15 and at["last_y"] >= 15 and at["beyond_x"] == 0
        else:
            assert at["beyond_x"] >= 15 and at["last_y"] >= 15
            assert c["refine"]["n_active"] <= 160 - 15
    if name == "step_010":
        assert R.steps_of(c["grid"], 0.1)[0] == 1 and 0.1 / 0.05 == 2.0          # the truncation, against the quotient in double
        plain = R.candidates(oracle, c["grid"], c["ref"], c["qry"], c["region"], c["theta_res"])
        assert np.array_equal(c["cands"], plain)
        assert np.array_equal(c["refine"]["bound"], [res32, res32, c["theta_res"]])
    if name == "step_2":
        assert R.steps_of(c["grid"], 0.15)[0] == 2 and RP.cells_per_angle(c["cands"]) == (6, 6, 4)
        one = M.family_a(oracle, "unsym_odd")["refine"]["bound"]
        assert np.array_equal(c["refine"]["bound"], [2 * one[0], 2 * one[1], one[2]]) and one[0] == res32
        clipped = c["clipped"]
        assert clipped["at_bound"] & 3 and np.array_equal(clipped["bound"][:2], [0.25 * 2 * res32] * 2)
        for k in range(2):
            if clipped["at_bound"] >> k & 1:
                assert abs(clipped["pose"][k] - c["winner"][k]) == pytest.approx(0.25 * 2 * res32, rel=1e-12)
    if name == "theta_26":
        assert c["winner"][2] > 2.5 and RP.cells_per_angle(c["cands"]) == (8, 8, 5)


def test_what_the_other_families_are_there_for(oracle):
    b = M.family_b(oracle)
    assert len(b["qry"]) > 2200 and len(b["qry"]) == 2710 and len(b["ref"]) == 1081 and b["n_search"] == 900
    assert b["polish"]["response"]["shape"] == (10, 10, 16)
    for n in M.C_ENTRIES:
        for p in M.C_PAIRS:
            c = M.family_c(oracle, n, p)
            assert c["found"] and c["cands0"].tobytes() == c["expected"].tobytes(), (n, p)
            assert len(c["qry"]) in (373, 391)
    c = M.family_c_vset(oracle)
    assert c["found"] and c["cands0"].tobytes() == c["expected"].tobytes() and len(c["scans"]) == 2
    assert any(M.family_c(oracle, "combo_a", 0)["cfg"]["laser_pose"]) and MC.CONFIGS["kr_03"][2]["edt"] == 0
    for n in MC.GENERIC:
        d = M.family_d(oracle, n)
        r = d["polish"]["refined"]
        assert d["n_search"] == (78000 if n == "radius_10" else 19500) and (r["n_iters"], r["stop"]) == (3, 1), n
        assert d["polish"]["response"]["shape"] == ((20, 20, 16) if n == "radius_10" else (10, 10, 17))


@pytest.mark.parametrize("name", list(MC.GENERIC))
def test_the_scan_form_of_the_loop_closure_cases_is_a_fair_comparison(oracle, name):
    """scanMatchingLC's own input (family D on a pair of scans): every winner of its two searches under the same conditions."""
    s = M.family_d_scans(oracle, name)
    assert len(s["winners"]) >= 1 and len(s["qry"]) == 373
    for k, p in enumerate(s["polish"]):
        r, q, d = p["refined"], p["response"], p["refined"]["diag"]
        print(f"{name} winner {k} {s['winners'][k]}: decision margin {d['decision']:.3e} kink margin {d['kink']:.3e} cells border margin "
              f"{d['border']:.3e} cells condition {d['cond']:.3e}; {r['n_iters']} moves, stop {r['stop']}; response {q['shape']}, "
              f"border mass {q['border_mass']:.3e}")
        assert r["status"] == 0 and q["status"] == 0 and np.isfinite(q["mass"]) and q["mass"] > 0 and np.all(np.isfinite(q["info"]))
        assert d["decision"] >= 1e-11 and d["kink"] >= 1e-9 and d["border"] >= 1e-9 and d["cond"] <= 1e4
        assert q["shape"] == ((20, 20, 16) if name == "radius_10" else (10, 10, 16))


def test_the_stop_codes_over_all_cases(oracle):
    stops = {M.case(oracle, label)[1]["stop"] for label in M.LABELS}
    assert stops >= {0, 1, 2}, stops
