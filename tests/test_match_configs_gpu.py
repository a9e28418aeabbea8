"""The response (k_match_response), the refinement (k_match_refine) and the polish (k_match_polish) on the GPU away from the
three grids their own tests run on: the cases of tests/match_config_cases.py against the float64 yardsticks
(tests/ref_match_response.py, ref_match_refine.py, ref_match_polish.py).  tests/test_match_configs_cpu.py asserts on the CPU
that every case is a fair comparison and is there for what its table says.

Bars: those of the three existing modules, taken over unchanged; derived there, none measured on the device, none widened.
- Response (test_match_response_gpu._check): the sums are of n non-negative double terms, n * 2^-53 relative plus a few ulp of
  exp, so mass and border mass agree to 1e-10 relative, a first moment to 1e-9 of the window's half-width h_i, a second moment
  to 1e-9 h_i h_j (a term of a moment is at most that large), info to 1e-8 of its largest entry; n_candidates is equal.  That
  derivation assumed n <= 4096.  Family C has up to 37 440 candidates: n * 2^-53 = 4e-12, still 25 times under the bar.
- Refinement (test_match_refine_gpu._check): sums of double terms with relative rounding about 1e-13 (2 710 terms in family B:
  3e-13), times the condition bound test_match_configs_cpu.py asserts on the yardstick (1e4) for what goes through the 3x3
  solves -- the pose agrees to 1e-9 of the bound per coordinate, the costs to 1e-9 cost0, the scores to 1e-9 of the fill value,
  the Hessian to 1e-8 of its largest entry; status, stop code, moves, halvings, active points and at_bound bits are equal (no
  decision of the yardstick hangs on less than 1e-11, no point comes within 1e-9 cells of a cell boundary or of the border test).

Every gap is printed before it is asserted.  Figures seen on the MI355X (the largest gap of a family against each bar):
  family    mass     border mass  mean     cov      info    | pose     cost     cost0    score    score0   Hessian
  A         3.4e-16  4.3e-16      4.2e-16  3.7e-16  1.6e-15 | 2.1e-15  7.2e-16  2.1e-16  1.7e-16  3.6e-17  1.1e-15
  B         1.2e-16  1.3e-16      2.8e-16  4.2e-16  1.8e-15 | 5.6e-16  0        2.1e-16  1.1e-16  0        3.7e-16
  C         9.2e-16  1.2e-15      2.2e-15  1.5e-15  2.6e-14 | 1.8e-14  6.1e-15  1.9e-16  1.6e-16  1.8e-17  1.5e-14
  D         3.9e-16  4.3e-16      3.5e-16  2.6e-16  2.9e-15 | 1.0e-14  3.2e-16  1.6e-16  1.9e-16  1.4e-17  1.1e-15
every integer equal, every byte comparison equal: no case found the kernels or their host code wrong.

Shapes: 160-point queries on grids of 161 x 121 to 250 x 250 cells (family A), 2 710 points on 700 x 700 cells (B), 244 to 391
points on 750 x 750 to 1200 x 1200 cells (C), 160 and 373 points on 653 x 517 to 800 x 800 cells (D).
"""
import ctypes as C

import numpy as np
import pytest

from cg_mrslam_amd.matcher import MatchPolished, MatchRefined, MatchResponse, PolishParams, RefineParams, ScanMatcher, normalize_theta

import match_config_cases as M
import matcher_configs as MC
import ref_match_polish as RP

pytestmark = pytest.mark.gpu

T = M.T
ENTRY, RESP, REFD = C.sizeof(MatchPolished), C.sizeof(MatchResponse), C.sizeof(MatchRefined)
LASER = (1081, -2.35, 0.004, 30.0)                               # (the generic calls take points: the laser is not used)
SEEN = {}                                                        # family -> bar -> the largest gap of this session


def _matcher(ctx, grid, laser=LASER):
    ll, ur, res, kr, ks = grid
    m = ScanMatcher(ctx, *laser, resolution=res, kernel_range=kr)
    m.initializeGrid(ll, ur, res)
    m.cfg.kscale = ks
    return m


def _configure(m, cfg):
    """A copy of test_matcher_config_gpu._configure, which stays where it is: the two belong in matcher_configs.py, a clean-up
    of its own because it rewrites that module's imports."""
    c = m.cfg
    c.grid_ll_x, c.grid_ll_y, c.grid_ur_x, c.grid_ur_y = cfg["ll"][0], cfg["ll"][1], cfg["ur"][0], cfg["ur"][1]
    c.resolution, c.kernel_range, c.kscale = cfg["resolution"], cfg["kernel_range"], cfg["kscale"]
    c.win_x, c.win_y, c.win_theta = cfg["win"]
    c.theta_res = cfg["theta_res"]
    c.bin_x, c.bin_y, c.bin_theta = cfg["bins"]
    c.subsample_res, c.min_range = cfg["subsample_res"], cfg["min_range"]
    for k in range(3):
        c.laser_pose[k] = cfg["laser_pose"][k]
    return m


def _note(family, gaps):
    seen = SEEN.setdefault(family, {})
    for k, v in gaps.items():
        seen[k] = max(seen.get(k, 0.0), float(v))
    print(f"family {family}, largest gaps so far: " + " ".join(f"{k} {v:.3e}" for k, v in seen.items()))


def _check_response(got, want, half, what, family):
    """The bars of tests/test_match_response_gpu.py; every figure is printed before it is asserted."""
    assert got["status"] == want["status"] == 0, (what, got["status"], want["status"])
    half = np.asarray(half, dtype=np.float64)
    rel = lambda a, b: abs(a - b) / abs(b)   # noqa: E731
    hh = np.outer(half, half)
    gaps = dict(mass=rel(got["mass"], want["mass"]), border=rel(got["border_mass"], want["border_mass"]),
                mean=np.max(np.abs(got["mean"] - want["mean"]) / half), cov=np.max(np.abs(got["cov"] - want["cov"]) / hh),
                info=np.max(np.abs(got["info"] - want["info"])) / np.max(np.abs(want["info"])))
    print(f"{what}: n {got['n_candidates']}/{want['n_candidates']} " + " ".join(f"{k} gap {v:.3e}" for k, v in gaps.items()))
    _note(family, gaps)
    assert got["n_candidates"] == want["n_candidates"], what
    assert gaps["mass"] <= 1e-10 and gaps["border"] <= 1e-10, (what, gaps)
    assert gaps["mean"] <= 1e-9 and gaps["cov"] <= 1e-9, (what, gaps)
    assert gaps["info"] <= 1e-8, (what, gaps)


def _check_refined(got, want, what, family):
    """The bars of tests/test_match_refine_gpu.py; every figure is printed before it is asserted."""
    ints = ("status", "stop", "n_iters", "n_halvings", "n_active", "at_bound")
    print(f"{what}: " + " ".join(f"{k} {got[k]}/{want[k]}" for k in ints))
    gaps = dict(pose=np.max(np.abs(got["pose"] - want["pose"]) / want["bound"]), cost=abs(got["cost"] - want["cost"]) / want["cost0"],
                cost0=abs(got["cost0"] - want["cost0"]) / want["cost0"], score=abs(got["score"] - want["score"]) / want["fill"],
                score0=abs(got["score0"] - want["score0"]) / want["fill"],
                hessian=np.max(np.abs(got["hessian"] - want["hessian"])) / np.max(np.abs(want["hessian"])))
    print(f"{what}: " + " ".join(f"{k} gap {v:.3e}" for k, v in gaps.items()))
    _note(family, gaps)
    for k in ints:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert gaps["pose"] <= 1e-9, (what, gaps)
    assert gaps["cost"] <= 1e-9 and gaps["cost0"] <= 1e-9, (what, gaps)
    assert gaps["score"] <= 1e-9 and gaps["score0"] <= 1e-9, (what, gaps)
    assert gaps["hessian"] <= 1e-8, (what, gaps)


def _same(a, b, what=""):
    """two result dicts (or dicts of them) hold the same values, bit for bit"""
    assert set(a) == set(b), what
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k], f"{what}.{k}")
        elif a[k] is None or b[k] is None:
            assert a[k] is b[k], (what, k)
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k, a[k], b[k])


def _refined_bytes(raw, job, k):
    o = (4 * job + k) * ENTRY + RESP
    return raw[o:o + REFD]


# ------------------------------------------------------------------------------------------------------------ family A
@pytest.mark.parametrize("name", list(M.A_CASES))
def test_response_and_refinement_on_the_room_scene(ctx, oracle, name):
    c = M.family_a(oracle, name)
    m = _matcher(ctx, c["grid"])
    a = (c["ref"], c["qry"])
    resp = m.matchResponse(*a, c["region"], c["theta_res"], T, c["winner"], step=c["step"])
    _check_response(resp, c["response"], c["half"], f"{name} response", "A")
    refd = m.matchRefine(*a, c["theta_res"], c["winner"], step=c["step"])
    _check_refined(refd, c["refine"], f"{name} refinement", "A")
    assert refd["cost"] <= refd["cost0"]
    if name == "step_010":                                        # (int)(0.1 / (float)0.05) == 1: the calls of step=None, bit for bit
        _same(resp, m.matchResponse(*a, c["region"], c["theta_res"], T, c["winner"]), "response with step=None")
        job = [(*a, c["region"], c["winner"])]
        assert m.matchResponseBatch(job, c["theta_res"], T, step=0.1, raw=True) == m.matchResponseBatch(job, c["theta_res"], T, raw=True)
        assert m.matchRefine(*a, c["theta_res"], c["winner"], step=0.1, raw=True) == m.matchRefine(*a, c["theta_res"], c["winner"], raw=True)
    if name == "step_2":                                          # the bound is bound_steps * x_steps * (float)resolution
        want = c["clipped"]
        got = m.matchRefine(*a, c["theta_res"], c["winner"], RefineParams(bound_steps=0.25), step=c["step"])
        _check_refined(got, want, f"{name} refinement under bound_steps 0.25", "A")
        bound = 0.25 * 2 * float(np.float32(c["grid"][2]))
        assert got["at_bound"] & 3
        for k in range(2):
            if got["at_bound"] >> k & 1:
                assert got["pose"][k] in (c["winner"][k] + bound, c["winner"][k] - bound), (k, got["pose"][k] - c["winner"][k], bound)
            else:
                assert abs(got["pose"][k] - c["winner"][k]) < bound


@pytest.mark.parametrize("name", list(M.A_CASES))
def test_polish_on_the_room_scene(ctx, oracle, name):
    """One matchPolishBatch on the case's own grid: `refined` has the bytes of the matchRefine call, `response` meets the
    yardstick over the window around the winner -- the statements of tests/test_match_polish_gpu.py on the loop-closure grid."""
    c = M.family_a(oracle, name)
    m = _matcher(ctx, c["grid"])
    par = PolishParams(T=T, window=c["half"], refine=RefineParams())
    jobs = [(c["ref"], c["qry"], [c["winner"]])]
    raw = m.matchPolishBatch(jobs, c["theta_res"], par, step=c["step"], raw=True)
    assert len(raw) == 4 * ENTRY
    assert _refined_bytes(raw, 0, 0) == m.matchRefine(c["ref"], c["qry"], c["theta_res"], c["winner"], step=c["step"], raw=True)
    got = m.matchPolishBatch(jobs, c["theta_res"], par, step=c["step"])[0][0]
    _check_response(got["response"], c["polish"]["response"], c["half"], f"{name} polished response", "A")
    _check_refined(got["refined"], c["polish"]["refined"], f"{name} polished refinement", "A")


def test_polish_batch_that_mixes_one_winner_two_winners_and_none(ctx, oracle):
    c = M.family_a(oracle, "unsym_odd")
    m = _matcher(ctx, c["grid"])
    par = PolishParams(T=T, window=c["half"], refine=RefineParams())
    a = (c["ref"], c["qry"])
    wins = [c["winner"], c["moved"]]
    jobs = [(*a, wins[:1]), (*a, wins), (*a, [])]
    raw = m.matchPolishBatch(jobs, c["theta_res"], par, raw=True)
    assert len(raw) == 4 * ENTRY * 3 and m.matchPolishBatch(jobs, c["theta_res"], par, raw=True) == raw
    single = [m.matchRefine(*a, c["theta_res"], w, raw=True) for w in wins]
    assert _refined_bytes(raw, 0, 0) == single[0] and _refined_bytes(raw, 1, 0) == single[0] and _refined_bytes(raw, 1, 1) == single[1]
    got = m.matchPolishBatch(jobs, c["theta_res"], par)
    assert [len(g) for g in got] == [1, 2, 0]
    _check_response(got[0][0]["response"], c["polish"]["response"], c["half"], "job of one winner", "A")
    _check_response(got[1][0]["response"], c["polish"]["response"], c["half"], "job of two winners, the first", "A")
    _check_response(got[1][1]["response"], c["polish_moved"]["response"], c["half"], "job of two winners, the second", "A")
    _same(got[0][0], got[1][0], "the same winner in two jobs")
    for j, n in enumerate((1, 2, 0)):                             # entries beyond n_winners: status 2 in both parts, everything else zero
        for k in range(n, 4):
            e = MatchPolished.from_buffer_copy(raw[(4 * j + k) * ENTRY:(4 * j + k + 1) * ENTRY])
            assert e.response.status == 2 and e.refined.status == 2
            e.response.status = e.refined.status = 0
            assert not any(bytes(e)), (j, k)


# ------------------------------------------------------------------------------------------------------------ family B
def test_more_query_points_than_one_kept_point_list_holds(ctx, oracle):
    """2 710 query points: three chunks of the kept-point list per (angle, pass) unit of the response and of the polish's response,
    and up to six points per thread of the refinement."""
    b = M.family_b(oracle)
    m = _matcher(ctx, b["grid"])
    a = (b["ref"], b["qry"])
    want = b["polish"]
    resp = m.matchResponse(*a, b["region"], b["theta_res"], T, b["winner"])
    _check_response(resp, want["response"], b["half"], "response", "B")
    refd = m.matchRefine(*a, b["theta_res"], b["winner"])
    _check_refined(refd, want["refined"], "refinement", "B")
    par = PolishParams(T=T, window=b["half"], refine=RefineParams())
    jobs = [(*a, [b["winner"]])]
    raw = m.matchPolishBatch(jobs, b["theta_res"], par, raw=True)
    assert _refined_bytes(raw, 0, 0) == m.matchRefine(*a, b["theta_res"], b["winner"], raw=True)
    got = m.matchPolishBatch(jobs, b["theta_res"], par)[0][0]
    _check_response(got["response"], want["response"], b["half"], "polished response", "B")
    _check_refined(got["refined"], want["refined"], "polished refinement", "B")
    assert m.matchPolishBatch(jobs, b["theta_res"], par, raw=True) == raw


# ------------------------------------------------------------------------------------------------------------ family C
def _close_with_both(ctx, c, scans, origin_index, what):
    cfg = c["cfg"]
    m = _configure(ScanMatcher(ctx, cfg["n_beams"], cfg["angle_min"], cfg["angle_inc"], cfg["max_range"]), cfg)
    call = (scans, origin_index, c["ranges_qry"], c["guess"], M.MAX_SCORE)
    par = RefineParams()
    f0, t0 = m.closeScanMatchingVSet(*call)
    f, trel, info, resp, refd = m.closeScanMatchingVSet(*call, covariance_T=T, refine=par)
    assert c["found"] and f0 and f, what
    # the search is matcher_configs.expected_close's, bit for bit, with or without the options
    assert t0.tobytes() == c["expected"][:3].tobytes() == refd["search"].tobytes(), (what, t0, c["expected"], refd["search"])
    _check_response(resp, c["response"], c["half"], f"{what} response", "C")
    assert np.array_equal(info, resp["info"])
    got = {k: v for k, v in refd.items() if k != "search"}
    _check_refined(got, c["refine"], f"{what} refinement", "C")
    assert np.array_equal(trel, refd["pose"]) and refd["cost"] <= refd["cost0"]
    # the two options as their own calls
    f1, t1, info1, resp1 = m.closeScanMatchingVSet(*call, covariance_T=T)
    f2, t2, refd2 = m.closeScanMatchingVSet(*call, refine=par)
    assert f1 and f2 and t1.tobytes() == t0.tobytes() and t2.tobytes() == trel.tobytes()
    assert np.array_equal(info1, info)
    _same(resp1, resp, f"{what}: the response as its own call")
    _same(refd2, refd, f"{what}: the refinement as its own call")


@pytest.mark.parametrize("pair", M.C_PAIRS)
@pytest.mark.parametrize("name", M.C_ENTRIES)
def test_close_matching_with_response_and_refinement_behind_it(ctx, oracle, name, pair):
    """closeScanMatchingVSet(..., covariance_T, refine) away from the default window, grid and laser pose: the points go through
    apply_transf(laser_pose) and the window comes from cfg->win_*."""
    c = M.family_c(oracle, name, pair)
    _close_with_both(ctx, c, [(c["ranges_ref"], np.zeros(3))], 0, f"{name} pair {pair}")


def test_close_matching_with_a_two_scan_reference_set_at_combo_a(ctx, oracle):
    c = M.family_c_vset(oracle)
    _close_with_both(ctx, c, c["scans"], c["origin_index"], "combo_a, two scans")


# ------------------------------------------------------------------------------------------------------------ family D
def _normalised(e):
    out = {"response": dict(e["response"]), "refined": dict(e["refined"])}
    out["response"]["mean"] = e["response"]["mean"].copy()
    out["refined"]["pose"] = e["refined"]["pose"].copy()
    out["response"]["mean"][2] = normalize_theta(out["response"]["mean"][2])
    out["refined"]["pose"][2] = normalize_theta(out["refined"]["pose"][2])
    return out


@pytest.mark.parametrize("name", list(MC.GENERIC))
def test_polished_loop_closure_search_at_other_configurations(ctx, oracle, name):
    par = PolishParams(T=T, refine=RefineParams())
    assert par.window == RP.LC_WINDOW
    # ---- the room scene: the device's own search over scanMatchingLC's region finds the oracle's winner, the polish meets the yardstick
    d = M.family_d(oracle, name)
    m = _matcher(ctx, d["grid"])
    found = m.greedySearch(d["ref"], d["qry"], d["search_region"], d["theta_res"], 0.3, 0.5, 0.5, 0.2)
    assert len(found) > 0 and found[0].tobytes() == d["winner"].tobytes(), (found[:1], d["winner"])
    got = m.matchPolishBatch([(d["ref"], d["qry"], [found[0]])], d["theta_res"], par)[0][0]
    _check_response(got["response"], d["polish"]["response"], d["half"], f"{name} room, polished response", "D")
    _check_refined(got["refined"], d["polish"]["refined"], f"{name} room, polished refinement", "D")
    # ---- scanMatchingLC itself on a pair of scans: the unpolished results are unchanged, every polished entry meets the yardstick
    s = M.family_d_scans(oracle, name)
    sp = s["sp"]
    lcm = _matcher(ctx, s["grid"], (sp["n_beams"], sp["angle_min"], sp["angle_inc"], sp["max_range"]))
    job = ([(sp["ranges_ref"][0], np.zeros(3))], 0, [(sp["ranges_qry"][0], sp["guess"][0])], 0)
    plain = lcm.scanMatchingLC(*job, M.D_SCAN_MAX_SCORE)
    res, pol = lcm.scanMatchingLC(*job, M.D_SCAN_MAX_SCORE, polish=par)
    assert len(res) == len(pol) == len(plain) == len(s["winners"]) >= 1
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res, plain))
    ref = lcm.transformPointsFromVSet(job[0], 0)
    qry = lcm.subsample(lcm.transformPointsFromVSet(job[2], 0), 0.1)
    assert np.array_equal(ref, s["ref"]) and np.array_equal(qry, s["qry"])          # (the points the yardstick was computed on)
    for k in range(len(res)):
        i = next(i for i, w in enumerate(s["winners"]) if (w[0], w[1], normalize_theta(w[2])) == tuple(res[k]))
        want = _normalised(s["polish"][i])
        _check_response(pol[k]["response"], want["response"], RP.LC_WINDOW, f"{name} scans, result {k}, polished response", "D")
        _check_refined(pol[k]["refined"], want["refined"], f"{name} scans, result {k}, polished refinement", "D")
        both = lcm.matchPolishBatch([(ref, qry, [s["winners"][i]])], RP.LC_THETA_RES, par)[0][0]
        _same(pol[k], _normalised(both), f"{name} scans, result {k}: the polish as its own call on the same points")
