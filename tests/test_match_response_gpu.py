"""The scan matcher's response surface on the GPU (include/cgmr.h, "Scan-match covariance") against the float64
yardstick of tests/ref_match_response.py: numpy over the CPU oracle's own candidate list.

Bars (derived, not measured): the sums are of n <= 4096 non-negative double terms -- n * 2^-53 ~ 5e-13 relative, plus a
few ulp of exp -- so mass and border_mass agree to 1e-10 relative, a second moment to 1e-9 h_i h_j and a first moment to
1e-9 h_i with h the window's half-widths (a term of a moment is at most that large), info to 1e-8 of its largest entry.

Temperature.  The scenes' T is 0.01.  At T = 0.01 the yardstick gives the corridor an eigenvalue ratio of 24 with the
large axis along x and a border mass of 0.43, as required, but the ROOM a border mass of 0.33, not < 1e-3: the window of
+-0.04 rad at 0.02 rad holds four angles, the winner is the third, so its neighbour at +0.02 rad is the last of its
range and carries weight at any temperature that is not small against that neighbour's score difference.  The
yardstick's room border mass is 0.030 at T = 0.002 and 8.9e-4 at T = 0.001; the corridor's border mass falls below 0.1
just under T = 0.00104.  No single T meets both conditions, so the room's condition is checked at T = 0.001 and the
corridor's at the scenes' 0.01; the conditions themselves stand as they were set.
"""
import os

import numpy as np
import pytest

from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import CgmrError
from cg_mrslam_amd.matcher import LCScanMatcher, ScanMatcher
from cg_mrslam_amd.slam import SM_INFO, GraphSLAMDriver, run_srslam

import oracle_backend as OB
import ref_match_response as R

pytestmark = pytest.mark.gpu

T = 0.01
T_ROOM_MEANING = 0.001
BIG_HALF = (0.65, 0.65, 0.03)                                  # 26 x 26 cells, 3 angles: 676 > 576 candidates per angle


def _matcher(ctx):
    ll, ur, res, kr, ks = R.GRID
    m = ScanMatcher(ctx, 1081, -2.35, 0.004, 30.0, resolution=res, kernel_range=kr)
    m.initializeGrid(ll, ur, res)
    m.cfg.kscale = ks
    return m


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (ref, qry, region, half-widths, every candidate of the region by the oracle); computed once, never changed."""
    cor, room = R.corridor(), R.room()
    assert len(cor) == 240 and len(room) == 320
    out = {}
    for name, ref, qry, centre, half, cap in (("corridor", cor, cor[::2], (0, 0, 0), R.HALF, 4096),
                                              ("room", room, room[::2], (0, 0, 0), R.HALF, 4096),
                                              ("big", room, room[::2], (0, 0, 0), BIG_HALF, 8192),
                                              ("rotated", room, R.turned(room[::2], 0.3), (0, 0, 0.3), R.HALF, 4096)):
        reg = R.region_around(centre, half)
        c = R.candidates(oracle, R.GRID, ref, qry, reg, R.THETA_RES, cap=cap)
        for a in (ref, qry, reg, c):
            a.setflags(write=False)
        out[name] = (ref, qry, reg, np.asarray(half), c)
    return out


def _want(case, t):
    return R.response(case[4], case[4][0], t, R.GRID, R.THETA_RES)


def _got(m, case, t):
    ref, qry, reg, _, c = case
    return m.matchResponse(ref, qry, reg, R.THETA_RES, t, c[0])


def _check(got, want, half, what):
    """The bars of the module docstring; every figure is printed before it is asserted."""
    assert got["status"] == want["status"] == 0, what
    rel = lambda a, b: abs(a - b) / abs(b)   # noqa: E731
    hh = np.outer(half, half)
    gaps = dict(mass=rel(got["mass"], want["mass"]), border=rel(got["border_mass"], want["border_mass"]),
                mean=np.max(np.abs(got["mean"] - want["mean"]) / half), cov=np.max(np.abs(got["cov"] - want["cov"]) / hh),
                info=np.max(np.abs(got["info"] - want["info"])) / np.max(np.abs(want["info"])))
    print(f"{what}: n {got['n_candidates']} " + " ".join(f"{k} gap {v:.3e}" for k, v in gaps.items()))
    assert got["n_candidates"] == want["n_candidates"], what
    assert gaps["mass"] <= 1e-10 and gaps["border"] <= 1e-10, (what, gaps)
    assert gaps["mean"] <= 1e-9 and gaps["cov"] <= 1e-9, (what, gaps)
    assert gaps["info"] <= 1e-8, (what, gaps)


def _meaning(corridor, room, what):
    ev, evec = np.linalg.eigh(corridor["cov"][:2, :2])
    assert ev[1] / ev[0] >= 10 and abs(evec[0, 1]) > abs(evec[1, 1]), (what, ev, evec)     # large axis along x
    assert corridor["border_mass"] > 0.1, (what, corridor["border_mass"])
    assert room["border_mass"] < 1e-3, (what, room["border_mass"])


@pytest.mark.parametrize("name", ["corridor", "room"])
def test_parity_with_the_yardstick(ctx, cases, name):
    m = _matcher(ctx)
    c = cases[name][4]
    assert len(c) == 8 * 8 * 4
    _check(_got(m, cases[name], T), _want(cases[name], T), cases[name][3], name)


def test_corridor_is_unconstrained_along_x_and_the_room_is_not(ctx, cases):
    # on the yardstick alone first
    _meaning(_want(cases["corridor"], T), _want(cases["room"], T_ROOM_MEANING), "yardstick")
    m = _matcher(ctx)
    room = _got(m, cases["room"], T_ROOM_MEANING)
    _check(room, _want(cases["room"], T_ROOM_MEANING), cases["room"][3], "room at the lower temperature")
    _meaning(_got(m, cases["corridor"], T), room, "device")


def test_more_than_one_candidate_pass_and_workgroup(ctx, cases):
    c = cases["big"][4]
    assert len(c) == 26 * 26 * 3 and len(np.unique(c[:, 0])) == 26 and len(np.unique(c[:, 1])) == 26
    _check(_got(_matcher(ctx), cases["big"], T), _want(cases["big"], T), cases["big"][3], "26 x 26 x 3")


def test_rotated_winner(ctx, cases):
    c = cases["rotated"][4]
    assert abs(c[0][2] - 0.3) < R.THETA_RES and abs(c[0][0]) <= 0.05 and abs(c[0][1]) <= 0.05
    want = _want(cases["rotated"], T)
    assert np.abs(want["info"][0, 1]) > 1e-3 * np.abs(want["info"]).max()        # (the rotation shows in the translation block)
    _check(_got(_matcher(ctx), cases["rotated"], T), want, cases["rotated"][3], "rotated by 0.3 rad")


def _batch_jobs(cases):
    return [(cases[n][0], cases[n][1], cases[n][2], cases[n][4][0]) for n in ("corridor", "room", "big", "rotated")]


def test_batch_equals_the_single_calls_and_is_deterministic(ctx, cases):
    m = _matcher(ctx)
    jobs = _batch_jobs(cases)
    got = m.matchResponseBatch(jobs + [(jobs[0][0], jobs[0][1], jobs[0][2], None)], R.THETA_RES, T)
    for k, n in enumerate(("corridor", "room", "big", "rotated")):
        _check(got[k], _got(m, cases[n], T), cases[n][3], f"batch job {n} against its single call")
        _check(got[k], _want(cases[n], T), cases[n][3], f"batch job {n} against the yardstick")
    skipped = got[4]                                              # the search before found nothing
    assert skipped["status"] == 2 and skipped["n_candidates"] == 0 and skipped["mass"] == 0
    assert not skipped["cov"].any() and not skipped["info"].any() and not skipped["mean"].any()
    a = m.matchResponseBatch(jobs, R.THETA_RES, T, raw=True)
    b = m.matchResponseBatch(jobs, R.THETA_RES, T, raw=True)
    assert len(a) > 0 and a == b


def test_status_paths(ctx, cases, oracle):
    m = _matcher(ctx)
    ref, qry, reg, _, c = cases["room"]
    assert len(R.candidates(oracle, R.GRID, ref, np.zeros((0, 2)), reg, R.THETA_RES)) == 0
    r = m.matchResponse(ref, np.zeros((0, 2)), reg, R.THETA_RES, T, c[0])       # k == 0: no candidate is counted
    assert r["status"] == 1 and r["n_candidates"] == 0 and r["mass"] == 0 and r["border_mass"] == 0
    assert not r["cov"].any() and not r["info"].any() and not r["mean"].any()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(CgmrError, match="temperature"):
            m.matchResponse(ref, qry, reg, R.THETA_RES, bad, c[0])
    with pytest.raises(CgmrError, match="exactly one"):
        m.matchResponseBatch([(ref, qry, np.concatenate([reg, reg]), c[0])], R.THETA_RES, T)
    # a close match with max_score below every score: nothing found, the response skipped
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "match_close12.npz"))
    cm = ScanMatcher(ctx, d["ranges_ref"].shape[1], float(d["angle_min"]), float(d["angle_inc"]), float(d["max_range"]))
    found, trel, info, resp = cm.closeScanMatchingVSet([(d["ranges_ref"][0], np.zeros(3))], 0, d["ranges_qry"][0], d["guess"][0],
                                                       maxScore=1e-9, covariance_T=T)
    assert not found and trel is None and resp["status"] == 2
    for v in (info, resp["cov"], resp["info"], resp["mean"], resp["mass"], resp["border_mass"]):
        assert np.all(np.isfinite(v)) and not np.any(v)


def test_close_matching_is_unchanged_by_the_response(ctx):
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "match_close12.npz"))
    cm = ScanMatcher(ctx, d["ranges_ref"].shape[1], float(d["angle_min"]), float(d["angle_inc"]), float(d["max_range"]))
    n_found = 0
    for p in range(4):
        scans = [(d["ranges_ref"][p], np.zeros(3))]
        f0, t0 = cm.closeScanMatchingVSet(scans, 0, d["ranges_qry"][p], d["guess"][p])
        f1, t1, info, resp = cm.closeScanMatchingVSet(scans, 0, d["ranges_qry"][p], d["guess"][p], covariance_T=T)
        assert f0 == f1 == bool(d["found"][p])
        if not f0:
            assert t1 is None and resp["status"] == 2
            continue
        n_found += 1
        assert t0.tobytes() == t1.tobytes() == d["xyt"][p].tobytes()
        assert resp["status"] == 0 and resp["n_candidates"] > 0 and np.array_equal(info, resp["info"])
        assert np.allclose(info, info.T, rtol=1e-12, atol=0) and np.all(np.linalg.eigvalsh(info) > 0)
        # the winner is one of the candidates: its own weight is exactly 1
        assert resp["mass"] >= 1.0
    assert n_found >= 2


def _run(ctx, tr, gpu, **kw):
    la = (tr["n_beams"], tr["angle_min"], tr["angle_inc"], tr["max_range"])
    if gpu:
        slam = GraphSLAMDriver(ctx, ScanMatcher(ctx, *la), LCScanMatcher(ctx, *la), **kw)
    else:
        slam = GraphSLAMDriver(OB.OracleContext(), OB.close_matcher(la), OB.lc_matcher(la), **kw)
    run_srslam(slam, tr["odom"], tr["scans"], linearUpdate=0.5)
    return slam


def test_driver_puts_the_response_on_scan_match_edges(ctx, oracle):
    tr = synth.make_trajectory(16, laps=0.04)                    # the smallest run with three scan-match edges
    ref = _run(ctx, tr, False)                                    # today's graph: the same driver on the oracle backend
    assert ref.edge_kind.count("sm") >= 3
    a = _run(ctx, tr, True)                                       # default mode
    assert a.sm_information == "fixed" and a.edge_kind == ref.edge_kind
    np.testing.assert_array_equal(a.g.edge_from, ref.g.edge_from)
    np.testing.assert_array_equal(a.g.edge_to, ref.g.edge_to)
    np.testing.assert_array_equal(a.g.meas, ref.g.meas)
    np.testing.assert_array_equal(a.g.info, ref.g.info)
    assert [l for l in a.log if l[0] != "lcc"] == [l for l in ref.log if l[0] != "lcc"]
    b = _run(ctx, tr, True, sm_information=("response", T))
    sm = [k for k, kind in enumerate(b.edge_kind) if kind == "sm"]
    fallbacks = [l for l in b.log if l[0] == "sm_information_fallback"]
    assert len(sm) >= 3 and len(fallbacks) < len(sm)
    changed = 0
    for k in sm:
        i = b.g.info[k]
        if np.array_equal(i, SM_INFO):
            continue
        changed += 1
        full = np.array([[i[0], i[1], i[2]], [i[1], i[3], i[4]], [i[2], i[4], i[5]]])
        assert np.all(np.isfinite(full)) and np.all(np.linalg.eigvalsh(full) > 0)
    assert changed == len(sm) - len(fallbacks) >= 3
    with pytest.raises(ValueError):
        GraphSLAMDriver(ctx, None, None, sm_information=("response", 0.0))
