"""GPU parity of the scan matcher away from its default grid, kernel and window: every entry of
tests/matcher_configs.py -- one per branch of the host's choice of device code -- must be BIT-IDENTICAL to
``closeScanMatching`` composed of the CPU oracle's primitives (matcher_configs.expected_close, anchored on the CPU by
tests/test_oracle_matcher.py), in every call shape, and must have taken the device code it is there for; the limits of
the configuration are rejections with a message, not wrong answers."""
import ctypes as C
import os

import numpy as np
import pytest

import matcher_configs as MC
from cg_mrslam_amd import CgmrError, synth
from cg_mrslam_amd.matcher import ScanMatcher

pytestmark = pytest.mark.gpu

N_ORD = 12                  # ordinary pairs of an entry; 12 edge / border pairs follow (matcher_configs.make_pairs)
N_FULL = 160                # more pairs than half the compute units: one workgroup per pair (P.split == 1)
MAX_SCORE = 0.15
_CACHE = {}


def _sp():
    if "sp" not in _CACHE:
        _CACHE["sp"] = synth.make_scan_pairs(N_ORD, seed=77)
    return _CACHE["sp"]


def _configure(m, cfg):
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


def _matcher(ctx, cfg):
    return _configure(ScanMatcher(ctx, cfg["n_beams"], cfg["angle_min"], cfg["angle_inc"], cfg["max_range"]), cfg)


def _entry(oracle, name):
    """(cfg, pairs, expectation) of an entry: the oracle runs once per distinct pair, every call shape shares it."""
    if name not in _CACHE:
        cfg = MC.full_config(name, _sp())
        rr, rq, g = MC.make_pairs(cfg, _sp(), N_ORD)
        _CACHE[name] = (cfg, (rr, rq, g), MC.expected_close_batch(oracle, cfg, rr, rq, g, MAX_SCORE))
    return _CACHE[name]


def _same(got, want, idx=slice(None)):
    assert np.array_equal(got[0], want[0][idx])
    assert np.array_equal(got[1], want[1][idx])
    assert np.array_equal(got[2], want[2][idx])
    if len(got) > 3:
        assert np.array_equal(got[3], want[3][idx])      # populated result bins == the oracle's total result count


@pytest.mark.parametrize("name", list(MC.CONFIGS))
def test_table_entry_is_bit_identical_in_every_call_shape_and_takes_its_path(ctx, oracle, name):
    cfg, (rr, rq, g), want = _entry(oracle, name)
    flags = MC.CONFIGS[name][2]
    if flags["match"]:
        assert want[0][:N_ORD].mean() >= 0.9, want[0][:N_ORD]          # (on the oracle's answer: the parity is not about nothing)
    m = _matcher(ctx, cfg)
    # ---- single calls: 16 workgroups share the pair
    for i in (0, 5, N_ORD + 5, N_ORD + 6):
        for nres in (False, True):
            _same(m.closeScanMatching(rr[i], rq[i], g[i], maxScore=MAX_SCORE, want_nresults=nres), want, slice(i, i + 1))
            st = m.last_stats()
            assert st["launch"]["split"] == 16 and st["launch"]["lean"] == 0 and st["redo_pairs"] == 0, st
    # ---- a handful: several workgroups per pair
    for nres in (False, True):
        _same(m.closeScanMatching(rr, rq, g, maxScore=MAX_SCORE, want_nresults=nres), want)
        st = m.last_stats()
        assert 1 < st["launch"]["split"] < 16 and st["launch"]["lean"] == 0 and st["redo_pairs"] == 0, st
        assert st["launch"]["edt"] == flags["edt"] and st["launch"]["sort32"] == flags["sort32"], st
        assert not flags["slow"] or st["slow_pairs"] == len(rr), st
    # ---- a full batch: one workgroup per pair, the only shape the lean instance can be chosen for
    # launch["edt"] and launch["sort32"] are what the HOST chose (P.edt, P.sort32).  What the device then does is not observed
    # directly: build_grid still stamps a pair whose tiles do not fit LDS although P.edt is set; that an entry with edt == 0
    # really took the stamping rasteriser is known from the code alone (build_grid: `edt = P.edt && ..`), and that its grid is
    # right from the parity.
    idx = np.random.default_rng(3).permutation(np.arange(N_FULL) % len(rr))
    offs = np.array([MC.window_offsets(cfg, g[i]) for i in idx]).max(axis=1)
    n_ord_wide = int(((offs > 32) & (idx < N_ORD)).sum())
    n_edge = int((idx >= N_ORD).sum())
    for nres in (False, True):
        _same(m.closeScanMatching(rr[idx], rq[idx], g[idx], maxScore=MAX_SCORE, want_nresults=nres), want, idx)
        st = m.last_stats()
        print(name, "exhaustive" if nres else "pruned", st, "ordinary pairs with > 32 offsets:", n_ord_wide)
        la = st["launch"]
        assert la["split"] == 1 and la["edt"] == flags["edt"] and la["sort32"] == flags["sort32"], st
        assert la["lean"] == (1 if flags["lean"] else 0), st
        assert st["pairs"] == N_FULL
        by = st["redo_by_cause"]
        assert not flags["slow"] or st["slow_pairs"] == N_FULL, st
        if not flags["lean"]:
            assert st["redo_pairs"] == 0 and sum(by.values()) == 0, st          # the general kernel ran alone
        elif flags["slow"]:
            assert st["redo_pairs"] == N_FULL and sum(by.values()) == N_FULL, st     # the lean instance keeps no pair
        elif flags["wide"]:
            # every pair goes back to the general kernel, every ordinary one for its window; an edge pair may be counted for
            # its grid instead (an empty reference scan, far points off the grid: the cause is the first that applies), so the
            # split between the two causes is pinned for the ordinary pairs only
            assert n_ord_wide == N_FULL - n_edge
            assert st["redo_pairs"] == N_FULL and sum(by.values()) == N_FULL and by["window_or_points"] >= n_ord_wide, st
        else:
            # the lean instance's usual counts: it keeps the ordinary pairs (all but those whose window is wider than 32
            # offsets) and hands on at most those and the edge pairs
            assert by["window_or_points"] >= n_ord_wide and st["redo_pairs"] <= n_ord_wide + n_edge, st
            assert name != "win_0405" or 0 < n_ord_wide < N_FULL - n_edge


VSET_ENTRIES = ("kr_03", "res_004", "kscale_100", "combo_b")


@pytest.mark.parametrize("name", VSET_ENTRIES)
def test_device_pointer_entry_point_at_table_entries(ctx, oracle, name):
    import torch
    cfg, (rr, rq, g), want = _entry(oracle, name)
    m = _matcher(ctx, cfg)
    dev = torch.device("cuda", 0)
    idx = np.random.default_rng(4).permutation(np.arange(N_FULL) % len(rr))
    for sel in (np.arange(len(rr)), idx):
        P = len(sel)
        d_r, d_q, d_g = (torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev) for a in (rr, rq, g))
        for nres in (False, True):
            d_x = torch.full((P, 3), 7.0, dtype=torch.float64, device=dev)
            d_s = torch.full((P,), 7.0, dtype=torch.float64, device=dev)
            d_f = torch.full((P,), 7, dtype=torch.uint8, device=dev)
            d_n = torch.full((P,), 7, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            m.closeScanMatching_dev(d_r.data_ptr(), d_q.data_ptr(), d_g.data_ptr(), P, d_x.data_ptr(), d_s.data_ptr(), d_f.data_ptr(),
                                    maxScore=MAX_SCORE, d_nres=d_n.data_ptr() if nres else 0)
            torch.cuda.synchronize()
            got = (d_f.cpu().numpy().astype(bool), d_x.cpu().numpy(), d_s.cpu().numpy()) + ((d_n.cpu().numpy(),) if nres else ())
            _same(got, want, sel)


def _vsets(n_sets):
    """Reference sets of three scans along a trajectory (the last vertex is the origin), the next key frame as the current scan."""
    tr = synth.make_trajectory(40 + 3 * n_sets, seed=77, laps=0.35)
    ref, rel, cur, guess = [], [], [], []
    for k in range(n_sets):
        last = 8 + 3 * k
        idx = [last - 4, last - 2, last]
        org = tr["odom"][last]
        ref.append(np.stack([tr["scans"][i] for i in idx]))
        rel.append(np.stack([np.zeros(3) if i == last else synth.se2_compose(synth.se2_inverse(org), tr["odom"][i]) for i in idx]))
        cur.append(tr["scans"][last + 2])
        guess.append(synth.se2_compose(synth.se2_inverse(org), tr["odom"][last + 2]))
    return np.stack(ref), np.stack(rel), np.stack(cur), np.stack(guess)


@pytest.mark.parametrize("name", VSET_ENTRIES)
def test_multi_scan_reference_sets_at_table_entries(ctx, oracle, name):
    """closeScanMatchingVSetBatch with three-scan reference sets (the cell-bitmap path of the rasteriser): the expectation is
    composed the same way over the set's points (matcher_configs.expected_close_vset)."""
    if "vsets" not in _CACHE:
        _CACHE["vsets"] = _vsets(10)
    ref, rel, cur, guess = (a.copy() for a in _CACHE["vsets"])
    cfg = MC.full_config(name, _sp())
    ref[7, 1] = 0.0                                                  # a set padded with a scan without a valid beam
    cur[8] = 100.0                                                   # an empty current scan
    ref[9] = cfg["max_range"] - 0.01                                 # far points in every scan of the set
    guess[6] = [cfg["ur"][0] - 0.05, cfg["ll"][1] + 0.05, 3.1]       # window off the corner, across pi
    want = [MC.expected_close_vset(oracle, cfg, ref[k], rel[k], cur[k], guess[k], MAX_SCORE) for k in range(len(ref))]
    assert sum(w[0] for w in want[:6]) >= 5
    m = _matcher(ctx, cfg)
    idx = np.random.default_rng(5).permutation(np.arange(N_FULL) % len(ref))
    for sel in (np.arange(len(ref)), np.array([2]), idx):
        f, x, s = m.closeScanMatchingVSetBatch(ref[sel], rel[sel], cur[sel], guess[sel], MAX_SCORE)
        st = m.last_stats()
        assert st["launch"]["lean"] == 0 and st["redo_pairs"] == 0 and st["launch"]["edt"] == MC.CONFIGS[name][2]["edt"], st
        assert np.array_equal(f, np.array([want[k][0] for k in sel]))
        assert np.array_equal(x, np.array([want[k][1][:3] for k in sel])) and np.array_equal(s, np.array([want[k][1][3] for k in sel]))


# ----------------------------------------------------------------------- generic searches at three other configurations

def _generic_matcher(ctx, sp, name):
    ll, ur, res, kr, ks = MC.GENERIC[name]
    m = ScanMatcher(ctx, sp["n_beams"], sp["angle_min"], sp["angle_inc"], sp["max_range"], resolution=res, kernel_range=kr)
    m.initializeGrid(ll, ur, res)
    m.cfg.kscale = ks
    return m


@pytest.mark.parametrize("name", list(MC.GENERIC))
def test_greedy_search_with_one_to_nine_regions_at_other_configurations(ctx, oracle, name):
    ll, ur, res, kr, ks = MC.GENERIC[name]
    sp = synth.make_scan_pairs(2, seed=90)
    m = _generic_matcher(ctx, sp, name)
    ref = m.cartesian(sp["ranges_ref"][0])
    q = m.subsample(m.cartesian(sp["ranges_qry"][0]))
    g = sp["guess"][0]
    base = np.array([-.5 + g[0], -1.5 + g[1], -.8 + g[2], .5 + g[0], 1.5 + g[1], .8 + g[2]])
    rng = np.random.default_rng(0)
    for nreg in (1, 3, 9):
        regs = np.array([base + np.tile(rng.uniform(-0.4, 0.4, 3), 2) for _ in range(nreg)], dtype=np.float32)
        regs[0] = base
        got = m.greedySearch(ref, q, regs, 0.025, 0.3, 0.5, 0.5, 0.2)
        n, want = oracle.greedy_search(ll, ur, res, res, kr, ref, q, regs, float(np.float32(res)), 0.025, 0.3, 0.5, 0.5, 0.2, kscale=ks)
        assert len(got) == n > 0
        assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(MC.GENERIC))
def test_hierarchical_search_on_the_device_loop_and_level_by_level_at_other_configurations(ctx, oracle, name):
    """(levels, maxScore) as in test_level_loop_on_the_device_and_level_by_level: the last one has more than 256 results on a
    level, which outgrows the device tables and is served level by level."""
    ll, ur, res, kr, ks = MC.GENERIC[name]
    sp = synth.make_scan_pairs(2, seed=77)
    m = _generic_matcher(ctx, sp, name)
    ref = m.cartesian(sp["ranges_ref"][0])
    q = m.subsample(m.cartesian(sp["ranges_qry"][0]))
    region = np.array([[-3, -2, np.float32(-np.pi), 3, 2, np.float32(np.pi)]], dtype=np.float32)
    counts = {}
    for levels, max_score in ((2, 0.2), (4, 0.25), (3, 0.45)):
        got = m.hierarchicalSearch(ref, q, region, 0.025, max_score, 0.5, 0.5, 0.2, levels)
        n, want = oracle.hierarchical_search(ll, ur, res, res, kr, ref, q, region, 0.025, max_score, 0.5, 0.5, 0.2, levels, kscale=ks)
        assert len(got) == n and np.array_equal(got, want), (levels, max_score, len(got), n)
        counts[(levels, max_score)] = n
    assert counts[(2, 0.2)] > 0 and 256 < counts[(3, 0.45)] <= 4096, counts


@pytest.mark.parametrize("name", list(MC.GENERIC))
def test_global_matching_at_other_configurations(ctx, oracle, name):
    """globalMatching (scan_matcher.cpp:366-428: +-(10, 5, pi) around the reference vertex, four hierarchy levels, the best
    result) against the oracle's hierarchical search on the oracle's own points: found on both sides, the same transform."""
    ll, ur, res, kr, ks = MC.GENERIC[name]
    region = np.array([[-10, -5, np.float32(-np.pi), 10, 5, np.float32(np.pi)]], dtype=np.float32)
    for seed, pairs, must_find in ((91, (0, 1), True), (77, (0,), name == "radius_10")):
        sp = synth.make_scan_pairs(2, seed=seed)
        m = _generic_matcher(ctx, sp, name)
        for p in pairs:
            ref = oracle.cartesian(sp["ranges_ref"][p], sp["angle_min"], sp["angle_inc"], sp["max_range"])
            q = oracle.subsample(oracle.cartesian(sp["ranges_qry"][p], sp["angle_min"], sp["angle_inc"], sp["max_range"]), 0.1)
            n, want = oracle.hierarchical_search(ll, ur, res, res, kr, ref, q, region, 0.025, 0.2, 0.5, 0.5, 0.2, 4, kscale=ks)
            assert (n > 0) == must_find, (name, seed, p, n)       # (on the oracle: the 0.8 m first level of a 0.1 m grid finds nothing for seed 77)
            ok, trel = m.globalMatching([(sp["ranges_ref"][p], np.zeros(3))], 0, [(sp["ranges_qry"][p], sp["guess"][p])], 0, 0.2)
            assert ok == must_find
            if must_find:
                assert np.array_equal(trel, want[0, :3])


@pytest.mark.parametrize("name", list(MC.GENERIC))
def test_verify_core_at_other_configurations(ctx, oracle, name):
    ll, ur, res, kr, ks = MC.GENERIC[name]
    sp = synth.make_scan_pairs(3, seed=92)
    m = _generic_matcher(ctx, sp, name)
    for p in range(3):
        pts2 = m.cartesian(sp["ranges_ref"][p])
        pts1 = m.applyTransfToScan(sp["true_rel"][p] + [0.4 * p, -0.2 * p, 0.05 * p], m.cartesian(sp["ranges_qry"][p]))
        for (lo, up) in (((-0.3, -0.3), (0.3, 0.3)), ((1.0, -2.0), (1.6, -1.4)), ((ur[0] - 0.2, ur[1] - 0.2), (ur[0] + 0.4, ur[1] + 0.4))):
            lo32, up32 = np.array(lo, dtype=np.float32), np.array(up, dtype=np.float32)
            score, nnm = C.c_double(), C.c_int()
            rc = ctx.lib.cgmr_match_verify(ctx.h, C.byref(m.cfg), C.c_int(len(pts2)), C.c_void_p(pts2.ctypes.data), C.c_int(len(pts1)),
                                           C.c_void_p(np.ascontiguousarray(pts1).ctypes.data), C.c_double(0.3),
                                           C.c_void_p(lo32.ctypes.data), C.c_void_p(up32.ctypes.data), C.byref(score), C.byref(nnm))
            assert rc == 0
            n_o, s_o = oracle.verify(ll, ur, res, res, kr, pts2, pts1, lo32, up32, kscale=ks)
            assert nnm.value == n_o
            assert score.value == s_o or (np.isnan(score.value) and np.isnan(s_o))


# ----------------------------------------------------------------------- one run of the node away from the defaults

def test_two_robot_run_at_resolution_005_kernel_radius_03_matches_oracle_backend(ctx, oracle):
    """cg_mrslam -resolution 0.05 -kernelRadius 0.3 (the close matcher as cg_mrslam.py builds it from its options: 600 cells, radius
    int(0.3 / 0.05) = 5, an 11 x 11 table, fill 38: the device code of res_005 with another table and fill) against the same run on the oracle backend, compared as tests/test_mr_graph_slam_gpu.py compares the default."""
    import oracle_backend as OB
    from ref_condensed import RefRobotGraph
    from test_mr_graph_slam_gpu import _compare
    from cg_mrslam_amd.condensed import RobotGraph
    from cg_mrslam_amd.matcher import LCScanMatcher
    from cg_mrslam_amd.mr_graph_slam import GraphCommSim, MRGraphSLAMDriver, run_cg_mrslam
    team = synth.make_robot_team(2, n_steps=70, laps=0.17, gap=3.0)
    la = (team[0]["n_beams"], team[0]["angle_min"], team[0]["angle_inc"], team[0]["max_range"])
    runs = []
    for gpu in (True, False):
        slams = []
        for r in range(2):
            if gpu:
                close = ScanMatcher(ctx, *la, resolution=0.05, kernel_range=0.3)
                close.initializeGrid((-15, -15), (15, 15), 0.05)
                s = MRGraphSLAMDriver(ctx, close, LCScanMatcher(ctx, *la), RobotGraph(ctx, r, 2), r, 2, windowLoopClosure=5, minInliers=4)
            else:
                octx = OB.OracleContext()
                close = OB.OracleMatcher(la[1], la[2], la[3], (-15.0, -15.0), (15.0, 15.0), 0.05, 0.3)
                s = MRGraphSLAMDriver(octx, close, OB.lc_matcher(la), RefRobotGraph(octx, r, 2), r, 2, windowLoopClosure=5, minInliers=4)
            s.setInterRobotClosureParams(0.15, 3, 5)
            slams.append(s)
        comm = GraphCommSim(slams)
        run_cg_mrslam(slams, team, comm=comm, linearUpdate=0.5)
        runs.append((slams, comm))
    (a, comm_a), (b, comm_b) = runs
    assert comm_a.delivered == comm_b.delivered > 20
    _compare(a, b)
    for s in a:
        kinds = {k: s.edge_kind.count(k) for k in set(s.edge_kind)}
        assert kinds.get("sm", 0) >= 8 and kinds.get("mr", 0) >= 3 and kinds.get("cond", 0) >= 2, kinds


# ----------------------------------------------------------------------- limits are rejections, not wrong answers

def _golden_still_right(ctx):
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "match_close12.npz"))
    m = ScanMatcher(ctx, d["ranges_ref"].shape[1], float(d["angle_min"]), float(d["angle_inc"]), float(d["max_range"]))
    found, xyt, score = m.closeScanMatching(d["ranges_ref"], d["ranges_qry"], d["guess"])
    assert np.array_equal(found, d["found"].astype(bool)) and np.array_equal(xyt, d["xyt"]) and np.array_equal(score, d["score"])


inf, nan = float("inf"), float("nan")
# (overrides just inside the limit or None, overrides just outside, where it is refused)
LIMITS = {
    "bins": (dict(bins=(0.15, 0.15, 0.1)), dict(bins=(0.1, 0.1, 0.05)), "the kernel's error word: 7 x 7 x 9 = 441 > MAXBINS = 128 bins"),
    "angles": (dict(win=(0.3, 0.3, 0.24375)), dict(win=(0.3, 0.3, 0.245)), "match_run: (2 win_theta) / theta_res + 2 = 80.4 > kMatchMaxTheta"),
    "angles_theta_res": (dict(theta_res=0.0125), dict(theta_res=0.005), "match_run: 0.4 / 0.005 + 2 = 82 > kMatchMaxTheta"),
    "directory_resolution": (None, dict(resolution=0.02), "setup_geometry: 1500 x 1500 cells beyond the 1200 x 1200 tile directory"),
    "directory_one_tile": (dict(ll=(-17.5, -12.5), ur=(17.5, 12.5)), dict(ur=(15.04, 15.0)), "setup_geometry: 1201 cells = 151 tiles along x"),
    "signed_char_fill": (None, dict(kscale=640), "make_kernel: int(0.2 * 640) = 128 does not fit a signed char"),
    "signed_char_table": (dict(kscale=450, kernel_range=0.22), dict(kscale=480, kernel_range=0.22),
                          "make_kernel: K1 12 * sqrt(128) = 135.8 does not fit a signed char (fill 105 would)"),
    "table_size": (dict(resolution=0.05, kernel_range=0.75, kscale=64), dict(resolution=0.05, kernel_range=0.8, kscale=64),
                   "make_kernel: radius 16 cells, 33 x 33 > 1024 table entries (radius 15 fits)"),
    "resolution_zero": (None, dict(resolution=0.0), "setup_geometry"), "resolution_negative": (None, dict(resolution=-0.025), "setup_geometry"),
    "resolution_nan": (None, dict(resolution=nan), "setup_geometry"), "resolution_inf": (None, dict(resolution=inf), "setup_geometry"),
    "resolution_denormal": (None, dict(resolution=1e-42), "setup_geometry: 1 / resolution is not finite in float"),
    "theta_res_zero": (None, dict(theta_res=0.0), "match_run"), "theta_res_negative": (None, dict(theta_res=-0.00625), "match_run"),
    "theta_res_nan": (None, dict(theta_res=nan), "match_run"), "theta_res_inf": (None, dict(theta_res=inf), "match_run"),
    "bin_zero": (None, dict(bins=(0.0, 0.5, 0.2)), "match_run"), "bin_negative": (None, dict(bins=(0.5, -0.5, 0.2)), "match_run"),
    "bin_nan": (None, dict(bins=(0.5, 0.5, nan)), "match_run"), "bin_inf": (None, dict(bins=(inf, 0.5, 0.2)), "match_run"),
    "subsample_zero": (None, dict(subsample_res=0.0), "match_run"), "subsample_negative": (None, dict(subsample_res=-0.1), "match_run"),
    "subsample_nan": (None, dict(subsample_res=nan), "match_run"), "subsample_inf": (None, dict(subsample_res=inf), "match_run"),
    "corners_equal": (None, dict(ll=(-15.0, -15.0), ur=(-15.0, 15.0)), "setup_geometry"),
    "corners_swapped": (None, dict(ll=(15.0, 15.0), ur=(-15.0, -15.0)), "setup_geometry"),
    "corners_nan": (None, dict(ur=(nan, 15.0)), "setup_geometry"),
    "kscale_zero": (None, dict(kscale=0), "setup_geometry"),
    "window_nan": (None, dict(win=(nan, 0.3, 0.2)), "match_run"),
}


@pytest.mark.parametrize("name", list(LIMITS))
def test_a_configuration_beyond_a_limit_is_refused_and_the_context_stays_good(ctx, oracle, name):
    inside, outside, _ = LIMITS[name]
    sp = _sp()
    rr, rq, g = sp["ranges_ref"][:4], sp["ranges_qry"][:4], sp["guess"][:4]
    if inside is not None:
        cfg = MC.full_config(inside, sp)
        _same(_matcher(ctx, cfg).closeScanMatching(rr, rq, g, maxScore=MAX_SCORE, want_nresults=True),
              MC.expected_close_batch(oracle, cfg, rr, rq, g, MAX_SCORE))
    m = _matcher(ctx, MC.full_config(outside, sp))
    for call in (lambda: m.closeScanMatching(rr, rq, g), lambda: m.closeScanMatching(rr[0], rq[0], g[0], want_nresults=True)):
        with pytest.raises(CgmrError) as e:
            call()
        assert e.value.code == -1 and len(str(e.value)) > 10, e.value        # CGMR_E_INVALID, with a message
    _golden_still_right(ctx)


def test_too_many_beams_are_refused(ctx, oracle):
    sp = _sp()
    for nb, ok in ((1088, True), (1089, False)):
        r = np.full((2, nb), 4.0, dtype=np.float32)
        m = ScanMatcher(ctx, nb, sp["angle_min"], sp["angle_inc"], sp["max_range"])
        if ok:
            sp2 = synth.make_scan_pairs(3, seed=77, n_beams=nb)
            cfg = MC.full_config({}, sp2)
            m2 = _matcher(ctx, cfg)
            _same(m2.closeScanMatching(sp2["ranges_ref"], sp2["ranges_qry"], sp2["guess"], maxScore=MAX_SCORE, want_nresults=True),
                  MC.expected_close_batch(oracle, cfg, sp2["ranges_ref"], sp2["ranges_qry"], sp2["guess"], MAX_SCORE))
            assert m.closeScanMatching(r, r, np.zeros((2, 3)))[0].all()
        else:
            with pytest.raises(CgmrError) as e:
                m.closeScanMatching(r, r, np.zeros((2, 3)))
            assert e.value.code == -1 and "n_beams" in str(e.value)
    _golden_still_right(ctx)


def test_non_finite_max_score_and_laser_ranges_are_refused(ctx):
    """match_run: the pruned search turns maxScore into an integer bound per angle and the beams are compared with max_range and
    min_range: a value that is not finite is refused (a caller who wants every candidate accepted passes a large finite maxScore,
    as test_parity_scores_and_laser_pose does with 5.0)."""
    sp = _sp()
    rr, rq, g = sp["ranges_ref"][:3], sp["ranges_qry"][:3], sp["guess"][:3]
    m = _matcher(ctx, MC.full_config({}, sp))
    for ms in (inf, -inf, nan):
        with pytest.raises(CgmrError) as e:
            m.closeScanMatching(rr, rq, g, maxScore=ms)
        assert e.value.code == -1
    for field in ("max_range", "min_range"):
        for v in (inf, nan):
            m = _matcher(ctx, MC.full_config({}, sp))
            setattr(m.cfg, field, v)
            with pytest.raises(CgmrError) as e:
                m.closeScanMatching(rr, rq, g)
            assert e.value.code == -1
    _golden_still_right(ctx)


def test_generic_entry_points_refuse_a_bad_grid(ctx):
    sp = _sp()
    pts = np.array([[1.0, 0.0], [1.0, 0.1]])
    reg = np.array([[-0.1, -0.1, -0.05, 0.1, 0.1, 0.05]], dtype=np.float32)
    for ov in (dict(resolution=0.0), dict(resolution=nan), dict(ur=(-15.0, 15.0)), dict(kscale=0), dict(kscale=640), dict(resolution=0.02)):
        m = _matcher(ctx, MC.full_config(ov, sp))
        with pytest.raises(CgmrError):
            m.greedySearch(pts, pts, reg, 0.0125, 0.3, 0.5, 0.5, 0.2, step=0.025)
        with pytest.raises(CgmrError):
            m.hierarchicalSearch(pts, pts, reg, 0.0125, 0.3, 0.5, 0.5, 0.2, 3)
        score, nnm = C.c_double(), C.c_int()
        lo32, up32 = np.array([-0.3, -0.3], dtype=np.float32), np.array([0.3, 0.3], dtype=np.float32)
        rc = ctx.lib.cgmr_match_verify(ctx.h, C.byref(m.cfg), C.c_int(2), C.c_void_p(pts.ctypes.data), C.c_int(2), C.c_void_p(pts.ctypes.data),
                                       C.c_double(0.3), C.c_void_p(lo32.ctypes.data), C.c_void_p(up32.ctypes.data), C.byref(score), C.byref(nnm))
        assert rc == -1
    _golden_still_right(ctx)
