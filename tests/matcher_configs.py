"""Test infrastructure: the scan matcher's configurations away from the close default, one per branch of the host's
choice of device code (csrc/matcher_api.cpp: setup_geometry, match_run; csrc/matcher_kernels.hip: match_close_lean_ok,
the v2 test of k_match_close_batch), and ONE way to compute the expected answer of ``closeScanMatching`` for any of
them from the CPU oracle's primitives.  Not imported by anything under ``cg_mrslam_amd/``.

``CONFIGS``: name -> (overrides of the close default, the branch the entry is there to reach, what the host must
choose for it).  The third member holds

  edt     1: the distance-transform rasteriser; 0: the compare-and-swap stamping one (``P.edt``)
  sort32  1: 32-bit subsample sort keys; 0: 64-bit ones (``P.sort32``)
  lean    True: a batch with one workgroup per pair runs the lean kernel instance (``match_close_lean_ok``)
  wide    True: every ordinary pair's window has more than 32 offsets along an axis (redo cause ``window_or_points``)
  slow    True: no pair takes the fast search (build_grid: cell counts that are no multiple of 8, or fill * PT > 255): every
          pair is counted under ``slow_pairs``
  match   True: the entry is meant to match: >= 90 % of the ordinary pairs are found BY THE ORACLE
"""
import math

import numpy as np

# the close default (cgmr_matcher_config_close: graph_slam.cpp:58-59, scan_matcher.cpp:131-151) and the test laser
DEFAULT = dict(ll=(-15.0, -15.0), ur=(15.0, 15.0), resolution=0.025, kernel_range=0.2, kscale=128,
               win=(0.3, 0.3, 0.2), theta_res=0.0125 * .5, bins=(0.5, 0.5, 0.2), subsample_res=0.1, min_range=0.0,
               laser_pose=(0.0, 0.0, 0.0))

_E = dict(edt=1, sort32=1, lean=True, wide=False, match=True, slow=False)


def _e(**kw):
    return dict(_E, **kw)


CONFIGS = {
    # ---- lean kernel still eligible at another size
    "res_005": (dict(resolution=0.05), "600 x 600 cells, 9 x 9 table (K1 6): match_close_lean_ok still true", _e()),
    "unsym_lean": (dict(ll=(-12.1, -9.0), ur=(12.3, 14.0)), "976 x 920 cells: unsymmetric, not square, both multiples of 8: lean", _e()),
    # ---- (nx & 7) / (ny & 7) of match_close_lean_ok
    "res_004": (dict(resolution=0.04), "750 x 750 cells: nx & 7 != 0, 11 x 11 table", _e(slow=True, lean=False)),
    "unsym_odd": (dict(ll=(-12.15, -9.05), ur=(12.3, 14.0)), "978 x 922 cells: nx & 7 and ny & 7 != 0, guesses against each border",
                  _e(slow=True, lean=False)),
    "ny_only_odd": (dict(ll=(-15.0, -15.0), ur=(15.0, 14.9)), "1200 x 1196 cells: only ny & 7 != 0", _e(slow=True, lean=False)),
    "few_tiles": (dict(ll=(-1.0, -0.8), ur=(1.0, 0.9)), "80 x 68 cells (10 x 9 tiles, the last row of tiles half off the grid): "
                  "most points off the grid", _e(slow=True, lean=False, match=False)),
    "tall_directory": (dict(ll=(-17.5, -12.5), ur=(17.5, 12.5)), "1400 x 1000 cells: more than 1200 along x, (ntx + 2) * (nty + 7) = "
                       "23364 <= kMatchMaxDir", _e()),
    # ---- P.edt: radius <= 8 cells
    "kr_03": (dict(kernel_range=0.3), "radius int(0.3 / 0.025) = 11 cells, 23 x 23 table, fill 38: stamping rasteriser", _e(edt=0, lean=False)),
    "radius_8": (dict(kernel_range=0.22), "radius exactly 8 cells with fill 28 (not the default's 25): distance transform", _e()),
    "radius_9": (dict(kernel_range=0.23), "radius exactly 9 cells, fill 29: first radius without the distance transform", _e(edt=0, lean=False)),
    "radius_1": (dict(kernel_range=0.03), "radius 1 cell, 3 x 3 table, fill 3: smallest table with the distance transform", _e(match=False)),
    # ---- kscale (P.fill, the table, 1 / kscale in every score)
    "kscale_64": (dict(kscale=64), "K1 1, fill 12, scores times 1/64", _e()),
    "kscale_100": (dict(kscale=100), "K1 2, fill 20: table and fill change, 1/100 is not a power of two", _e()),
    "kscale_315": (dict(kscale=315), "K1 7, fill 63: the largest fill the fast search takes (fill * PT <= 255)", _e()),
    "kscale_320": (dict(kscale=320), "K1 8, fill 64: fill * PT = 256, every pair takes the generic search", _e(slow=True)),
    "kscale_450": (dict(kscale=450, kernel_range=0.22), "K1 11, fill 99: the largest table values that still fit a signed char "
                   "(11 * sqrt(128) = 124.4)", _e(slow=True)),
    # ---- P.sort32: n_beams < 2048 and max_range / subsample_res < 500
    "sub_005": (dict(subsample_res=0.05), "30 / 0.05 = 600: 64-bit sort keys", _e(sort32=0, lean=False)),
    "sub_006": (dict(subsample_res=0.06), "30 / 0.06 == 500.0: not below 500, 64-bit sort keys", _e(sort32=0, lean=False)),
    "sub_00601": (dict(subsample_res=0.0601), "30 / 0.0601 = 499.17: 32-bit sort keys", _e()),
    # ---- more than 32 offsets along an axis (v2 of k_match_close_batch: ni <= 32 && nj <= 32)
    "wide_x": (dict(win=(0.5, 0.3, 0.2)), "40 +- 1 offsets along x", _e(wide=True)),
    "wide_y": (dict(win=(0.3, 0.5, 0.2)), "40 +- 1 offsets along y", _e(wide=True)),
    "wide_xy": (dict(win=(0.5, 0.45, 0.2)), "40 x 36 offsets", _e(wide=True)),
    "win_0405": (dict(win=(0.405, 0.405, 0.2)), "32 or 33 offsets (the corners are rounded separately): exactly 32 stays, exactly 33 goes", _e()),
    # ---- angle count (kMatchMaxTheta = 80; the host lets (2 win_theta) / theta_res + 2 <= 80 through)
    "theta_00125": (dict(theta_res=0.0125), "32 or 33 angles", _e()),
    "win_theta_024": (dict(win=(0.3, 0.3, 0.24)), "77 or 78 angles", _e()),
    "theta_max": (dict(win=(0.3, 0.3, 0.24375)), "(2 * 0.24375) / 0.00625 + 2 == 80.0: the largest count the host lets through", _e()),
    # ---- result bins (MAXBINS = 128)
    "bins_125": (dict(bins=(0.15, 0.15, 0.1)), "up to 5 x 5 x 5 = 125 bins", _e()),
    "bins_one": (dict(bins=(2.0, 2.0, 1.0)), "bins larger than the window: one bin", _e()),
    # ---- min_range
    "min_range": (dict(min_range=2.5), "beams at or below 2.5 m dropped from both scans", _e()),
    # ---- several at once
    "combo_a": (dict(resolution=0.04, kernel_range=0.3, kscale=64, min_range=0.5, laser_pose=(0.1, -0.05, 0.2)),
                "750 cells, radius 7, fill 19, K1 2, laser off centre", _e(slow=True, lean=False)),
    "combo_b": (dict(resolution=0.05, kernel_range=0.5, ll=(-12.1, -9.0), ur=(12.3, 14.0), subsample_res=0.05, theta_res=0.0125,
                     win=(0.5, 0.4, 0.24), bins=(0.25, 0.25, 0.2), min_range=0.5),
                "488 x 460 cells, radius 10 (stamping), 64-bit keys, 20 x 16 offsets, 39 angles, up to 100 bins", _e(slow=True, edt=0, sort32=0, lean=False)),
    "combo_c": (dict(kscale=100, win=(0.5, 0.3, 0.2), min_range=0.5, laser_pose=(0.12, -0.05, 0.3), bins=(0.3, 0.3, 0.2)),
                "lean-eligible grid, kscale 100, 40 offsets along x, laser off centre", _e(wide=True)),
}

# the entries repeated for the generic searches (greedySearch, hierarchicalSearch, verify), as (ll, ur, resolution, kernel_range, kscale)
GENERIC = {
    "radius_10": ((-20.0, -20.0), (20.0, 20.0), 0.05, 0.5, 128),          # 800 x 800 cells, radius 10: stamping rasteriser
    "unsym_odd": ((-30.3, -21.7), (35.0, 30.0), 0.1, 0.5, 128),           # 653 x 517 cells: not square, no multiple of 8
    "kscale_64": ((-35.0, -35.0), (35.0, 35.0), 0.1, 0.5, 64),            # K1 6, fill 32
}


def full_config(name_or_overrides, sp):
    """The close default with an entry's overrides and the laser of ``synth.make_scan_pairs``' dict."""
    ov = CONFIGS[name_or_overrides][0] if isinstance(name_or_overrides, str) else name_or_overrides
    cfg = dict(DEFAULT, **ov)
    cfg.update(n_beams=sp["n_beams"], angle_min=sp["angle_min"], angle_inc=sp["angle_inc"], max_range=sp["max_range"])
    return cfg


def window_offsets(cfg, guess):
    """(ni, nj): the offsets of closeScanMatching's window along x and y -- both corners narrowed to float and rounded to
    cells separately (scan_matcher.cpp:149-150, gridmap.h world2grid)."""
    f32 = np.float32
    inv = f32(1.0 / f32(cfg["resolution"]))
    out = []
    for a in (0, 1):
        lo = f32(-cfg["win"][a] + guess[a]); hi = f32(cfg["win"][a] + guess[a])
        l = int(np.rint((lo - f32(cfg["ll"][a])) * inv)); h = int(np.rint((hi - f32(cfg["ll"][a])) * inv))
        out.append(max(0, h - l))
    return tuple(out)


def _se2_mul(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    t = a[2] + b[2]
    if not (-math.pi <= t < math.pi):
        t = t - 2 * math.pi * math.floor((t + math.pi) / (2 * math.pi))
    return np.array([a[0] + (c * b[0] - s * b[1]), a[1] + (s * b[0] + c * b[1]), t])


def _search(oracle, cfg, ref_pts, ranges_qry, guess, max_score):
    q = oracle.cartesian(ranges_qry, cfg["angle_min"], cfg["angle_inc"], cfg["max_range"], cfg["min_range"])
    q = oracle.apply_transf(cfg["laser_pose"], oracle.subsample(q, cfg["subsample_res"]))
    w = cfg["win"]
    region = np.array([-w[0] + guess[0], -w[1] + guess[1], -w[2] + guess[2], w[0] + guess[0], w[1] + guess[1], w[2] + guess[2]],
                      dtype=np.float32)
    res = cfg["resolution"]
    n, r = oracle.greedy_search(cfg["ll"], cfg["ur"], res, res, cfg["kernel_range"], ref_pts, q, region, float(np.float32(res)),
                                cfg["theta_res"], max_score, cfg["bins"][0], cfg["bins"][1], cfg["bins"][2], kscale=cfg["kscale"])
    return (True, r[0].copy(), n) if n > 0 else (False, np.zeros(4), 0)


def expected_close(oracle, cfg, ranges_ref, ranges_qry, guess, max_score):
    """``closeScanMatching`` (scan_matcher.cpp:112-189) for one pair with a single-scan reference set, composed of the
    oracle's primitives: (found, mresvec[0] as (x, y, theta, score), len(mresvec))."""
    ref = oracle.cartesian(ranges_ref, cfg["angle_min"], cfg["angle_inc"], cfg["max_range"], cfg["min_range"])
    return _search(oracle, cfg, oracle.apply_transf(cfg["laser_pose"], ref), ranges_qry, guess, max_score)


def vset_points(oracle, cfg, ranges_ref_set, ref_rel):
    """The reference points of a set of several scans (transformPointsFromVSet, scan_matcher.cpp:89-110): ``ref_rel[k]``
    = origin^-1 * v_k, zeros for the origin vertex; every scan goes through (origin^-1 * v_k) * laserPose."""
    parts = []
    for k in range(len(ranges_ref_set)):
        v = oracle.cartesian(ranges_ref_set[k], cfg["angle_min"], cfg["angle_inc"], cfg["max_range"], cfg["min_range"])
        parts.append(oracle.apply_transf(_se2_mul(np.asarray(ref_rel[k], dtype=np.float64), np.asarray(cfg["laser_pose"], dtype=np.float64)), v))
    return np.concatenate(parts)


def expected_close_vset(oracle, cfg, ranges_ref_set, ref_rel, ranges_qry, guess, max_score):
    """The same with a reference set of several scans: the search over ``vset_points``."""
    return _search(oracle, cfg, vset_points(oracle, cfg, ranges_ref_set, ref_rel), ranges_qry, guess, max_score)


def expected_close_batch(oracle, cfg, ranges_ref, ranges_qry, guess, max_score):
    """Arrays in the shape the C ABI returns them: found[P] bool, xyt[P, 3], score[P] (zeros when not found), nres[P]."""
    P = len(ranges_ref)
    found, xyt, score, nres = np.zeros(P, dtype=bool), np.zeros((P, 3)), np.zeros(P), np.zeros(P, dtype=np.int32)
    for p in range(P):
        f, r, n = expected_close(oracle, cfg, ranges_ref[p], ranges_qry[p], guess[p], max_score)
        found[p], xyt[p], score[p], nres[p] = f, r[:3], r[3], n
    return found, xyt, score, nres


def make_pairs(cfg, sp, n_ordinary):
    """The pairs every entry is run on: ``n_ordinary`` ordinary pairs of ``sp`` first, then the edge pairs of
    test_parity_edge_cases placed for this grid, then a guess against each border of the grid."""
    n = n_ordinary
    rr = np.concatenate([sp["ranges_ref"][:n], sp["ranges_ref"][:12]]).copy()
    rq = np.concatenate([sp["ranges_qry"][:n], sp["ranges_qry"][:12]]).copy()
    g = np.concatenate([sp["guess"][:n], sp["guess"][:12]]).copy()
    far = np.float32(cfg["max_range"] - 0.01)
    (lx, ly), (ux, uy) = cfg["ll"], cfg["ur"]
    rr[n + 0] = 100.0                                   # empty reference scan
    rq[n + 1] = 100.0                                   # empty query scan
    rr[n + 2, ::2] = 100.0                              # ragged: every other beam invalid
    rq[n + 3, 100:900] = 0.0                            # zero ranges fail r > min_range
    g[n + 4] += [1.02 * cfg["win"][0], -0.97 * cfg["win"][1], 1.05 * cfg["win"][2]]   # guess off by about the window
    g[n + 5] = [ux - 0.1, ly + 0.05, 3.1]               # window partly off the grid's corner, angle window across pi
    rr[n + 6] = far; rq[n + 6] = far                    # a circle of far points: stamps hang over the border (or lie off the grid)
    rr[n + 7, 1::3] = 0.0; rq[n + 7, ::5] = 100.0       # ragged both
    g[n + 8] = [lx + 0.02, 0.5 * (ly + uy), 0.1]        # against the left border
    g[n + 9] = [ux - 0.02, 0.5 * (ly + uy), -0.1]       # the right one
    g[n + 10] = [0.5 * (lx + ux), ly + 0.02, 0.2]       # the lower one
    g[n + 11] = [0.5 * (lx + ux), uy - 0.02, -3.1]      # the upper one, angle window across -pi
    return rr, rq, g
