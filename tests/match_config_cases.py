"""Test infrastructure: the cases that take the response (k_match_response), the refinement (k_match_refine) and the polish
(k_match_polish) away from the three grids their own tests run on, and ONE builder per family that returns what the
device call needs plus the float64 yardstick's result (tests/ref_match_response.py, ref_match_refine.py,
ref_match_polish.py).  Not imported by anything under ``cg_mrslam_amd/``; imports nothing from there but ``synth`` for scans.
Every builder's result is computed once per session (``_CACHE``) and never changed.

Family A  generic calls on the room scene of ref_match_refine.named_cases (the room seen from a pose between the grid's
          nodes, every second point, noise of sigma 0.01 with seed 7, theta resolution 0.02, half-widths R.HALF, the winner
          row 0 of ``R.candidates``), one entry of ``A_CASES`` per property the three grids of the existing tests share.
Family B  more query points than one kept-point list holds: the construction of
          test_greedy_with_more_query_points_than_one_list_holds with the oracle's primitives, on the loop-closure grid.
Family C  close matches composed as ``matcher_configs._search`` composes them, at four entries of ``matcher_configs.CONFIGS``,
          and one two-scan reference set.
Family D  the room seen from ``ref_match_polish.LC_TRUE`` on the three grids of ``matcher_configs.GENERIC``, the winner by the
          oracle's search over scanMatchingLC's region.

Seeds and corners.  No seed and no corner of a case of families A to D as they were first listed was changed: with the border
diagnostic of ref_match_refine every one of them meets the conditions of tests/test_match_configs_cpu.py as named.  Two things
were chosen here and not taken from that list:
- `edge_out_k100` was added to family A beyond the original case list: the refinement's own fill value (fill / kscale) is read
  only by a point beyond the border, and every case with such a point had kscale 128.
- The pair of scans behind family D's scan form (``family_d_scans``: scanMatchingLC takes scans, not points) was picked for
  fairness by the yardstick's own diagnostics: pair 0 of seed 77, decision margin 2.4e-7 on all three grids.  Pair 0 of seed 90,
  the first pair tried, leaves 3.5e-12 on two grids, below the condition of 1e-11.
"""
import numpy as np

from cg_mrslam_amd import synth

import matcher_configs as MC
import ref_match_polish as RP
import ref_match_refine as RR
import ref_match_response as R

T = 0.01                                                      # the temperature of every response here
MAX_SCORE = 0.15                                              # family C: closeScanMatching's default bound
UNSYM_ODD = ((-4.35, -2.65), (5.0, 3.0), 0.05, 0.2, 128)
_ROOM = dict(theta_res=R.THETA_RES, half=R.HALF, true=RR.TRUE_POSE, centre=(0.0, 0.0, 0.0), step=None, stop=1)


def _a(grid, cells, n_cands, why, **kw):
    return dict(_ROOM, grid=grid, cells=cells, n_cands=n_cands, why=why, **kw)


# name -> grid (ll, ur, resolution, kernel_range, kscale), the field's cell counts, the candidates of the region, the stop code the
# yardstick's refinement ends with, and what the entry is there for
A_CASES = {
    "unsym_odd": _a(UNSYM_ODD, (187, 113), 256, "not square, no multiple of 8, corners that no float represents"),
    "radius_10": _a(((-5.0, -5.0), (5.0, 5.0), 0.05, 0.5, 128), (200, 200), 256, "radius 10 cells: the stamping rasteriser, fill 64"),
    "kscale_100": _a(((-5.0, -5.0), (5.0, 5.0), 0.05, 0.2, 100), (200, 200), 256, "fill 20, 1 / 100 is no power of two"),
    "res_004": _a(((-5.0, -5.0), (5.0, 5.0), 0.04, 0.2, 128), (250, 250), 400, "250 x 250 cells, 10 x 10 x 4 candidates", stop=0),
    "edge_in": _a(((-5.0, -5.0), (3.12, 1.08), 0.05, 0.2, 128), (162, 121), 256,
                  "points in the last layer of cells along x and y, one beyond the border along y", stop=2),
    "edge_out": _a(((-5.0, -5.0), (3.07, 1.07), 0.05, 0.2, 128), (161, 121), 256,
                   "the right wall beyond the border along x, points in the last layer along y", stop=2),
    "edge_out_k100": _a(((-5.0, -5.0), (3.07, 1.07), 0.05, 0.2, 100), (161, 121), 256,
                        "`edge_out` with kscale 100: the fill value of the points beyond the border is 20 / 100, not 20 / 128 "
                        "(added beyond the original case list: a point on the grid never reads the refinement's own fill value)", stop=2),
    "step_010": _a(R.GRID, (200, 200), 256, "a step of 0.1 on the 0.05 m grid: (int)(0.1 / (float)0.05) == 1", step=0.1),
    "step_2": _a(UNSYM_ODD, (187, 113), 144, "a step of 0.15: two cells, 6 x 6 x 4 candidates, bound and floor doubled", step=0.15,
                 half=(0.3, 0.3, 0.04)),
    "theta_26": _a(R.GRID, (200, 200), 320, "an angle beyond pi / 4 in the generic calls", true=(RR.TRUE_POSE[0], RR.TRUE_POSE[1], 2.6 - 0.0169),
                   centre=(0.0, 0.0, 2.6)),
}
C_ENTRIES = ("combo_a", "kscale_100", "unsym_odd", "kr_03")
C_PAIRS = (0, 5)
_CACHE = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def border_census(oracle, grid, ref_pts, qry_pts, pose):
    """Where the query points fall under ``pose``, by the border test of the definition: how many sit in the last layer of
    cells along x / along y (inside, with i0 + 1 == nx - 1 / j0 + 1 == ny - 1) and how many beyond the upper border along x /
    along y (u >= nx - 1 / v >= ny - 1)."""
    F, llx, lly, res, _ = RR.field(oracle, grid, ref_pts)
    nx, ny = F.shape
    q = np.asarray(qry_pts, dtype=np.float64).reshape(-1, 2)
    c, s = np.cos(pose[2]), np.sin(pose[2])
    u = ((c * q[:, 0] - s * q[:, 1] + pose[0]) - llx) / res
    v = ((s * q[:, 0] + c * q[:, 1] + pose[1]) - lly) / res
    inside = (u >= 0) & (u < nx - 1) & (v >= 0) & (v < ny - 1)
    return dict(last_x=int(np.count_nonzero(inside & (np.floor(u) == nx - 2))), last_y=int(np.count_nonzero(inside & (np.floor(v) == ny - 2))),
                beyond_x=int(np.count_nonzero(u >= nx - 1)), beyond_y=int(np.count_nonzero(v >= ny - 1)))


# ------------------------------------------------------------------------------------------------------------ family A
def family_a(oracle, name):
    """dict(grid, theta_res, step, half, ref, qry, region, cands, winner, refine, response, polish): ``response`` over ``region``,
    ``polish`` the yardstick's {"response", "refined"} with the response over the window of ``half`` around the winner.  For
    `step_2` also ``clipped``, the refinement under bound_steps = 0.25; for `unsym_odd` also ``moved`` and ``polish_moved``."""
    def make():
        c = A_CASES[name]
        room = R.room()
        seen = RR.seen_from(room, c["true"])[::2]
        qry = seen + np.random.default_rng(7).normal(0, 0.01, size=seen.shape)
        region = R.region_around(c["centre"], c["half"])
        cands = R.candidates(oracle, c["grid"], room, qry, region, c["theta_res"], c["step"])
        _frozen(room, qry, region, cands)
        winner = cands[0].copy()
        out = dict(grid=c["grid"], theta_res=c["theta_res"], step=c["step"], half=c["half"], ref=room, qry=qry, region=region, cands=cands,
                   winner=winner, refine=RR.refine(oracle, c["grid"], room, qry, c["theta_res"], winner, None, c["step"]),
                   response=R.response(cands, winner, T, c["grid"], c["theta_res"], c["step"]))
        # through the polish the response is taken over the window around the winner, not over `region`
        out["polish"] = RP.polish(oracle, c["grid"], room, qry, c["theta_res"], [winner], T=T, window=c["half"], refine={}, step=c["step"])[0]
        if name == "step_2":
            out["clipped"] = RR.refine(oracle, c["grid"], room, qry, c["theta_res"], winner, dict(bound_steps=0.25), c["step"])
        if name == "unsym_odd":                                   # the mixed batch's second winner: moved by one search step in x
            moved = winner.copy()
            moved[0] += float(np.float32(c["grid"][2]))
            out["moved"] = moved
            out["polish_moved"] = RP.polish(oracle, c["grid"], room, qry, c["theta_res"], [moved], T=T, window=c["half"], refine={})[0]
        return out
    return _once(("A", name), make)


# ------------------------------------------------------------------------------------------------------------ family B
def family_b(oracle):
    """dict(grid, theta_res, half, ref, qry, search_region, n_search, winner, region, polish): ``polish`` is the yardstick's
    {"response", "refined"} for the winner at T, RP.LC_WINDOW and the default refinement; ``region`` the window's region."""
    def make():
        sp = synth.make_scan_pairs(6, seed=93)
        la = (sp["angle_min"], sp["angle_inc"], sp["max_range"])
        ref = oracle.cartesian(sp["ranges_ref"][0], *la)
        rng = np.random.default_rng(2)
        parts = [oracle.cartesian(sp["ranges_qry"][p], *la) + rng.uniform(-0.05, 0.05, size=2) for p in range(6)]
        qry = oracle.subsample(np.concatenate(parts), 0.1)
        search_region = R.region_around(sp["guess"][0], (0.5, 0.5, 0.1))
        cands = R.candidates(oracle, RP.LC_GRID, ref, qry, search_region, RP.LC_THETA_RES)
        winner = cands[0].copy()
        _frozen(ref, qry, search_region, winner)
        pol = RP.polish(oracle, RP.LC_GRID, ref, qry, RP.LC_THETA_RES, [winner], T=T, window=RP.LC_WINDOW, refine={})[0]
        return dict(grid=RP.LC_GRID, theta_res=RP.LC_THETA_RES, half=RP.LC_WINDOW, ref=ref, qry=qry, search_region=search_region,
                    n_search=len(cands), winner=winner, region=RP.window_region(winner, RP.LC_WINDOW), polish=pol)
    return _once(("B",), make)


# ------------------------------------------------------------------------------------------------------------ family C
def _composed(oracle, cfg, ref_pts, ranges_qry, guess, expected):
    """The response and the refinement behind closeScanMatching, composed of the oracle's primitives on the points and the
    window ``matcher_configs._search`` forms."""
    found, win, _ = expected
    grid = (cfg["ll"], cfg["ur"], cfg["resolution"], cfg["kernel_range"], cfg["kscale"])
    q = oracle.cartesian(ranges_qry, cfg["angle_min"], cfg["angle_inc"], cfg["max_range"], cfg["min_range"])
    q = oracle.apply_transf(cfg["laser_pose"], oracle.subsample(q, cfg["subsample_res"]))
    w = cfg["win"]
    region = np.array([-w[0] + guess[0], -w[1] + guess[1], -w[2] + guess[2], w[0] + guess[0], w[1] + guess[1], w[2] + guess[2]],
                      dtype=np.float32)
    out = dict(cfg=cfg, grid=grid, found=found, expected=win.copy(), half=w, ref=ref_pts, qry=q, region=region, guess=np.array(guess))
    if found:
        cands = R.candidates(oracle, grid, ref_pts, q, region, cfg["theta_res"], cap=65536)
        out.update(cands0=cands[0].copy(), response=R.response(cands, win, T, grid, cfg["theta_res"]),
                   refine=RR.refine(oracle, grid, ref_pts, q, cfg["theta_res"], win))
    _frozen(ref_pts, q, region)
    return out


def family_c_scans():
    return _once(("C", "scans"), lambda: synth.make_scan_pairs(12, seed=77))


def family_c(oracle, name, pair):
    """dict(cfg, grid, found, expected (x, y, theta, score of matcher_configs.expected_close), cands0, half, ref, qry, region, guess,
    ranges_ref, ranges_qry, response, refine) for one pair of ``synth.make_scan_pairs(12, seed=77)`` at an entry of CONFIGS."""
    def make():
        sp = family_c_scans()
        cfg = MC.full_config(name, sp)
        rr, rq, g = sp["ranges_ref"][pair], sp["ranges_qry"][pair], sp["guess"][pair]
        ref = oracle.apply_transf(cfg["laser_pose"], oracle.cartesian(rr, cfg["angle_min"], cfg["angle_inc"], cfg["max_range"], cfg["min_range"]))
        out = _composed(oracle, cfg, ref, rq, g, MC.expected_close(oracle, cfg, rr, rq, g, MAX_SCORE))
        return dict(out, ranges_ref=rr, ranges_qry=rq)
    return _once(("C", name, pair), make)


def family_c_vset(oracle, name="combo_a"):
    """The same for a reference set of two scans along a trajectory, the later one the origin vertex: also ``scans`` (the
    [(ranges, pose relative to the origin)] list of the device call), ``origin_index`` and ``ranges_qry``."""
    def make():
        tr = synth.make_trajectory(43, seed=77, laps=0.35)
        cfg = MC.full_config(name, tr)
        last = 8
        org = tr["odom"][last]
        rel = [synth.se2_compose(synth.se2_inverse(org), tr["odom"][last - 2]), np.zeros(3)]
        sets = [tr["scans"][last - 2], tr["scans"][last]]
        rq = tr["scans"][last + 2]
        g = synth.se2_compose(synth.se2_inverse(org), tr["odom"][last + 2])
        ref = MC.vset_points(oracle, cfg, sets, rel)              # (the points expected_close_vset itself searches)
        out = _composed(oracle, cfg, ref, rq, g, MC.expected_close_vset(oracle, cfg, sets, rel, rq, g, MAX_SCORE))
        return dict(out, scans=[(sets[k], np.asarray(rel[k], dtype=np.float64)) for k in range(2)], origin_index=1, ranges_qry=rq)
    return _once(("C", "vset", name), make)


# ------------------------------------------------------------------------------------------------------------ family D
def family_d(oracle, name):
    """dict(grid, theta_res, half, ref, qry, search_region, n_search, winner, polish) on ``matcher_configs.GENERIC[name]``.  The
    search over scanMatchingLC's region has 78 000 candidates at `radius_10`'s 0.05 m: the list is taken with a larger cap, the
    region stays whole (it is the region the device's own search covers)."""
    def make():
        grid = MC.GENERIC[name]
        room = R.room()
        seen = RR.seen_from(room, RP.LC_TRUE)[::2]
        qry = seen + np.random.default_rng(7).normal(0, 0.01, size=seen.shape)
        search_region = R.region_around((0.0, 0.0, 0.0), RP.LC_SEARCH_HALF)
        cands = R.candidates(oracle, grid, room, qry, search_region, RP.LC_THETA_RES, cap=131072)
        winner = cands[0].copy()
        _frozen(room, qry, search_region, winner)
        pol = RP.polish(oracle, grid, room, qry, RP.LC_THETA_RES, [winner], T=T, window=RP.LC_WINDOW, refine={})[0]
        return dict(grid=grid, theta_res=RP.LC_THETA_RES, half=RP.LC_WINDOW, ref=room, qry=qry, search_region=search_region,
                    n_search=len(cands), winner=winner, polish=pol)
    return _once(("D", name), make)


D_SCAN_MAX_SCORE = 0.15


def family_d_scans(oracle, name):
    """scanMatchingLC's own input on ``matcher_configs.GENERIC[name]``: pair 0 of family C's scans as two single-scan sets.
    (Chosen by the yardstick's own diagnostics: of three pairs each of the seeds 90, 91, 92 and 77 it is the one whose refinement
    keeps the largest decision margin on all three grids, 2.4e-7; pair 0 of seed 90, the pair of test_matcher_config_gpu's greedy
    test, leaves 3.5e-12 on two of them, below the condition of 1e-11.)  dict(sp, grid, ref, qry, winners, polish): the points as scan_matcher.cpp:201-294 forms them (the laser at
    the robot's origin), ``winners`` row 0 of each of its two searches that found something (the region of +-(0.5, 1.5, 0.8)
    around the reference scan, then the same turned by pi; result bins (0.5, 0.5, 0.2)) with the search's own angle, ``polish``
    the yardstick per winner."""
    def make():
        sp = family_c_scans()
        grid = MC.GENERIC[name]
        ll, ur, res, kr, ks = grid
        la = (sp["angle_min"], sp["angle_inc"], sp["max_range"])
        ref = oracle.cartesian(sp["ranges_ref"][0], *la)
        qry = oracle.subsample(oracle.cartesian(sp["ranges_qry"][0], *la), 0.1)
        base = R.region_around((0.0, 0.0, 0.0), RP.LC_SEARCH_HALF)
        turned = base.copy()
        turned[2] = np.float32(float(base[2]) + np.pi)
        turned[5] = np.float32(float(base[5]) + np.pi)
        winners = []
        for reg in (base, turned):
            n, r = oracle.greedy_search(ll, ur, res, res, kr, ref, qry, reg.reshape(1, 6), float(np.float32(res)), RP.LC_THETA_RES,
                                        D_SCAN_MAX_SCORE, 0.5, 0.5, 0.2, kscale=ks)
            if n > 0:
                winners.append(r[0].copy())
        _frozen(ref, qry)
        pol = RP.polish(oracle, grid, ref, qry, RP.LC_THETA_RES, winners, T=T, window=RP.LC_WINDOW, refine={})
        return dict(sp=sp, grid=grid, ref=ref, qry=qry, winners=winners, polish=pol)
    return _once(("D", "scans", name), make)


# ------------------------------------------------------------------------------------------------------------ every case
# label -> (family, the builder's arguments, the candidates of its response as the table of the families says: a count or a range)
LABELS = {f"A-{n}": ("A", (n,), A_CASES[n]["n_cands"]) for n in A_CASES}
LABELS["B"] = ("B", (), 10 * 10 * 16)
LABELS.update({f"C-{n}-pair{p}": ("C", (n, p), (14400, 37440)) for n in C_ENTRIES for p in C_PAIRS})
LABELS["C-combo_a-two_scans"] = ("Cv", (), (14400, 37440))
LABELS.update({f"D-{n}": ("D", (n,), 20 * 20 * 16 if n == "radius_10" else 10 * 10 * 17) for n in MC.GENERIC})


def case(oracle, label):
    """(the builder's dict, the yardstick's refinement, the yardstick's response, the stated candidate count or range)."""
    family, args, n = LABELS[label]
    if family == "A":
        c = family_a(oracle, *args)
        return c, c["refine"], c["response"], n
    if family in ("B", "D"):
        c = family_b(oracle) if family == "B" else family_d(oracle, *args)
        return c, c["polish"]["refined"], c["polish"]["response"], n
    c = family_c(oracle, *args) if family == "C" else family_c_vset(oracle)
    assert c["found"], label
    return c, c["refine"], c["response"], n
