"""Test infrastructure: small maps for the scan ranking and the greedy pruning (cgmr_scan_information, cgmr_scan_prune), one per
way in which the windows, the Delta H pass, the pick or the scratch handling could be wrong.  12 x 12 to 48 x 48 cells, 1 to 7
scans, 1 to 90 beams.  Every entry of ``CASES`` names the gap it is there for (``why``) and carries a predicate (``reach``) that
the tests assert on what tests/ref_scan_info.py makes of it: no case passes vacuously.  Not imported by anything under
``cg_mrslam_amd/``; everything is generated, computed once per session (``resolved``) and never changed.

Every case is a *map* case in the sense of tests/occupancy_cases.py: size, offset and the robot poses as integrateScan gets them.
Unless an entry says otherwise: resolution 0.5, offset (0, 0), laser range 30 = usableRange, maxRange -1, no infinity filling,
gain 3, squareSize 0, laser at the robot's origin; the greedy loop with max_remove = the number of scans, no budget, nothing
protected; the library's default scratch.  The room cases cast their beams against the walls of an axis-aligned box.
"""
import math

import numpy as np

import ref_occupancy as RO
import ref_scan_info as RS

f32 = np.float32
PI = math.pi

_BASE = dict(resolution=0.5, offset=(0.0, 0.0), rows=12, cols=12, first_beam_angle=0.0, angular_step=0.0, laser_max_range=30.0,
             laser_pose=(0.0, 0.0, 0.0), max_range=-1.0, usable_range=30.0, infinity_filling_range=-1.0, gain=3, square_size=0,
             max_remove=None, budget=-1.0, protected=None, info_limit=0, prune_limit=0)

WORKGROUP_CELLS = 1024            # csrc/scan_info_device.h: kSiCellsPerBlock, the window cells one workgroup reduces


def _c(why, reach, poses, scans, **kw):
    return dict(_BASE, why=why, reach=reach, poses=np.array(poses, dtype=np.float64).reshape(-1, 3),
                scans=np.array(scans, dtype=np.float32), **kw)


def _room(poses, n_beams, a0, da, box, scale=None):
    """Ranges of a fan of beams from each pose to the walls of the box (x0, y0, x1, y1) around it; ``scale`` [n]: a factor per scan."""
    out = np.empty((len(poses), n_beams))
    for k, (x, y, t) in enumerate(poses):
        for i in range(n_beams):
            a = t + a0 + i * da
            c, s = math.cos(a), math.sin(a)
            d = [(box[2] - x) / c if c > 1e-9 else (box[0] - x) / c if c < -1e-9 else math.inf,
                 (box[3] - y) / s if s > 1e-9 else (box[1] - y) / s if s < -1e-9 else math.inf]
            out[k, i] = min(d) * (1.0 if scale is None else scale[k])
    return out


# ---------------------------------------------------------------------------------------------------------- reach predicates
def _bytes(r):
    return [RS.window_bytes(h, m) for h, m in r["counts"]]


def _inside(r, cell):
    return RO.is_inside(cell, r["rows"], r["cols"])


def _footprint_inside(r, s):
    cx, cy = r["robot_cells"][s]
    return sum(_inside(r, (cx + a, cy + b)) for a in range(-4, 5) for b in range(-4, 5))


def _reach_one_beam(r):
    return r["scans"].shape == (1, 1) and _footprint_inside(r, 0) == 81 and r["info"]["cells"][0] > 81 and r["info"]["hit_sum"][0] == 3


def _reach_beams_82(r):
    return r["scans"].shape[1] == 82 and _footprint_inside(r, 0) == 81 and r["info"]["hit_sum"][0] > 0


def _reach_half_outside(r):
    w = RS.window(*r["counts"][1])
    ends = [b[0] for b in r["beams"][1] if b is not None]
    return (0 < _footprint_inside(r, 1) < 81 and any(not _inside(r, e) for e in ends) and any(_inside(r, e) for e in ends)
            and w[0] == 0 and r["info"]["cells"][1] > 0)


def _reach_wholly_outside(r):
    return (r["info"]["cells"][2] == 0 and r["info"]["delta"][2] == 0.0 and RS.window(*r["counts"][2]) is None
            and all(c > 0 for c in r["info"]["cells"][:2]))


def _reach_footprint_only(r):
    return (r["infinity_filling_range"] == 0.0 and all(b is None for bs in r["beams"] for b in bs) and r["info"]["hit_sum"].sum() == 0
            and list(r["info"]["miss_sum"]) == [_footprint_inside(r, s) for s in range(len(r["scans"]))] and r["info"]["miss_sum"][0] == 81)


def _reach_square1(r):
    return r["square_size"] == 1 and r["gain"] == 3 and r["hits"].max() >= 6 and r["info"]["hit_sum"][0] % 27 != 0 and (r["hits"] > 0).sum() > 9


def _reach_duplicates(r):
    a, b = r["counts"][1], r["counts"][3]
    first = r["greedy"]["rounds"][0]
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and r["info"]["delta"][1] == r["info"]["delta"][3]
            and first["tie"] == [1, 3] and r["greedy"]["order"][0] == 1)


def _reach_contradiction(r):
    return r["info"]["delta"][-1] < -1e-3 and all(d > 0 for d in r["info"]["delta"][:-1]) and r["greedy"]["order"][0] == len(r["scans"]) - 1


def _reach_wide_window(r):
    return max(_bytes(r)) // 8 > 2 * WORKGROUP_CELLS and min(_bytes(r)) // 8 < WORKGROUP_CELLS


def _reach_protected(r):
    free = RS.greedy(r["counts"], (r["rows"], r["cols"]), len(r["scans"]))
    return (bool(r["protected"][free["order"][0]]) and not any(r["protected"][s] for s in r["greedy"]["order"])
            and len(r["greedy"]["order"]) == len(r["scans"]) - sum(r["protected"]) and r["greedy"]["order"] != free["order"][:len(r["greedy"]["order"])])


def _reach_max_remove_large(r):
    n_cand = len(r["scans"]) - sum(r["protected"])
    return r["max_remove"] > n_cand > 0 and len(r["greedy"]["order"]) == n_cand and all(rd["took"] for rd in r["greedy"]["rounds"])


def _reach_budget(r):
    k = len(r["greedy"]["order"])
    return 1 <= k < len(r["scans"]) - 1 and not r["greedy"]["rounds"][-1]["took"] and r["budget"] > 0 and k < r["max_remove"]


def _reach_max_remove_small(r):
    return len(r["greedy"]["order"]) == r["max_remove"] == 2 < len(r["scans"]) and all(rd["took"] for rd in r["greedy"]["rounds"])


def _overlap(a, b):
    return a is not None and b is not None and not (a[2] < b[0] or b[2] < a[0] or a[3] < b[1] or b[3] < a[1])


def _reach_disjoint(r):
    w = [RS.window(h, m) for h, m in r["counts"]]
    order = r["greedy"]["order"]
    # every round but the last leaves alive scans on both sides: some whose window the taken one overlaps, some it does not
    mixed = 0
    for k, s in enumerate(order[:-1]):
        rest = [_overlap(w[s], w[q]) for q in order[k + 1:]]
        mixed += any(rest) and not all(rest)
    return mixed >= 3 and len(order) == len(w)


def _reach_three_chunks(r):
    b = _bytes(r)
    return len(RS.chunks(b, r["info_limit"])) == 3 and max(b) <= r["info_limit"] < sum(b)


def _reach_prune_alloc(r):
    b = _bytes(r)
    return max(b) <= r["prune_limit"] < sum(b) and len(RS.chunks(b, r["prune_limit"])) >= 2


# ---------------------------------------------------------------------------------------------------------------------- cases
_BOX = (2.0, 2.0, 20.0, 20.0)
_ROOM_POSES = [(5.0, 6.0, 0.3), (9.5, 7.2, 1.9), (14.0, 8.1, -2.6), (15.2, 13.3, 0.7), (10.1, 15.4, 2.2), (6.3, 12.2, -1.1)]
_ROOM_KW = dict(rows=48, cols=48, first_beam_angle=-PI, angular_step=2 * PI / 36)
_ROOM_SCANS = _room(_ROOM_POSES, 36, -PI, 2 * PI / 36, _BOX)
_DUP_POSES = [_ROOM_POSES[0], _ROOM_POSES[1], _ROOM_POSES[2], _ROOM_POSES[1], _ROOM_POSES[4]]
# a wall along the cells x = 12 seen by four scans from the left; the last scan stands outside the map (its footprint too) and
# looks along that wall: its one live beam walks through the very cells the others call occupied
_WALL_POSES = [(3.0, 3.0 + 0.3 * k, 0.0) for k in range(4)]
_WALL_SCANS = _room(_WALL_POSES, 21, -0.6, 0.06, (-50.0, -50.0, 6.0, 50.0))
_ALONG = np.zeros((1, 21))
_ALONG[0, 10] = 9.0
_ISLAND_POSES = [(4.0, 4.0, 0.0), (5.1, 4.6, 0.9), (19.0, 5.0, 2.0), (19.8, 4.1, -0.4), (5.0, 19.0, 1.1), (12.0, 12.0, 0.3), (4.4, 18.2, 2.8)]
_SMALL_POSES = [(2.6, 2.7, 0.2), (3.4, 3.1, 1.3), (2.9, 3.6, -2.0)]

CASES = {
    "one_beam": _c("one scan with one beam: the 81 footprint cells on one thread", _reach_one_beam, [(2.5, 2.5, 0.0)], [[2.5]]),
    "beams_82": _c("82 beams: more beams than footprint cells", _reach_beams_82, [(3.0, 3.0, 0.0)],
                   [[1.0 + 0.02 * i for i in range(82)]], rows=16, cols=16, first_beam_angle=-PI, angular_step=2 * PI / 82),
    "half_outside": _c("a scan half outside the map: a clipped window", _reach_half_outside, [(4.0, 4.0, 0.4), (0.6, 3.0, 0.0)],
                       [[2.0 + 0.1 * i for i in range(12)], [2.5 + 0.05 * i for i in range(12)]], rows=16, cols=16,
                       first_beam_angle=-PI, angular_step=2 * PI / 12),
    "wholly_outside": _c("a scan wholly outside: Delta H == 0, cells == 0, no window", _reach_wholly_outside,
                         [(3.0, 3.0, 0.0), (4.0, 3.5, 1.0), (40.0, 40.0, 0.0)], [[2.0 + 0.1 * i for i in range(8)]] * 2 + [[1.0] * 8],
                         rows=16, cols=16, first_beam_angle=-PI, angular_step=2 * PI / 8),
    "footprint_only": _c("every beam out of range with infinity_filling_range == 0: footprint only", _reach_footprint_only,
                         [(3.0, 3.0, 0.0), (1.0, 4.0, 0.5)], [[40.0] * 5, [31.0, 0.0, -1.0, 30.0, 55.0]], rows=16, cols=16,
                         angular_step=0.5, infinity_filling_range=0.0),
    "square1_gain3": _c("square_size = 1 with gain = 3: stamps that overlap and stamps clipped by the border", _reach_square1,
                        [(3.0, 3.0, 0.0), (4.2, 3.4, 2.0)], _room([(3.0, 3.0, 0.0), (4.2, 3.4, 2.0)], 24, -PI, 2 * PI / 24, (0.2, 0.2, 7.0, 6.4)),
                        rows=16, cols=14, first_beam_angle=-PI, angular_step=2 * PI / 24, square_size=1),
    "duplicates": _c("two identical scans at the same pose: bit-equal Delta H, the lower index first", _reach_duplicates, _DUP_POSES,
                     _room(_DUP_POSES, 36, -PI, 2 * PI / 36, _BOX), **_ROOM_KW),
    "contradiction": _c("a scan that contradicts the others: negative Delta H, taken first", _reach_contradiction,
                        _WALL_POSES + [(6.0, -3.0, PI / 2)], np.vstack([_WALL_SCANS, _ALONG]), rows=24, cols=24, first_beam_angle=-0.6,
                        angular_step=0.06),
    "wide_window": _c("a window wider than one workgroup's share beside one that fits a single one", _reach_wide_window,
                      [(12.0, 12.0, 0.1), (3.0, 3.0, 0.0)], np.vstack([_room([(12.0, 12.0, 0.1)], 90, -PI, 2 * PI / 90, (0.6, 0.9, 23.2, 23.4)),
                                                                        np.full((1, 90), 1.5)]),
                      rows=48, cols=48, first_beam_angle=-PI, angular_step=2 * PI / 90),
    "protected": _c("protected scans: the scan an unprotected loop takes first stays", _reach_protected, _ROOM_POSES, _ROOM_SCANS,
                    protected=[1, 0, 0, 1, 0, 0], **_ROOM_KW),
    "max_remove_large": _c("max_remove larger than the number of candidates: the loop ends for want of one", _reach_max_remove_large,
                           _ROOM_POSES, _ROOM_SCANS, protected=[0, 1, 0, 0, 1, 0], max_remove=40, **_ROOM_KW),
    "max_remove_small": _c("max_remove ends the loop", _reach_max_remove_small, _ROOM_POSES, _ROOM_SCANS, max_remove=2, **_ROOM_KW),
    "budget": _c("a budget that stops the loop mid-way", _reach_budget, _ROOM_POSES, _ROOM_SCANS, budget=75.0, **_ROOM_KW),
    "disjoint": _c("windows that do not overlap the one taken: their Delta H need not be computed again, and must not change",
                   _reach_disjoint, _ISLAND_POSES, _room(_ISLAND_POSES, 16, -PI, 2 * PI / 16, (-50.0, -50.0, 50.0, 50.0)).clip(0, 1) *
                   np.array([[2.0], [2.4], [1.7], [2.2], [1.9], [2.6], [2.1]]), rows=48, cols=48, first_beam_angle=-PI, angular_step=2 * PI / 16),
    "three_chunks": _c("a scratch limit that forces three chunks in cgmr_scan_information", _reach_three_chunks, _ROOM_POSES, _ROOM_SCANS,
                       info_limit=24000, **_ROOM_KW),
    "prune_alloc": _c("a scratch limit under which cgmr_scan_prune cannot hold all windows: CGMR_E_ALLOC", _reach_prune_alloc, _SMALL_POSES,
                      _room(_SMALL_POSES, 12, -PI, 2 * PI / 12, (0.4, 0.3, 5.6, 5.7), scale=[1.0, 0.8, 0.6]), first_beam_angle=-PI, angular_step=2 * PI / 12,
                      prune_limit=1600),
}


# ----------------------------------------------------------------------------------------------------------------- resolving
_CACHE = {}


def config_kw(c):
    return {k: c[k] for k in ("resolution", "offset", "max_range", "usable_range", "infinity_filling_range", "gain", "square_size",
                              "first_beam_angle", "angular_step", "laser_max_range", "laser_pose")}


def resolved(name):
    """The case with what the references make of it: ``counts`` (per scan (hits, misses)), ``info`` (ref_scan_info.information),
    ``greedy`` (ref_scan_info.greedy with the case's max_remove / budget / protected), ``hits`` / ``misses`` (the totals of all
    scans), ``beams`` (ref_occupancy.beam_ends per scan), ``robot_cells``."""
    if name in _CACHE:
        return _CACHE[name]
    c = CASES[name]
    r = dict(c, name=name, case=c)
    r["offset"] = (f32(c["offset"][0]), f32(c["offset"][1]))
    n = len(c["scans"])
    r["max_remove"] = n if c["max_remove"] is None else c["max_remove"]
    r["protected"] = [0] * n if c["protected"] is None else list(c["protected"])
    shape = (c["rows"], c["cols"])
    r["counts"] = RS.scan_counts(c["rows"], c["cols"], c["resolution"], r["offset"], c["scans"], c["poses"], c["first_beam_angle"],
                                 c["angular_step"], c["laser_max_range"], c["laser_pose"], c["max_range"], c["usable_range"],
                                 c["infinity_filling_range"], c["gain"], c["square_size"])
    r["info"] = RS.information(r["counts"], shape)
    r["hits"], r["misses"] = r["info"]["hits"], r["info"]["misses"]
    r["greedy"] = RS.greedy(r["counts"], shape, r["max_remove"], c["budget"], r["protected"])
    r["beams"] = [RO.beam_ends(c["rows"], c["cols"], c["resolution"], r["offset"], ranges, pose, c["first_beam_angle"], c["angular_step"],
                               c["laser_max_range"], c["laser_pose"], c["max_range"], c["usable_range"], c["infinity_filling_range"])[2]
                  for ranges, pose in zip(c["scans"], c["poses"])]
    r["robot_cells"] = [RO.world2map(f32(p[0]), f32(p[1]), r["offset"], f32(c["resolution"])) for p in c["poses"]]
    for k in ("poses", "scans", "hits", "misses"):
        r[k].setflags(write=False)
    _CACHE[name] = r
    return r
