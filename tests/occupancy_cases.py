"""Test infrastructure: small occupancy-map cases, one per way in which the ray casting (k_occ_integrate, k_occ_image), its host
layer (cgmr_occupancy_map) or the Python mirror (Graph2occupancy) could be wrong without the trajectory tests noticing.  Every
entry of ``CASES`` names the gap it is there for (``why``) and carries a predicate (``reach``) that the tests assert: the case
really sits on the equality, takes the branch or crosses the border it is named after, judged on what tests/ref_occupancy.py
decides per beam.  No case passes vacuously, none is filtered out at run time.  Not imported by anything under
``cg_mrslam_amd/``; everything here is generated, computed once per session (``resolved``) and never changed.

Two levels.  A *map* case states the FrequencyMap directly: size, offset and the robot poses as integrateScan receives them
(the tests pin Graph2occupancy's geometry to these, the rest of computeMap runs as it is).  A *graph* case states vertex
estimates, the base angle and the fixed flags; size, offset and transformed poses then come from ref_occupancy.geometry, and
the mirror's own geometry() and map centre must equal them.

Unless an entry says otherwise: resolution 0.5, offset (0, 0), laser range 30 = usableRange, maxRange -1, no infinity
filling, gain 3, squareSize 0, thresholds 0.65 / 0.196 (srslam.cpp:101-108), laser at the robot's origin.  At resolution 0.5
every multiple of 0.25 is an exact float, cosf(0) = 1 and sinf(0) = 0, so the cells below can be worked out by hand.

Hand-worked answers (asserted as literals: ``KNOWN``)
-----------------------------------------------------
`single_beam`   Map 12 x 12, robot (1.25, 1.25, 0), one beam at angle 0 with r = 2.  world2map (frequency_map.h:42-45):
                1.25 / 0.5 = 2.5, a tie, lrint -> 2 (even): start (2, 2).  End point (3.25, 1.25): 6.5 -> 6: end (6, 2).
                Half-away rounding would give (3, 3) and (7, 3).  gridLine: dy = 0 <= dx = 4, cells (2..6, 2), a miss each.
                End inside, not cropped, squareSize 0: hits 3 at (6, 2).  fillRobotPose: the 9 x 9 cells around (2, 2) are
                rows -2..6 x cols -2..6, inside the map rows 0..6 x cols 0..6 = 49 misses.  Misses in all 49 + 5 = 54.
                Image: (6, 2) lies in the footprint too (row 6 = 2 + 4), so it has 2 misses: 3 / (3 + 2) = 0.6, neither > 0.65
                nor < 0.196 -> 255; every other touched cell has fraction 0 < 0.196 -> 0.
`diagonal`      Map 12 x 12, beam angle pi / 4, r = float(2 sqrt 2).  Scan 0 from (1, 1, 0): start (2, 2); the end point is
                (3, 3) up to 3e-7, 6.000001 -> (6, 6).  dy = dx = 4: the x-major branch (dy <= dx), d = 2 dy - dx = 4 >= 0 and
                incr2 = 0, so y steps with every x: (2,2) (3,3) (4,4) (5,5) (6,6).  Scan 1 from (4, 1, pi / 2): the beam points
                along 3 pi / 4, start (8, 2), end (4, 6); start.x > end.x, so gridLineCore walks from the end, (4,6) (5,5) (6,4)
                (7,3) (8,2), and gridLine turns the list round.  Hits 3 at (6, 6) and at (4, 6).  Footprints: rows 0..6 x cols
                0..6 (49) and rows 4..11 x cols 0..6 (56).  Misses 49 + 56 + 5 + 5 = 115.  Both end cells lie in both footprints and on
                their own line: 3 misses, 3 / (3 + 3) = 0.5 -> 255.
`zero_length`   Map 12 x 12, robot (1, 1, 0), r = 0.1: end point 1.1 / 0.5 = 2.2 -> 2: end = start = (2, 2).  dx = dy = 0: one cell,
                one miss; 3 hits on it.  Misses 49 + 1 = 50.  (2, 2): 3 / (3 + 2) = 0.6, neither > 0.65 nor < 0.196 -> 255.
`image_half`    Gain 1, robot (1, 1, 0), r = 4: end (10, 2), outside the footprint, 1 hit and 1 miss: fraction 0.5.  With threshold
                = freeThreshold = 0.5 both comparisons are strict (graph2occupancy.cpp:142-144): the cell stays 255.
`image_075_at`  Gain 3, the same beam: 3 / 4 = 0.75f exactly.  threshold 0.75 -> 255.
`image_075_below`  threshold = nextafter(0.75f, 0) -> 100.

An equivalence worth knowing: on an exact diagonal both branches of gridLineCore visit the same cells (in the y-major branch d
= 2 dx - dy = dx >= 0 and incr2 = 0, so x steps with every y), so ``dy < dx`` in place of ``dy <= dx`` changes the order of
the cells only, never a count.  `diagonal` and `compass_256` pin the cells; no count-based test can tell those two apart.
"""
import math

import numpy as np

import ref_occupancy as RO

f32 = np.float32
PI = math.pi

_MAP = dict(level="map", resolution=0.5, offset=(0.0, 0.0), rows=12, cols=12, first_beam_angle=0.0, angular_step=0.0,
            laser_max_range=30.0, laser_pose=(0.0, 0.0, 0.0), max_range=-1.0, usable_range=30.0, infinity_filling_range=-1.0,
            gain=3, square_size=0, threshold=0.65, free_threshold=0.196)
_GRAPH = dict(_MAP, level="graph", resolution=0.1, rows=0, cols=0, offset=None, usable_range=4.0, angle=PI / 2, fixed=None)


def _m(why, reach, poses, scans, **kw):
    return dict(_MAP, why=why, reach=reach, poses=np.array(poses, dtype=np.float64).reshape(-1, 3),
                scans=np.array(scans, dtype=np.float32), **kw)


def _g(why, reach, poses, scans, **kw):
    return dict(_GRAPH, why=why, reach=reach, poses=np.array(poses, dtype=np.float64).reshape(-1, 3),
                scans=np.array(scans, dtype=np.float32), **kw)


# ------------------------------------------------------------------------------------------------- what the predicates read
def _is_tie(q):
    q = float(q)
    return q - math.floor(q) == 0.5


def _quot(r, pt):
    """The two float quotients world2map rounds, for a float point."""
    res, off = f32(r["resolution"]), r["offset"]
    return (pt[0] - off[0]) / res, (pt[1] - off[1]) / res


def _inside(r, p):
    return RO.is_inside(p, r["rows"], r["cols"])


def _footprint(r, s):
    cx, cy = r["trace"][s]["robot_cell"]
    return [(cx + (c % 9) - 4, cy + (c // 9) - 4) for c in range(81)]          # cell c as the beams of a scan share them out


def _cast(r):
    """(scan, beam index, input range, (end, cropped, range cast, float end point)) of every beam that is not skipped."""
    return [(s, i, r["scans"][s][i], b) for s, t in enumerate(r["trace"]) for i, b in enumerate(t["beams"]) if b is not None]


def _fraction(r, cell):
    h, m = int(r["hits"][cell]), int(r["misses"][cell])
    return f32(h) / f32(h + m)


def _directions(r, s):
    """The (sign dx, sign dy, |dx| ? |dy|) classes of the lines of scan ``s``: '=' an exact diagonal, '>' x-major, '<' y-major."""
    sx, sy = r["trace"][s]["start"]
    out = set()
    for b in r["trace"][s]["beams"]:
        if b is not None:
            dx, dy = b[0][0] - sx, b[0][1] - sy
            out.add((int(np.sign(dx)), int(np.sign(dy)), "=" if abs(dx) == abs(dy) else ">" if abs(dx) > abs(dy) else "<"))
    return out


_AXES = {(1, 0, ">"), (-1, 0, ">"), (0, 1, "<"), (0, -1, "<")}
_DIAGONALS = {(a, b, "=") for a in (1, -1) for b in (1, -1)}
_OCTANTS = {(a, b, o) for a in (1, -1) for b in (1, -1) for o in "<>"}


# ---------------------------------------------------------------------------------------------------------- reach predicates
def _reach_single_beam(r):
    t = r["trace"][0]
    (end, cropped, _, pt), = t["beams"]
    return (all(_is_tie(q) for q in _quot(r, t["start_pt"])) and _is_tie(_quot(r, pt)[0]) and not cropped
            and t["start"] == (2, 2) and end == (6, 2))


def _reach_ties(r):
    qs = [float(q) for t in r["trace"] for q in _quot(r, t["start_pt"])]
    return all(_is_tie(q) for q in qs) and {0.5, 2.5, -0.5, 4.5} <= set(qs) and all(_inside(r, t["start"]) for t in r["trace"])


def _reach_usable_eq(r):
    on = [(i, b) for _, i, rng, b in _cast(r) if rng == f32(r["usable_range"])]
    over = [b for _, _, rng, b in _cast(r) if rng > f32(r["usable_range"])]
    return (len(on) == 1 and not on[0][1][1] and r["hits"][on[0][1][0]] >= r["gain"]
            and len(over) == 1 and over[0][1] and r["hits"][over[0][0]] == 0)


def _reach_max_eq(fill):
    def reach(r):
        mr = f32(r["max_range"])
        on = [i for i, v in enumerate(r["scans"][0]) if v == mr]
        below = [i for i, v in enumerate(r["scans"][0]) if v == np.nextafter(mr, f32(0))]
        beams = r["trace"][0]["beams"]
        if len(on) != 1 or len(below) != 1 or mr <= 0 or beams[below[0]] is None or beams[below[0]][1]:
            return False
        nonpos = [i for i, v in enumerate(r["scans"][0]) if v <= 0]
        if fill:
            return all(beams[i] is not None and beams[i][1] and beams[i][2] == f32(r["infinity_filling_range"]) for i in on + nonpos)
        return all(beams[i] is None for i in on + nonpos) and len(nonpos) == 2
    return reach


def _reach_image_eq(cell, h, m, value):
    def reach(r):
        thr = f32(r["threshold"])
        return (int(r["hits"][cell]), int(r["misses"][cell])) == (h, m) and r["image"][cell] == value and (
            _fraction(r, cell) == thr or np.nextafter(_fraction(r, cell), f32(0)) == thr)
    return reach


def _reach_image_half(r):
    return (_reach_image_eq((10, 2), 1, 1, 255)(r) and f32(r["threshold"]) == f32(r["free_threshold"]) == f32(0.5)
            and _fraction(r, (10, 2)) == f32(0.5))


def _reach_threshold_zero(r):
    hit = r["hits"] > 0
    return (r["threshold"] == 0.0 and hit.any() and all(_fraction(r, tuple(c)) > f32(0.65) for c in np.argwhere(hit))
            and (r["image"][hit] == 255).all() and not (r["image"] == 100).any() and (r["image"] == 0).any())


def _reach_free_zero(r):
    only_miss = (r["hits"] == 0) & (r["misses"] > 0)
    return (r["free_threshold"] == 0.0 and only_miss.sum() > 40 and (r["image"][only_miss] == 255).all()
            and (r["image"] == 100).any() and not (r["image"] == 0).any())


def _reach_start_outside(r):
    t0, t1 = r["trace"]
    return (not _inside(r, t0["start"]) and not _inside(r, t1["start"])
            and 0 < sum(_inside(r, c) for c in _footprint(r, 0)) < 81 and not any(_inside(r, c) for c in _footprint(r, 1))
            and all(_inside(r, b[0]) for _, _, _, b in _cast(r)) and r["hits"].sum() == r["gain"] * len(_cast(r)))


def _reach_stamp_clipped(r):
    q = r["square_size"]
    ends = [b[0] for _, _, _, b in _cast(r)]
    clipped = [e for e in ends if _inside(r, e) and not all(_inside(r, (e[0] + a, e[1] + b)) for a in range(-q, q + 1) for b in range(-q, q + 1))]
    whole = [e for e in ends if all(_inside(r, (e[0] + a, e[1] + b)) for a in range(-q, q + 1) for b in range(-q, q + 1))]
    outside = [e for e in ends if not _inside(r, e)]
    return q >= 2 and len(clipped) >= 2 and len(outside) >= 1 and len(whole) >= 1 and _inside(r, r["trace"][0]["start"])


def _reach_diagonal(r):
    return _directions(r, 0) == {(1, 1, "=")} and _directions(r, 1) == {(-1, 1, "=")}


def _reach_zero_length(r):
    t = r["trace"][0]
    return t["beams"][0][0] == t["start"] and not t["beams"][0][1]


def _reach_compass(r):
    return (r["scans"].size == 256 and _AXES | _DIAGONALS | _OCTANTS <= _directions(r, 0)
            and len(set().union(*[_directions(r, s) for s in range(16)]) & _OCTANTS) == 8
            and all(b is not None for t in r["trace"] for b in t["beams"]))


def _reach_footprint(n_beams):
    def reach(r):
        inside = [[_inside(r, c) for c in _footprint(r, s)] for s in range(4)]
        return (r["scans"].shape == (4, n_beams) and all(inside[0]) and inside[0][80]          # cell 80: the loop's last
                and 0 < sum(inside[1]) < 81 and _inside(r, r["trace"][1]["robot_cell"])        # within 4 cells of the border
                and 0 < sum(inside[2]) < 81 and not _inside(r, r["trace"][2]["robot_cell"])    # the robot itself outside
                and not any(inside[3]))
    return reach


def _reach_laser_offset(r):
    return (all(t["start"] != t["robot_cell"] for t in r["trace"]) and all(-PI <= t["theta_sum"] < PI for t in r["trace"])
            and r["hits"].sum() > 0)


def _reach_laser_wrap(sign):
    def reach(r):
        return all((t["theta_sum"] >= PI) if sign > 0 else (t["theta_sum"] < -PI) for t in r["trace"]) and r["hits"].sum() > 0
    return reach


def _reach_multi_block(r):
    n = r["scans"].size
    cast = _cast(r)
    return (n > 256 and n % 256 != 0 and sum(1 for _, _, rng, b in cast if b[1] and b[2] == f32(r["usable_range"])) > 20
            and sum(1 for _, _, rng, b in cast if b[2] == f32(r["infinity_filling_range"])) > 5
            and (r["hits"] > 0).sum() > 50 and {0, 100, 255} == set(np.unique(r["image"]).tolist()) and tuple(r["offset"]) != (0, 0))


def _reach_graph(first_fixed, wrapped, derived):
    def reach(r):
        sums = [RO.base_transform(r["angle"])[2] + p[2] for p in r["poses"]]
        wraps = [k for k, t in enumerate(sums) if not -PI <= t < PI]
        return (int(np.flatnonzero(r["fixed"])[0]) == first_fixed and first_fixed != 0 and wraps == wrapped
                and (r["case"]["rows"] == 0) == derived and r["hits"].sum() > 0 and r["rows"] <= 400 and r["cols"] <= 400)
    return reach


def _reach_graph_far(r):
    """The float base angle decides the map's very size: turned by the double pi / 2, the same graph gives one row fewer."""
    tp, size, _ = RO.geometry(r["poses"], r["angle"], r["usable_range"], r["resolution"], base=(0.0, 0.0, float(r["angle"])))
    return (r["case"]["rows"] == 0 and size != (r["rows"], r["cols"]) and not np.array_equal(tp[:, :2], r["tposes"][:, :2])
            and r["hits"].sum() > 0 and max(r["rows"], r["cols"]) <= 400)


# -------------------------------------------------------------------------------------------------------------------- scans
def _footprint_scans(n_beams):
    i = np.arange(n_beams)
    row = np.where(i % 2 == 0, 1.0 + 0.02 * i, 0.0)                               # every second beam is skipped (r <= 0)
    return np.tile(row, (4, 1))


def _room_scans(n_scans, n_beams, a0, da):
    a = a0 + da * np.arange(n_beams)
    out = np.stack([3.0 + 1.5 * np.sin(3 * a + k) + 0.4 * np.cos(11 * a - k) for k in range(n_scans)])
    out[:, 5::17] = 40.0                                                          # beyond the laser's range
    out[:, 9::23] = 0.0
    out[0, 100:130] = 7.5                                                         # beyond usableRange, within the laser's
    return out


_A16 = [(10.0, 10.0, 0.0)] + [(7.0 + 0.37 * k, 12.0 - 0.29 * k, 0.4 * k - 3.0) for k in range(1, 16)]
_R16 = [[6.2] * 16] + [[3.0 + 0.25 * ((5 * k + 3 * i) % 17) for i in range(16)] for k in range(1, 16)]
_FP_POSES = [(5.0, 5.0, 0.0), (1.0, 9.0, 0.3), (-1.0, 4.0, 0.0), (30.0, 30.0, 0.0)]
_GP = [(0.3, -0.2, 0.1), (1.1, 0.4, 2.5), (2.0, 1.5, -3.0)]
_G_A0, _G_DA = -PI / 2, PI / 30


def _graph_scans(n, n_beams=31):
    a = _G_A0 + (PI / (n_beams - 1)) * np.arange(n_beams)
    return np.stack([2.0 + np.sin(2 * a + k) + 0.1 * k for k in range(n)])


CASES = {
    "single_beam": _m("world2map ties: 2.5 and 6.5 round to even; the hand-worked single beam", _reach_single_beam,
                      [(1.25, 1.25, 0.0)], [[2.0]]),
    "ties": _m("world2map ties at 0.5, 2.5, 4.5 and -0.5 (-> 0, 2, 4, 0; half-away: 1, 3, 5, -1) in start, robot and end cells",
               _reach_ties, [(0.25, 1.25, 0.0), (-0.25, 2.25, 0.0), (1.25, 0.25, 0.0)], [[1.0], [1.0], [1.0]]),
    "usable_eq": _m("r == usableRange is not cropped and scores a hit; the next float above is cropped", _reach_usable_eq,
                    [(1.0, 1.0, 0.0)], [[2.0, np.nextafter(f32(2.0), f32(3.0)), 1.5]], angular_step=0.4, usable_range=2.0),
    "max_eq_skip": _m("explicit maxRange: r == maxRange is skipped, the next float below is a hit; r = 0 and r < 0 are skipped",
                      _reach_max_eq(False), [(1.0, 1.0, 0.0)], [[3.0, np.nextafter(f32(3.0), f32(0.0)), 0.0, -1.0, 35.0]],
                      rows=16, cols=16, angular_step=0.3, max_range=3.0),
    "max_eq_fill": _m("explicit maxRange with infinity filling: r == maxRange, r = 0 and r < 0 are cast at the filling range, cropped",
                      _reach_max_eq(True), [(1.0, 1.0, 0.0)], [[3.0, np.nextafter(f32(3.0), f32(0.0)), 0.0, -1.0, 35.0]],
                      rows=16, cols=16, angular_step=0.3, max_range=3.0, infinity_filling_range=1.5),
    "image_half": _m("fraction == threshold == freeThreshold == 0.5 stays unknown", _reach_image_half, [(1.0, 1.0, 0.0)], [[4.0]],
                     gain=1, threshold=0.5, free_threshold=0.5),
    "image_075_at": _m("fraction 0.75f == threshold stays unknown", _reach_image_eq((10, 2), 3, 1, 255), [(1.0, 1.0, 0.0)], [[4.0]],
                       threshold=0.75),
    "image_075_below": _m("fraction 0.75f > nextafter(0.75f, 0) is occupied", _reach_image_eq((10, 2), 3, 1, 100), [(1.0, 1.0, 0.0)],
                          [[4.0]], threshold=float(np.nextafter(f32(0.75), f32(0.0)))),
    "threshold_zero": _m("threshold == 0 switches the occupied branch of the image off", _reach_threshold_zero, [(1.0, 1.0, 0.0)],
                         [[4.0, 3.0]], angular_step=0.5, threshold=0.0),
    "free_zero": _m("freeThreshold == 0 switches the free branch of the image off", _reach_free_zero, [(1.0, 1.0, 0.0)], [[4.0, 3.0]],
                    angular_step=0.5, free_threshold=0.0),
    "start_outside": _m("start cells outside a map smaller than the scans' extent; one footprint clipped, one wholly outside",
                        _reach_start_outside, [(-2.0, 3.0, 0.0), (20.0, 3.0, PI)], [[5.0] * 5, [17.0] * 5],
                        first_beam_angle=-0.1, angular_step=0.05),
    "stamp_clipped": _m("squareSize 2: stamps over the lower and the upper border, one whole, one end cell outside (no stamp at all)",
                        _reach_stamp_clipped, [(3.0, 3.0, 0.0)], [[2.5, 4.0, 3.0, 2.0]], angular_step=PI / 2, square_size=2),
    "diagonal": _m("dy == dx: the x-major branch, walked from the start and from the end; the hand-worked cell lists",
                   _reach_diagonal, [(1.0, 1.0, 0.0), (4.0, 1.0, PI / 2)], [[f32(2 * math.sqrt(2))]] * 2, first_beam_angle=PI / 4),
    "zero_length": _m("start == end: one cell, one miss, one stamp", _reach_zero_length, [(1.0, 1.0, 0.0)], [[0.1]]),
    "compass_256": _m("16 x 16 = 256 threads, one full block; scan 0 has the four axis lines, the four exact diagonals and all eight "
                      "octants by construction", _reach_compass, _A16, _R16, rows=41, cols=41, angular_step=PI / 8),
    **{f"footprint_b{b}": _m(f"fillRobotPose shared out over {b} beams (the loop's bound is 81): inside, at the border, robot outside, "
                             "wholly outside", _reach_footprint(b), _FP_POSES, _footprint_scans(b), rows=20, cols=20,
                             first_beam_angle=-PI, angular_step=2 * PI / b) for b in (1, 80, 81, 82)},
    "laser_offset": _m("a mounting pose: the rays start at robotPose * laserPose, the footprint stays around the robot",
                       _reach_laser_offset, [(4.0, 5.0, 1.0), (6.5, 4.2, -2.0)], [[2.0 + 0.3 * i for i in range(7)]] * 2, rows=24,
                       cols=24, first_beam_angle=-0.9, angular_step=0.3, laser_pose=(0.75, -0.5, 0.3)),
    "laser_wrap_up": _m("theta_robot + theta_laser >= pi: normalize_theta acts before cos / sin", _reach_laser_wrap(1),
                        [(6.0, 6.0, 3.0), (5.0, 7.0, 2.9)], [[2.0 + 0.3 * i for i in range(7)]] * 2, rows=24, cols=24,
                        first_beam_angle=-0.9, angular_step=0.3, laser_pose=(0.3, 0.2, 0.5)),
    "laser_wrap_down": _m("theta_robot + theta_laser < -pi", _reach_laser_wrap(-1), [(6.0, 6.0, -3.0), (5.0, 7.0, -2.9)],
                          [[2.0 + 0.3 * i for i in range(7)]] * 2, rows=24, cols=24, first_beam_angle=-0.9, angular_step=0.3,
                          laser_pose=(0.3, 0.2, -0.5)),
    "multi_block": _m("3 x 181 = 543 threads: three blocks, the last one part empty; cropping, infinity filling, squareSize 1, an "
                      "offset that is not zero, a map that is not square", _reach_multi_block,
                      [(5.0, 4.0, 0.2), (6.1, 4.7, 1.9), (7.3, 3.1, -2.6)], _room_scans(3, 181, -PI / 2, PI / 180), rows=64, cols=48,
                      resolution=0.25, offset=(-1.0, -2.0), first_beam_angle=-PI / 2, angular_step=PI / 180, usable_range=6.0,
                      infinity_filling_range=2.0, square_size=1),
    "graph_derived": _g("geometry from the graph: base angle float(pi / 2), angle + theta wraps for vertex 1, size from the bounding "
                        "box, the fixed vertex is not the first", _reach_graph(1, [1], True), _GP, _graph_scans(3),
                        first_beam_angle=_G_A0, angular_step=_G_DA, fixed=[False, True, True]),
    "graph_rows_cols": _g("explicit rows / cols, a negative base angle, angle + theta < -pi for vertex 2, which is the fixed one",
                          _reach_graph(2, [2], False), _GP, _graph_scans(3), first_beam_angle=_G_A0, angular_step=_G_DA,
                          rows=70, cols=90, angle=-0.5, fixed=[False, False, True]),
    "graph_far": _g("vertices 250 m from the origin: float(pi / 2) turns them 1.1e-5 m further than pi / 2 would, enough for another "
                    "bounding box and one more row of cells", _reach_graph_far, [(250.0, 12.0, 0.2), (251.3, 12.7, -1.0)],
                    _graph_scans(2, 91), resolution=0.05, first_beam_angle=_G_A0, angular_step=PI / 90, fixed=[True, False]),
}


# ----------------------------------------------------------------------------------------------------------------- resolving
_CACHE = {}


def _integrate(c, tposes, rows, cols, offset):
    return RO.integrate(rows, cols, c["resolution"], offset, c["scans"], tposes, c["first_beam_angle"], c["angular_step"],
                        c["laser_max_range"], c["laser_pose"], c["max_range"], c["usable_range"], c["infinity_filling_range"],
                        c["gain"], c["square_size"])


def resolved(name):
    """The case with what ref_occupancy makes of it: ``rows``, ``cols``, ``offset`` (two float32), ``tposes`` (the robot poses as
    integrateScan gets them), ``hits`` / ``misses`` (int64), ``image``, ``center`` (graph cases) and ``trace``: per scan
    dict(start, start_pt, robot_cell, theta_sum, beams) with ``beams`` as ref_occupancy.beam_ends returns them."""
    if name in _CACHE:
        return _CACHE[name]
    c = CASES[name]
    r = dict(c, case=c, name=name)
    if c["level"] == "graph":
        r["tposes"], (r["rows"], r["cols"]), r["offset"] = RO.geometry(c["poses"], c["angle"], c["usable_range"], c["resolution"],
                                                                       c["rows"], c["cols"])
        r["fixed"] = np.asarray(c["fixed"], dtype=bool)
        r["center"] = RO.map_center(c["poses"], r["fixed"], c["angle"], r["offset"], c["resolution"], r["rows"])
    else:
        r["tposes"], r["offset"] = c["poses"], (f32(c["offset"][0]), f32(c["offset"][1]))
    r["hits"], r["misses"] = _integrate(c, r["tposes"], r["rows"], r["cols"], r["offset"])
    r["image"] = RO.image(r["hits"], r["misses"], c["threshold"], c["free_threshold"])
    trace = []
    for ranges, pose in zip(c["scans"], r["tposes"]):
        start, start_pt, beams = RO.beam_ends(r["rows"], r["cols"], c["resolution"], r["offset"], ranges, pose, c["first_beam_angle"],
                                              c["angular_step"], c["laser_max_range"], c["laser_pose"], c["max_range"], c["usable_range"],
                                              c["infinity_filling_range"])
        trace.append(dict(start=start, start_pt=start_pt, beams=beams, theta_sum=float(pose[2]) + float(c["laser_pose"][2]),
                          robot_cell=RO.world2map(f32(pose[0]), f32(pose[1]), r["offset"], f32(c["resolution"]))))
    r["trace"] = trace
    for k in ("poses", "scans", "tposes", "hits", "misses", "image"):
        r[k].setflags(write=False)
    _CACHE[name] = r
    return r


# --------------------------------------------------------------------------------------------- the hand-worked answers, as literals
def _known(hits, boxes, lines, image):
    """12 x 12 arrays from literal cells: ``hits`` {cell: count}; a miss on every cell of each inclusive box (x0, x1, y0, y1) and
    on every cell of ``lines``; ``image`` {cell: value} over 0 where a cell was touched and 255 elsewhere."""
    h = np.zeros((12, 12), dtype=np.int64)
    m = np.zeros((12, 12), dtype=np.int64)
    for cell, n in hits.items():
        h[cell] = n
    for x0, x1, y0, y1 in boxes:
        m[x0:x1 + 1, y0:y1 + 1] += 1
    for cell in lines:
        m[cell] += 1
    img = np.where((h + m) > 0, 0, 255).astype(np.uint8)
    for cell, v in image.items():
        img[cell] = v
    return dict(hits=h, misses=m, image=img)


_BEAM_10_2 = [(2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (7, 2), (8, 2), (9, 2), (10, 2)]
KNOWN = {
    "single_beam": _known({(6, 2): 3}, [(0, 6, 0, 6)], [(2, 2), (3, 2), (4, 2), (5, 2), (6, 2)], {(6, 2): 255}),
    "diagonal": _known({(6, 6): 3, (4, 6): 3}, [(0, 6, 0, 6), (4, 11, 0, 6)],
                       [(2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (8, 2), (7, 3), (6, 4), (5, 5), (4, 6)], {(6, 6): 255, (4, 6): 255}),
    "zero_length": _known({(2, 2): 3}, [(0, 6, 0, 6)], [(2, 2)], {(2, 2): 255}),
    "image_half": _known({(10, 2): 1}, [(0, 6, 0, 6)], _BEAM_10_2, {(10, 2): 255}),
    "image_075_at": _known({(10, 2): 3}, [(0, 6, 0, 6)], _BEAM_10_2, {(10, 2): 255}),
    "image_075_below": _known({(10, 2): 3}, [(0, 6, 0, 6)], _BEAM_10_2, {(10, 2): 100}),
}
KNOWN_MISS_SUMS = {"single_beam": 54, "diagonal": 115, "zero_length": 50}
KNOWN_LINES = {                                                  # gridLine's cells in its own order: from the start cell
    ((2, 2), (6, 6)): [(2, 2), (3, 3), (4, 4), (5, 5), (6, 6)],
    ((8, 2), (4, 6)): [(8, 2), (7, 3), (6, 4), (5, 5), (4, 6)],
    ((2, 2), (2, 2)): [(2, 2)],
    ((2, 2), (6, 2)): [(2, 2), (3, 2), (4, 2), (5, 2), (6, 2)],
    ((3, 7), (3, 4)): [(3, 7), (3, 6), (3, 5), (3, 4)],
    ((0, 0), (5, 2)): [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)],      # d = -1, 3, -3, 1, -5: y steps after d >= 0
}
