"""The occupancy-map case table (tests/occupancy_cases.py) without a GPU: every case reaches the gap it is named after, the
independent reference (tests/ref_occupancy.py) gives the hand-worked answers, the oracle (oracle/occupancy_oracle.c) equals the
reference on every case, and the host logic of the Python mirror (geometry, map centre) equals the reference's.  Every
comparison is exact equality of integer, byte or float arrays."""
import math

import numpy as np
import pytest

from cg_mrslam_amd.occupancy import Graph2occupancy

import occupancy_cases as OC
import ref_occupancy as RO

GRAPH_CASES = [n for n, c in OC.CASES.items() if c["level"] == "graph"]


@pytest.mark.parametrize("name", list(OC.CASES))
def test_case_reaches_its_gap(name):
    r = OC.resolved(name)
    assert r["reach"](r), f"{name}: {r['why']}"
    assert r["rows"] <= 400 and r["cols"] <= 400 and r["scans"].shape[0] <= 16 and r["scans"].shape[1] <= 361


def test_table_covers_the_thread_counts():
    sizes = {n: c["scans"].size for n, c in OC.CASES.items()}
    assert sizes["compass_256"] == 256
    assert sizes["multi_block"] > 256 and sizes["multi_block"] % 256 != 0
    assert {c["scans"].shape[1] for c in OC.CASES.values()} >= {1, 80, 81, 82}


@pytest.mark.parametrize("name", list(OC.KNOWN))
def test_reference_gives_the_hand_worked_answers(name):
    r, k = OC.resolved(name), OC.KNOWN[name]
    np.testing.assert_array_equal(r["hits"], k["hits"])
    np.testing.assert_array_equal(r["misses"], k["misses"])
    np.testing.assert_array_equal(r["image"], k["image"])
    if name in OC.KNOWN_MISS_SUMS:
        assert int(r["misses"].sum()) == OC.KNOWN_MISS_SUMS[name]


def test_hand_worked_literals():
    r = OC.resolved("single_beam")
    assert r["trace"][0]["start"] == (2, 2) and r["trace"][0]["beams"][0][0] == (6, 2)
    assert int(r["hits"].sum()) == 3 and r["hits"][6, 2] == 3 and int(r["misses"].sum()) == 54
    assert (r["misses"][:7, :7] >= 1).all() and [int(v) for v in r["misses"][2:7, 2]] == [2] * 5
    assert OC.resolved("image_half")["image"][10, 2] == 255
    assert OC.resolved("image_075_at")["image"][10, 2] == 255
    assert OC.resolved("image_075_below")["image"][10, 2] == 100
    # world2map ties at resolution 0.5: 0.25 and 1.25 -> cells 0 and 2 (half-away rounding: 1 and 3)
    off, res = (np.float32(0), np.float32(0)), np.float32(0.5)
    assert RO.world2map(np.float32(0.25), np.float32(1.25), off, res) == (0, 2)
    assert RO.world2map(np.float32(-0.25), np.float32(2.25), off, res) == (0, 4)
    assert RO.world2map(np.float32(0.75), np.float32(1.75), off, res) == (2, 4)


def test_grid_line_literals(oracle):
    for (start, end), cells in OC.KNOWN_LINES.items():
        assert RO.grid_line(start, end) == cells
        core = [tuple(int(v) for v in p) for p in oracle.grid_line(*start, *end)]
        assert core in (cells, cells[::-1]) and core == RO.grid_line_core(start, end)


def test_grid_line_oracle_vs_reference(oracle):
    """Every line of up to 6 cells' extent from one start, all octants and degenerate ones: the oracle's gridLineCore equals the
    reference's, and gridLine begins at the start."""
    for ex in range(-6, 7):
        for ey in range(-6, 7):
            core = RO.grid_line_core((1, -2), (1 + ex, -2 + ey))
            assert [tuple(int(v) for v in p) for p in oracle.grid_line(1, -2, 1 + ex, -2 + ey)] == core
            line = RO.grid_line((1, -2), (1 + ex, -2 + ey))
            assert line[0] == (1, -2) and line[-1] == (1 + ex, -2 + ey) and sorted(line) == sorted(core)


@pytest.mark.parametrize("name", list(OC.CASES))
def test_oracle_matches_reference(oracle, name):
    r = OC.resolved(name)
    h, m = oracle.occupancy_integrate(r["rows"], r["cols"], r["resolution"], (float(r["offset"][0]), float(r["offset"][1])), r["scans"],
                                      r["tposes"], r["first_beam_angle"], r["angular_step"], r["laser_max_range"],
                                      laser_pose=r["laser_pose"], max_range=r["max_range"], usable_range=r["usable_range"],
                                      infinity_filling_range=r["infinity_filling_range"], gain=r["gain"], square_size=r["square_size"])
    np.testing.assert_array_equal(h, r["hits"])
    np.testing.assert_array_equal(m, r["misses"])
    np.testing.assert_array_equal(oracle.occupancy_image(h, m, r["threshold"], r["free_threshold"]), r["image"])


def test_oracle_resolves_negative_ranges_as_the_reference(oracle):
    """usableRange < 0 with an explicit maxRange, and both negative: integrateScan's own resolution (frequency_map.cpp:29-30)."""
    r = OC.resolved("max_eq_skip")
    for max_range, usable in ((3.0, -1.0), (-1.0, -1.0), (-1.0, 2.5)):
        want = RO.integrate(16, 16, 0.5, (0.0, 0.0), r["scans"], r["tposes"], 0.0, 0.3, 30.0, (0.0, 0.0, 0.0), max_range, usable, -1.0, 3, 0)
        got = oracle.occupancy_integrate(16, 16, 0.5, (0.0, 0.0), r["scans"], r["tposes"], 0.0, 0.3, 30.0, max_range=max_range,
                                         usable_range=usable, infinity_filling_range=-1.0, gain=3, square_size=0)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def _mirror(r):
    c = r["case"]
    return Graph2occupancy(None, c["poses"], c["scans"], c["first_beam_angle"], c["angular_step"], c["laser_max_range"],
                           laser_pose=c["laser_pose"], fixed=c["fixed"], resolution=c["resolution"], threshold=c["threshold"],
                           rows=c["rows"], cols=c["cols"], maxRange=c["max_range"], usableRange=c["usable_range"],
                           infinityFillingRange=c["infinity_filling_range"], gain=c["gain"], squareSize=c["square_size"],
                           angle=c["angle"], freeThreshold=c["free_threshold"])


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_mirror_geometry_and_center_match_reference(name):
    """tposes (the heading included), size, offset and map centre of the mirror against the reference's, bit for bit.  The
    heading column is where a base angle held as a double shows at once: float(pi / 2) + theta is not pi / 2 + theta."""
    r = OC.resolved(name)
    g = _mirror(r)
    tposes, size, offset = g.geometry()
    np.testing.assert_array_equal(tposes, r["tposes"])
    assert tuple(size) == (r["rows"], r["cols"])
    assert (np.float32(offset[0]), np.float32(offset[1])) == tuple(r["offset"])
    center = g.mapCenterOf(tposes, size, offset)
    assert center.dtype == np.float32
    np.testing.assert_array_equal(center, r["center"])


def test_base_angle_is_a_float():
    assert RO.base_transform(math.pi / 2)[2] == 1.5707963705062866 != math.pi / 2
    g = Graph2occupancy(None, [(1.0, 2.0, 0.25)], np.ones((1, 3), dtype=np.float32), 0.0, 0.1, 30.0)
    tposes, _, _ = g.geometry()
    assert tposes[0, 2] == 1.5707963705062866 + 0.25


def test_center_without_a_fixed_vertex_is_zero():
    r = OC.resolved("graph_derived")
    assert RO.map_center(r["poses"], [False] * 3, r["angle"], r["offset"], r["resolution"], r["rows"]).tolist() == [0.0, 0.0]
    g = _mirror(r)
    g.fixed = None
    assert g.mapCenterOf(*g.geometry()).tolist() == [0.0, 0.0]
