"""The scan ranking and the greedy pruning on the GPU (cgmr_scan_information, cgmr_scan_prune) against the float64 reference
(tests/ref_scan_info.py) on every case of tests/scan_info_cases.py, the bare C ABI, and GraphSLAM.pruneScans end to end.

Counts are integers: hits, misses, cells, hit and miss sums are compared for equality, with the reference and with
cgmr_occupancy_map.  The order of the greedy loop is compared for equality too: tests/test_scan_info_cpu.py shows that every
decision of the reference stands 1e-6 nats clear of the alternative, exact ties excepted.

Floating-point results -- Delta H, the map's entropy before and after -- are compared relative to the sum of the absolute values
of the terms of the sum in question (what ref_scan_info reports as its ``scale``).  Measured on the MI355X over all cases, device
against the exactly rounded reference: worst Delta H 1.72e-17 (square1_gain3), worst map entropy 1.74e-16 (half_outside, before
pruning; 1.59e-16 after, budget), worst entropy_after - entropy_before against the sum of the deltas 1.02e-16 (relative to the
terms of both entropies; budget).  MEASURED_WORST is the largest of them, rounded up; the assertions are at ten times that, the project's practice.  Every figure is printed before it is asserted.
"""
import ctypes as C

import numpy as np
import pytest

from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import CgmrError
from cg_mrslam_amd.graph import ODOM_INFO, GraphSLAM, PoseGraph, RobotLaser
from cg_mrslam_amd.occupancy import Graph2occupancy, OccupancyConfig

import ref_scan_info as RS
import scan_info_cases as SC

pytestmark = pytest.mark.gpu

CGMR_E_INVALID, CGMR_E_ALLOC = -1, -4                # include/cgmr.h
MEASURED_WORST = 1.8e-16
TOL = 10 * MEASURED_WORST
GREEDY = [n for n in SC.CASES if n != "prune_alloc"]


def _cfg(r, **over):
    kw = dict(SC.config_kw(r), rows=r["rows"], cols=r["cols"])
    kw.update(over)
    cfg = OccupancyConfig()
    cfg.resolution, cfg.offset_x, cfg.offset_y, cfg.rows, cfg.cols = kw["resolution"], kw["offset"][0], kw["offset"][1], kw["rows"], kw["cols"]
    cfg.max_range, cfg.usable_range, cfg.infinity_filling_range = kw["max_range"], kw["usable_range"], kw["infinity_filling_range"]
    cfg.gain, cfg.square_size = kw["gain"], kw["square_size"]
    cfg.first_beam_angle, cfg.angular_step, cfg.laser_max_range = kw["first_beam_angle"], kw["angular_step"], kw["laser_max_range"]
    for k in range(3):
        cfg.laser_pose[k] = kw["laser_pose"][k]
    cfg.threshold, cfg.free_threshold = 0.65, 0.196
    return cfg


def _occupancy(ctx, r, keep=None):
    """cgmr_occupancy_map over the scans ``keep`` (default all) on the case's map."""
    scans = np.ascontiguousarray(r["scans"] if keep is None else r["scans"][keep], dtype=np.float32)
    poses = np.ascontiguousarray(r["poses"] if keep is None else r["poses"][keep], dtype=np.float64)
    hits, misses = np.zeros((r["rows"], r["cols"]), dtype=np.int32), np.zeros((r["rows"], r["cols"]), dtype=np.int32)
    cfg = _cfg(r)
    rc = ctx.lib.cgmr_occupancy_map(ctx.h, C.byref(cfg), C.c_int(len(scans)), C.c_int(r["scans"].shape[1]), C.c_void_p(scans.ctypes.data),
                                    C.c_void_p(poses.ctypes.data), C.c_void_p(hits.ctypes.data), C.c_void_p(misses.ctypes.data),
                                    C.c_void_p(None), C.c_void_p(None))
    assert rc == 0
    return hits, misses


def _info(ctx, r, limit=None):
    return ctx.scan_information(_cfg(r), r["scans"], r["poses"], r["info_limit"] if limit is None else limit)


def _prune(ctx, r):
    return ctx.scan_prune(_cfg(r), r["scans"], r["poses"], r["max_remove"], r["budget"], r["protected"] if r["case"]["protected"] else None,
                          r["prune_limit"])


def _rel(got, want, scale):
    """|got - want| relative to the sum of the absolute values of the terms; a sum without terms must be exactly zero."""
    got, want, scale = np.atleast_1d(got).astype(float), np.atleast_1d(want).astype(float), np.atleast_1d(scale).astype(float)
    assert got.shape == want.shape
    assert np.all(got[scale == 0] == 0.0)
    return float(np.max(np.abs(got - want)[scale > 0] / scale[scale > 0], initial=0.0))


def info_errors(got, r):
    ref = r["info"]
    return dict(delta=_rel(got["delta"], ref["delta"], ref["scale"]), map_entropy=_rel(got["map_entropy"], ref["map_entropy"], ref["map_scale"]))


def prune_errors(got, r):
    ref = r["greedy"]
    k = len(ref["order"])
    both = ref["before_scale"] + ref["after_scale"]
    return dict(delta=_rel(got["delta"][:k], ref["delta"], ref["scale"]) if len(got["delta"]) >= k else float("inf"),
                entropy_before=_rel(got["entropy_before"], ref["entropy_before"], ref["before_scale"]),
                entropy_after=_rel(got["entropy_after"], ref["entropy_after"], ref["after_scale"]),
                balance=_rel(got["entropy_after"] - got["entropy_before"], float(np.sum(got["delta"])), both))


# ------------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", list(SC.CASES))
def test_information_matches_reference(ctx, name):
    r = SC.resolved(name)
    assert r["reach"](r), f"{name}: {r['why']}"
    got, ref = _info(ctx, r), r["info"]
    for k in ("hits", "misses", "cells", "hit_sum", "miss_sum"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert got["hits"].dtype == got["misses"].dtype == got["cells"].dtype == np.int32 and got["hit_sum"].dtype == np.int64
    h, m = _occupancy(ctx, r)
    assert got["hits"].tobytes() == h.tobytes() and got["misses"].tobytes() == m.tobytes()
    err = info_errors(got, r)
    print(f"scan_info figures {name}: information {err}")
    assert max(err.values()) <= TOL, err
    total, n_chunks, largest, _ = ctx.scan_info_last_stats()
    b = [RS.window_bytes(*c) for c in r["counts"]]
    assert total == sum(b) and largest == max(b) and n_chunks == len(RS.chunks(b, r["info_limit"] or 1 << 30))


@pytest.mark.parametrize("name", GREEDY)
def test_prune_matches_reference(ctx, name):
    r = SC.resolved(name)
    got, ref = _prune(ctx, r), r["greedy"]
    assert got["order"].tolist() == ref["order"] and len(got["delta"]) == len(ref["order"])
    err = prune_errors(got, r)
    print(f"scan_info figures {name}: prune {err}")
    assert max(err.values()) <= TOL, err
    np.testing.assert_array_equal(got["hits"], ref["hits"])
    np.testing.assert_array_equal(got["misses"], ref["misses"])
    keep = np.array([s for s in range(len(r["scans"])) if s not in ref["order"]], dtype=np.int64)
    h, m = _occupancy(ctx, r, keep)                            # bit for bit the map of the kept scans alone
    assert got["hits"].tobytes() == h.tobytes() and got["misses"].tobytes() == m.tobytes()


def test_prune_refuses_windows_that_do_not_fit(ctx):
    r = SC.resolved("prune_alloc")
    assert r["reach"](r)
    need = sum(RS.window_bytes(*c) for c in r["counts"])
    with pytest.raises(CgmrError) as e:
        _prune(ctx, r)
    assert e.value.code == CGMR_E_ALLOC and str(need) in str(e.value) and str(r["prune_limit"]) in str(e.value)
    got = _info(ctx, r, limit=r["prune_limit"])                # the ranking takes the same limit in chunks
    assert ctx.scan_info_last_stats()[1] == len(RS.chunks([RS.window_bytes(*c) for c in r["counts"]], r["prune_limit"])) >= 2
    assert max(info_errors(got, r).values()) <= TOL
    with pytest.raises(CgmrError) as e:                        # one window alone over the limit: neither call can run
        _info(ctx, r, limit=100)
    assert e.value.code == CGMR_E_ALLOC
    roomy = ctx.scan_prune(_cfg(r), r["scans"], r["poses"], r["max_remove"], r["budget"], None, need)     # exactly enough
    assert roomy["order"].tolist() == r["greedy"]["order"]


# ---------------------------------------------------------------------------------------------------------------- determinism
def _bytes_of(d):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in d.items() if k != "kernel_seconds"}


@pytest.mark.parametrize("name", ["duplicates", "wide_window", "disjoint", "budget"])
def test_two_calls_give_identical_bytes(ctx, name):
    r = SC.resolved(name)
    assert _bytes_of(_info(ctx, r)) == _bytes_of(_info(ctx, r))
    assert _bytes_of(_prune(ctx, r)) == _bytes_of(_prune(ctx, r))


def test_duplicate_scans_tie_bit_for_bit(ctx):
    r = SC.resolved("duplicates")
    got = _info(ctx, r)
    assert got["delta"][1].tobytes() == got["delta"][3].tobytes() and got["delta"][1] != got["delta"][0]
    order = _prune(ctx, r)["order"].tolist()
    assert order[0] == 1 and order.index(1) < order.index(3)


@pytest.mark.parametrize("name", ["three_chunks", "disjoint", "wide_window"])
def test_chunked_and_unchunked_give_identical_bytes(ctx, name):
    r = SC.resolved(name)
    b = [RS.window_bytes(*c) for c in r["counts"]]
    whole = _info(ctx, r, limit=0)
    assert ctx.scan_info_last_stats()[1] == 1
    limit = r["info_limit"] or max(b)
    parts = _info(ctx, r, limit=limit)
    assert ctx.scan_info_last_stats()[1] == len(RS.chunks(b, limit)) >= 2
    if name == "three_chunks":
        assert ctx.scan_info_last_stats()[1] == 3
    assert _bytes_of(whole) == _bytes_of(parts)


# ----------------------------------------------------------------------------------------------------------------- the bare ABI
_SENTINEL = -7


def _raw_info(ctx, cfg, scans, poses, n_scans=None, n_beams=None, limit=0, cfg_null=False):
    n = len(scans) if n_scans is None else n_scans
    shape = (max(cfg.rows, 1), max(cfg.cols, 1))
    out = dict(delta=np.full(max(n, 1), float(_SENTINEL)), cells=np.full(max(n, 1), _SENTINEL, dtype=np.int32),
               hit_sum=np.full(max(n, 1), _SENTINEL, dtype=np.int64), miss_sum=np.full(max(n, 1), _SENTINEL, dtype=np.int64),
               hits=np.full(shape, _SENTINEL, dtype=np.int32), misses=np.full(shape, _SENTINEL, dtype=np.int32))
    ent = C.c_double(float(_SENTINEL))
    p = lambda a: C.c_void_p(None if a is None else a.ctypes.data)     # noqa: E731
    rc = ctx.lib.cgmr_scan_information(ctx.h, None if cfg_null else C.byref(cfg), C.c_int(n),
                                       C.c_int(scans.shape[1] if n_beams is None else n_beams), p(scans), p(poses), C.c_int64(limit),
                                       p(out["delta"]), p(out["cells"]), p(out["hit_sum"]), p(out["miss_sum"]), p(out["hits"]),
                                       p(out["misses"]), C.byref(ent), C.c_void_p(None))
    out["map_entropy"] = ent.value
    return rc, out


def _raw_prune(ctx, cfg, scans, poses, max_remove, budget=-1.0, limit=0, null=(), n_scans=None):
    n = len(scans) if n_scans is None else n_scans
    shape = (max(cfg.rows, 1), max(cfg.cols, 1))
    out = dict(order=np.full(max(n, 1), _SENTINEL, dtype=np.int32), delta=np.full(max(n, 1), float(_SENTINEL)),
               hits=np.full(shape, _SENTINEL, dtype=np.int32), misses=np.full(shape, _SENTINEL, dtype=np.int32))
    k, before, after = C.c_int32(_SENTINEL), C.c_double(float(_SENTINEL)), C.c_double(float(_SENTINEL))
    p = lambda name, a: C.c_void_p(None if a is None or name in null else a.ctypes.data)     # noqa: E731
    rc = ctx.lib.cgmr_scan_prune(ctx.h, C.byref(cfg), C.c_int(n), C.c_int(scans.shape[1]), p("ranges", scans),
                                 p("poses", poses), C.c_void_p(None), C.c_int(max_remove), C.c_double(budget), C.c_int64(limit),
                                 p("order", out["order"]), p("delta", out["delta"]), None if "n_removed" in null else C.byref(k),
                                 C.byref(before), C.byref(after), p("hits", out["hits"]), p("misses", out["misses"]), C.c_void_p(None))
    out.update(n_removed=k.value, entropy_before=before.value, entropy_after=after.value)
    return rc, out


def _untouched(out):
    return all((np.all(v == _SENTINEL) if isinstance(v, np.ndarray) else v == _SENTINEL) for v in out.values())


def _abi_inputs():
    r = SC.resolved("half_outside")
    return r, np.ascontiguousarray(r["scans"], dtype=np.float32), np.ascontiguousarray(r["poses"], dtype=np.float64)


def test_abi_null_context():
    from cg_mrslam_amd import _lib
    lib = _lib.load_library()
    assert lib.cgmr_scan_information(*([None] * 6), C.c_int64(0), *([None] * 8)) == CGMR_E_INVALID
    assert lib.cgmr_scan_prune(*([None] * 7), C.c_int(1), C.c_double(-1.0), C.c_int64(0), *([None] * 8)) == CGMR_E_INVALID
    assert lib.cgmr_scan_info_last_stats(None, None) == CGMR_E_INVALID


@pytest.mark.parametrize("bad", ["n_beams", "rows", "resolution", "square_size", "gain", "limit", "ranges", "cfg"])
def test_abi_information_refuses(ctx, bad):
    r, scans, poses = _abi_inputs()
    over = {"rows": dict(rows=0), "resolution": dict(resolution=0.0), "square_size": dict(square_size=-1), "gain": dict(gain=-1)}.get(bad, {})
    rc, out = _raw_info(ctx, _cfg(r, **over), None if bad == "ranges" else scans, poses, n_scans=len(poses),
                        n_beams=0 if bad == "n_beams" else scans.shape[1], limit=-1 if bad == "limit" else 0, cfg_null=bad == "cfg")
    assert rc == CGMR_E_INVALID and _untouched(out)
    rc, out = _raw_info(ctx, _cfg(r), scans, poses)            # and the context still works
    assert rc == 0
    np.testing.assert_array_equal(out["hits"], r["hits"])


@pytest.mark.parametrize("bad", ["max_remove", "nan_budget", "order", "delta", "n_removed", "ranges", "poses", "limit"])
def test_abi_prune_refuses(ctx, bad):
    r, scans, poses = _abi_inputs()
    rc, out = _raw_prune(ctx, _cfg(r), scans, poses, -1 if bad == "max_remove" else 2, float("nan") if bad == "nan_budget" else -1.0,
                         -1 if bad == "limit" else 0, null=(bad,))
    assert rc == CGMR_E_INVALID and _untouched(out)
    assert ctx.lib.cgmr_last_error(ctx.h).decode().startswith("cgmr_scan_prune")
    rc, out = _raw_prune(ctx, _cfg(r), scans, poses, 2)
    assert rc == 0 and out["n_removed"] == 2 and out["order"][:2].tolist() == r["greedy"]["order"][:2]


def test_abi_every_output_is_optional(ctx):
    r, scans, poses = _abi_inputs()
    cfg = _cfg(r)
    rc = ctx.lib.cgmr_scan_information(ctx.h, C.byref(cfg), C.c_int(2), C.c_int(12), C.c_void_p(scans.ctypes.data),
                                       C.c_void_p(poses.ctypes.data), C.c_int64(0), *([None] * 8))
    assert rc == 0
    k = C.c_int32(_SENTINEL)
    rc = ctx.lib.cgmr_scan_prune(ctx.h, C.byref(cfg), C.c_int(2), C.c_int(12), C.c_void_p(scans.ctypes.data), C.c_void_p(poses.ctypes.data),
                                 None, C.c_int(0), C.c_double(-1.0), C.c_int64(0), None, None, C.byref(k), *([None] * 5))
    assert rc == 0 and k.value == 0                            # max_remove == 0: order_out and delta_out are not needed


def test_abi_no_scans(ctx):
    r, scans, poses = _abi_inputs()
    cfg = _cfg(r, rows=13, cols=9)
    rc, out = _raw_info(ctx, cfg, scans[:0], None, n_scans=0, n_beams=5)
    assert rc == 0 and not out["hits"].any() and not out["misses"].any()
    assert abs(out["map_entropy"] - 13 * 9 * RS.LN2) <= TOL * 13 * 9 * RS.LN2
    assert np.all(out["delta"] == _SENTINEL)
    rc, out = _raw_prune(ctx, cfg, scans[:0], None, 3, n_scans=0, null=("ranges",))
    assert rc == 0 and out["n_removed"] == 0 and out["entropy_before"] == out["entropy_after"]
    assert abs(out["entropy_after"] - 13 * 9 * RS.LN2) <= TOL * 13 * 9 * RS.LN2 and not out["hits"].any()


# ------------------------------------------------------------------------------------------------------------------ end to end
class _PinnedGeometry(Graph2occupancy):
    def geometry(self):
        return self.pinned


def _corridor(ctx):
    tr = synth.make_trajectory(30, laps=0.2)
    scans = tr["scans"][:, ::6]                                # every sixth beam: 181 beams, six times the angular step
    n = len(tr["odom"])
    ef, et = np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    meas = synth.se2_compose(synth.se2_inverse(tr["odom"][:-1]), tr["odom"][1:])
    info = np.zeros((n - 1, 6))
    info[:, 0], info[:, 3], info[:, 5] = ODOM_INFO
    fixed = np.zeros(n, dtype=np.uint8)
    fixed[0] = 1
    g = PoseGraph(10 + 3 * np.arange(n), tr["odom"].copy(), fixed, ef, et, meas, info)
    g.lasers = {v: RobotLaser(scans[v], tr["angle_min"], tr["angle_inc"] * 6, tr["max_range"]) for v in range(n) if v != 17}
    return GraphSLAM(g, ctx), tr


_MAP_KW = dict(resolution=0.25, usableRange=8.0)


def test_graph_prune_scans_end_to_end(ctx):
    slam, tr = _corridor(ctx)
    g = slam.graph
    idx, occ = slam._laser_map("test", **_MAP_KW)
    assert 17 not in idx and len(idx) == 29
    vid, dh = slam.scanInformation(**_MAP_KW)
    assert np.array_equal(vid, idx) and dh.shape == (29,) and np.all(dh > 0)
    keep = [5]
    protected = np.asarray(g.fixed[idx]).astype(bool) | np.isin(idx, keep)
    sel = occ.pruneScans(8, protected=protected)               # the selection alone, for its totals
    tposes, size, offset = occ.geometry()
    poses_before, ids_before = g.poses.copy(), g.ids.copy()
    index_map, new_edges, skipped, order, delta = slam.pruneScans(8, keep=keep, **_MAP_KW)
    assert order.tolist() == idx[sel["order"]].tolist() and delta.tobytes() == sel["delta"].tobytes() and len(order) == 8
    assert 0 not in order and 5 not in order and 17 not in order
    gone = sorted(set(order.tolist()) - {v for v, _ in skipped})
    assert np.flatnonzero(index_map < 0).tolist() == gone and g.n_vertices == 30 - len(gone)
    assert np.array_equal(g.ids, ids_before[index_map >= 0]) and np.array_equal(g.poses, poses_before[index_map >= 0])
    assert sorted(g.lasers) == [int(index_map[v]) for v in idx if index_map[v] >= 0]
    # the map of the surviving key frames, on the geometry the selection ran on, is the totals the selection returned
    assert not skipped
    stay = np.array([k for k, v in enumerate(idx) if index_map[v] >= 0])
    rest = _PinnedGeometry(ctx, g.poses[[int(index_map[v]) for v in idx[stay]]], occ.scans[stay], occ.first_beam_angle, occ.angular_step,
                           occ.laser_max_range, **_MAP_KW)
    rest.pinned = (tposes[stay], size, offset)
    assert rest.computeMap()
    assert rest.hits.tobytes() == sel["hits"].tobytes() and rest.misses.tobytes() == sel["misses"].tobytes()
    slam.optimize(3)                                           # and the graph still optimises
    assert np.isfinite(g.poses).all() and np.isfinite(slam.chi2())


def test_graph_prune_scans_raises_as_remove_vertices(ctx):
    slam, _ = _corridor(ctx)
    g = slam.graph
    with pytest.raises(ValueError, match="out of range"):
        slam.pruneScans(2, keep=[99], **_MAP_KW)
    g.lasers[3] = RobotLaser(np.ones(7), 0.0, 0.1, 30.0)
    with pytest.raises(ValueError, match="different lasers"):
        slam.scanInformation(**_MAP_KW)
    slam, _ = _corridor(ctx)
    slam.graph.set_edge_mixture(0, [(1.0, slam.graph.meas[0], slam.graph.info[0]), (0.5, slam.graph.meas[0], slam.graph.info[0])])
    with pytest.raises(ValueError, match="mixture"):
        slam.pruneScans(2, **_MAP_KW)
    slam, _ = _corridor(ctx)
    slam.addLandmark(999, [1.0, 1.0])
    with pytest.raises(ValueError, match="pose graphs only"):
        slam.pruneScans(2, **_MAP_KW)
    slam, _ = _corridor(ctx)
    slam.graph.lasers = {}
    with pytest.raises(ValueError, match="no vertex carries"):
        slam.scanInformation(**_MAP_KW)
