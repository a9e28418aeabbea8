"""The occupancy map on the GPU (cgmr_occupancy_map) against the independent reference (tests/ref_occupancy.py) on the case
table of tests/occupancy_cases.py, the branches of the C ABI that the Python mirror never takes, and the arena it shares with
the matcher.  Hits, misses and the image are integer / byte arrays: every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

from cg_mrslam_amd import synth
from cg_mrslam_amd.matcher import ScanMatcher
from cg_mrslam_amd.occupancy import Graph2occupancy, OccupancyConfig

import occupancy_cases as OC
import ref_occupancy as RO

pytestmark = pytest.mark.gpu

CGMR_E_INVALID = -1                                            # include/cgmr.h


class _PinnedGeometry(Graph2occupancy):
    """Graph2occupancy with the FrequencyMap's size, offset and robot poses given (a *map* case); computeMap is the class's own."""

    def geometry(self):
        return self.pinned


def _mirror(ctx, r):
    c = r["case"]
    cls = Graph2occupancy if c["level"] == "graph" else _PinnedGeometry
    g = cls(ctx, c["poses"], c["scans"], c["first_beam_angle"], c["angular_step"], c["laser_max_range"], laser_pose=c["laser_pose"],
            fixed=c.get("fixed"), resolution=c["resolution"], threshold=c["threshold"], rows=c["rows"], cols=c["cols"],
            maxRange=c["max_range"], usableRange=c["usable_range"], infinityFillingRange=c["infinity_filling_range"], gain=c["gain"],
            squareSize=c["square_size"], angle=c.get("angle", 0.0), freeThreshold=c["free_threshold"])
    g.pinned = (np.array(r["tposes"]), (r["rows"], r["cols"]), r["offset"])
    return g


@pytest.mark.parametrize("name", list(OC.CASES))
def test_map_matches_reference(ctx, name):
    r = OC.resolved(name)
    assert r["reach"](r), f"{name}: {r['why']}"
    g = _mirror(ctx, r)
    assert g.computeMap()
    assert g.hits.shape == (r["rows"], r["cols"]) and g.hits.dtype == np.int32 and g.image.dtype == np.uint8
    np.testing.assert_array_equal(g.hits, r["hits"])
    np.testing.assert_array_equal(g.misses, r["misses"])
    np.testing.assert_array_equal(g.image, r["image"])
    if r["level"] == "graph":
        tposes, size, offset = g.geometry()
        np.testing.assert_array_equal(tposes, r["tposes"])
        assert tuple(size) == (r["rows"], r["cols"]) and tuple(g.offset) == tuple(r["offset"])
        np.testing.assert_array_equal(g.getMapCenter(), r["center"])
    if name in OC.KNOWN:                                       # and the literals themselves, not only the reference
        np.testing.assert_array_equal(g.hits, OC.KNOWN[name]["hits"])
        np.testing.assert_array_equal(g.misses, OC.KNOWN[name]["misses"])
        np.testing.assert_array_equal(g.image, OC.KNOWN[name]["image"])


# ---------------------------------------------------------------------------------------------------------- the C ABI itself
def _config(rows, cols, resolution=0.5, offset=(0.0, 0.0), max_range=-1.0, usable_range=-1.0, infinity_filling_range=-1.0, gain=3,
            square_size=0, first_beam_angle=0.0, angular_step=0.0, laser_max_range=30.0, laser_pose=(0.0, 0.0, 0.0), threshold=0.65,
            free_threshold=0.196):
    cfg = OccupancyConfig()
    cfg.resolution, cfg.offset_x, cfg.offset_y, cfg.rows, cfg.cols = resolution, offset[0], offset[1], rows, cols
    cfg.max_range, cfg.usable_range, cfg.infinity_filling_range = max_range, usable_range, infinity_filling_range
    cfg.gain, cfg.square_size = gain, square_size
    cfg.first_beam_angle, cfg.angular_step, cfg.laser_max_range = first_beam_angle, angular_step, laser_max_range
    for k in range(3):
        cfg.laser_pose[k] = laser_pose[k]
    cfg.threshold, cfg.free_threshold = threshold, free_threshold
    return cfg


def _call(ctx, cfg, scans, poses, n_beams=None, outputs=("hits", "misses", "image")):
    """cgmr_occupancy_map as a C caller reaches it.  Returns (status, {name: array}); arrays not asked for are passed as null,
    the others start out as a pattern that no map holds."""
    scans = None if scans is None else np.ascontiguousarray(scans, dtype=np.float32)
    poses = None if poses is None else np.ascontiguousarray(poses, dtype=np.float64)
    n_scans = 0 if scans is None else scans.shape[0]
    n_beams = scans.shape[1] if n_beams is None else n_beams
    shape = (max(cfg.rows, 0), max(cfg.cols, 0))
    out = {"hits": np.full(shape, -7, dtype=np.int32), "misses": np.full(shape, -7, dtype=np.int32), "image": np.full(shape, 7, dtype=np.uint8)}
    ptr = [C.c_void_p(out[k].ctypes.data if k in outputs else None) for k in ("hits", "misses", "image")]
    rc = ctx.lib.cgmr_occupancy_map(ctx.h, C.byref(cfg), C.c_int(n_scans), C.c_int(n_beams),
                                    C.c_void_p(None if scans is None else scans.ctypes.data),
                                    C.c_void_p(None if poses is None else poses.ctypes.data), *ptr, C.c_void_p(None))
    return rc, {k: out[k] for k in outputs}


def _ref(cfgkw, rows, cols, scans, poses):
    kw = dict(resolution=0.5, offset=(0.0, 0.0), first_beam_angle=0.0, angular_step=0.0, laser_max_range=30.0, laser_pose=(0.0, 0.0, 0.0),
              max_range=-1.0, usable_range=-1.0, infinity_filling_range=-1.0, gain=3, square_size=0, threshold=0.65, free_threshold=0.196)
    kw.update(cfgkw)
    h, m = RO.integrate(rows, cols, kw["resolution"], kw["offset"], np.asarray(scans, dtype=np.float32), poses, kw["first_beam_angle"],
                        kw["angular_step"], kw["laser_max_range"], kw["laser_pose"], kw["max_range"], kw["usable_range"],
                        kw["infinity_filling_range"], kw["gain"], kw["square_size"])
    return h, m, RO.image(h, m, kw["threshold"], kw["free_threshold"])


_ABI_RANGES = {
    # maxRange 40 beyond the laser's 30, usableRange -1 -> 40: r = 35 is NOT cropped and scores a hit (a usableRange resolved to
    # the laser's range would crop it); r = 40 is skipped, the float below 40 is a hit
    "usable_follows_explicit_max": (dict(resolution=1.0, max_range=40.0, usable_range=-1.0, angular_step=0.2),
                                    [[35.0, 29.0, 40.0, float(np.nextafter(np.float32(40.0), np.float32(0.0)))]]),
    # both negative: maxRange = usableRange = the laser's 30; r = 30 is skipped, r = 31 cropped and then skipped
    "both_from_the_laser": (dict(resolution=1.0, angular_step=0.2), [[30.0, 29.5, 31.0, 12.0]]),
    "explicit_max_with_filling": (dict(resolution=1.0, max_range=20.0, usable_range=-1.0, infinity_filling_range=5.0, angular_step=0.2),
                                  [[20.0, 19.5, 25.0, 0.0, 7.0]]),
}


@pytest.mark.parametrize("name", list(_ABI_RANGES))
def test_abi_resolves_negative_ranges(ctx, name):
    """cfg->usable_range < 0 and an explicit cfg->max_range: the mirror resolves the first before the call and the tests always
    passed -1 for the second."""
    kw, scans = _ABI_RANGES[name]
    poses = np.array([[2.0, 2.0, 0.0]])
    rc, got = _call(ctx, _config(48, 48, **kw), scans, poses)
    assert rc == 0
    h, m, img = _ref(kw, 48, 48, scans, poses)
    assert h.sum() >= 6                                        # at least two beams score
    np.testing.assert_array_equal(got["hits"], h)
    np.testing.assert_array_equal(got["misses"], m)
    np.testing.assert_array_equal(got["image"], img)
    if name == "usable_follows_explicit_max":
        assert h[37, 2] == 3                                   # the r = 35 beam at angle 0: end cell (2 + 35, 2)


def test_abi_no_scans(ctx):
    """n_scans == 0: nothing is launched on the beams; the counters come back zero and the image unknown (also with null inputs)."""
    rc, got = _call(ctx, _config(13, 9), None, None, n_beams=5)
    assert rc == 0
    assert not got["hits"].any() and not got["misses"].any() and (got["image"] == 255).all()


def test_abi_image_only(ctx):
    r = OC.resolved("multi_block")
    c = r["case"]
    cfg = _config(r["rows"], r["cols"], **{k: c[k] for k in ("resolution", "offset", "max_range", "usable_range", "infinity_filling_range",
                                                               "gain", "square_size", "first_beam_angle", "angular_step", "laser_max_range",
                                                               "laser_pose", "threshold", "free_threshold")})
    rc, got = _call(ctx, cfg, r["scans"], r["tposes"], outputs=("image",))
    assert rc == 0
    np.testing.assert_array_equal(got["image"], r["image"])
    rc, got = _call(ctx, cfg, r["scans"], r["tposes"], outputs=("misses",))
    assert rc == 0
    np.testing.assert_array_equal(got["misses"], r["misses"])


@pytest.mark.parametrize("bad", ["n_beams", "rows", "resolution", "square_size"])
def test_abi_rejects_bad_arguments(ctx, bad):
    kw = dict(rows=12, cols=12)
    if bad == "rows":
        kw["rows"] = 0
    if bad == "resolution":
        kw["resolution"] = 0.0
    if bad == "square_size":
        kw["square_size"] = -1
    scans, poses = np.ones((1, 1), dtype=np.float32), np.array([[1.0, 1.0, 0.0]])
    rc, _ = _call(ctx, _config(**kw), scans, poses, n_beams=0 if bad == "n_beams" else None)
    assert rc == CGMR_E_INVALID
    rc, got = _call(ctx, _config(12, 12), [[2.0]], [[1.25, 1.25, 0.0]])            # and the context still works
    assert rc == 0
    np.testing.assert_array_equal(got["hits"], OC.KNOWN["single_beam"]["hits"])


# ------------------------------------------------------------------------------------------------------------ the shared arena
def test_map_and_matcher_share_the_arena(ctx):
    """cgmr_occupancy_map stages into the context's matcher arena and pinned buffer.  A matcher call, a map, the same matcher call
    and the map again on one context: both matcher results bit-identical, both maps bit-identical (and the reference's)."""
    sp = synth.make_scan_pairs(2, seed=77)
    m = ScanMatcher(ctx, sp["n_beams"], sp["angle_min"], sp["angle_inc"], sp["max_range"])
    r = OC.resolved("multi_block")
    first = m.closeScanMatching(sp["ranges_ref"], sp["ranges_qry"], sp["guess"])
    assert first[0].all()
    g1 = _mirror(ctx, r)
    assert g1.computeMap()
    second = m.closeScanMatching(sp["ranges_ref"], sp["ranges_qry"], sp["guess"])
    g2 = _mirror(ctx, r)
    assert g2.computeMap()
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for k in ("hits", "misses", "image"):
        assert getattr(g1, k).tobytes() == getattr(g2, k).tobytes()
        np.testing.assert_array_equal(getattr(g1, k), r[k])
