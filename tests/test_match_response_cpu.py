"""CPU-side checks of the scan matcher's response surface (include/cgmr.h, "Scan-match covariance"): the host-only
finishing arithmetic against numpy, the argument checks that need no device, and the float64 yardstick the GPU tests
compare with (tests/ref_match_response.py) on the configuration it was written on."""
import ctypes as C
import math

import numpy as np
import pytest

from cg_mrslam_amd import _lib
from cg_mrslam_amd.matcher import MatcherConfig, MatchResponse, ResponseJob

import ref_match_response as R

NEW = ("cgmr_match_response", "cgmr_match_response_batch", "cgmr_close_scan_matching_cov", "cgmr_match_response_information")


def test_the_library_exports_the_response_entry_points():
    lib = _lib.load_library()
    declared = _lib.declared_symbols()
    for n in NEW:
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    assert C.sizeof(MatchResponse) == 8 * (3 + 9 + 9 + 2) + 8 + 4 + 4


def _information(cov, theta, sx, sy, tr):
    lib = _lib.load_library()
    cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(9)
    out = np.full(9, np.nan)
    rc = lib.cgmr_match_response_information(C.c_void_p(cov.ctypes.data), C.c_double(theta), C.c_double(sx), C.c_double(sy),
                                             C.c_double(tr), C.c_void_p(out.ctypes.data))
    return rc, out.reshape(3, 3)


@pytest.mark.parametrize("name,cov,theta", [
    ("diagonal", np.diag([4e-4, 9e-6, 1e-5]), 0.0),
    ("rotated by pi/2", np.array([[4e-4, 1e-5, 2e-6], [1e-5, 9e-6, -1e-6], [2e-6, -1e-6, 1e-5]]), math.pi / 2),
    ("zero: the floor alone", np.zeros((3, 3)), 0.7),
])
def test_information_from_a_covariance(name, cov, theta):
    sx, sy, tr = 0.05, 0.1, 0.02
    rc, got = _information(cov, theta, sx, sy, tr)
    assert rc == 0
    want = R.information(cov, theta, sx, sy, tr)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), name
    if name.startswith("zero"):                                   # (x and y steps differ: the rotation shows in the floor as well)
        assert abs(got[2, 2] - 12.0 / tr ** 2) <= 1e-9 * got[2, 2] and abs(got[0, 1]) > 0
    if name.startswith("rotated"):                                # x of the search is -y of the measurement's frame
        assert abs(got[1, 1] - np.linalg.inv(cov + np.diag([sx ** 2, sy ** 2, tr ** 2]) / 12)[0, 0]) <= 1e-9 * got[1, 1]


def test_information_rejects_what_it_cannot_invert():
    rc, out = _information(np.zeros((3, 3)), 0.0, 0.0, 0.05, 0.02)           # singular: no step along x
    assert rc < 0 and not out.any()
    rc, out = _information(np.full((3, 3), np.nan), 0.0, 0.05, 0.05, 0.02)
    assert rc < 0 and not out.any()
    assert _lib.load_library().cgmr_match_response_information(None, C.c_double(0), C.c_double(1), C.c_double(1), C.c_double(1), None) < 0


def test_bad_arguments_are_rejected_without_a_device():
    """No context can exist without a device: every call must turn a missing one down before it looks at anything else --
    with a bad temperature, two regions or null pointers beside it -- and leave the outputs alone."""
    lib = _lib.load_library()
    E_INVALID = lib.cgmr_match_last_stats(None, (C.c_int64 * 4)())    # (the code every entry point returns for a null context)
    assert E_INVALID < 0
    cfg = MatcherConfig()
    lib.cgmr_matcher_config_close(C.byref(cfg), C.c_int(1081), C.c_double(-2.35), C.c_double(0.004), C.c_double(30.0))
    pts = np.zeros((4, 2))
    reg = np.tile(R.region_around((0, 0, 0)), 2)
    win = np.zeros(4)
    out = MatchResponse()
    out.status = 77
    for T in (0.01, 0.0, -1.0, float("nan")):
        rc = lib.cgmr_match_response(None, C.byref(cfg), C.c_int(4), C.c_void_p(pts.ctypes.data), C.c_int(4), C.c_void_p(pts.ctypes.data),
                                     C.c_void_p(reg.ctypes.data), C.c_double(0.05), C.c_double(0.05), C.c_double(0.02), C.c_double(T),
                                     C.c_void_p(win.ctypes.data), C.byref(out))
        assert rc == E_INVALID and out.status == 77
        job = ResponseJob(4, pts.ctypes.data, 4, pts.ctypes.data, 2, reg.ctypes.data, (C.c_double * 4)(), 1)      # two regions
        rc = lib.cgmr_match_response_batch(None, C.byref(cfg), C.c_int(1), C.byref(job), C.c_double(0.05), C.c_double(0.05),
                                           C.c_double(0.02), C.c_double(T), C.byref(out))
        assert rc == E_INVALID and out.status == 77
        trel, found, info = (C.c_double * 3)(), C.c_int(5), (C.c_double * 9)(*([3.0] * 9))
        rc = lib.cgmr_close_scan_matching_cov(None, C.byref(cfg), None, None, None, C.c_double(0.15), C.c_double(T), trel,
                                              C.byref(found), info, C.byref(out))
        assert rc == E_INVALID and found.value == 5 and info[0] == 3.0 and out.status == 77
    assert lib.cgmr_match_response(None, None, C.c_int(0), None, C.c_int(0), None, None, C.c_double(0), C.c_double(0), C.c_double(0),
                                   C.c_double(0.01), None, None) == E_INVALID


def test_yardstick_on_the_configuration_it_was_written_on(oracle):
    """[-5, 5]^2 at 0.05 m, kernel range 0.2, region +-(0.2, 0.2, 0.04), theta_res 0.02: all 8 * 8 * 4 = 256 candidates,
    each in a bin of its own, the winner at the origin."""
    for scene in (R.corridor(), R.room()):
        c = R.candidates(oracle, R.GRID, scene, scene[::2], R.region_around((0, 0, 0)), R.THETA_RES)
        assert c.shape == (256, 4)
        assert len(np.unique(c[:, 0])) == 8 and len(np.unique(c[:, 1])) == 8 and len(np.unique(c[:, 2])) == 4
        assert len({tuple(r[:3]) for r in c}) == 256
        assert c[0][0] == 0 and c[0][1] == 0 and abs(c[0][2]) < 1e-8 and np.all(np.diff(c[:, 3]) >= 0)
        r = R.response(c, c[0], 0.01, R.GRID, R.THETA_RES)
        assert r["status"] == 0 and r["n_candidates"] == 256 and r["mass"] >= 1.0 and 0 < r["border_mass"] < 1
        assert np.allclose(r["cov"], r["cov"].T, rtol=0, atol=1e-18) and np.all(np.linalg.eigvalsh(r["cov"]) > 0)
        assert np.allclose(r["info"] @ (r["cov"] + np.diag([0.05 ** 2, 0.05 ** 2, 0.02 ** 2]) / 12), np.eye(3), atol=1e-6)   # theta* ~ 0: J ~ 1
    assert R.response(c[:0], c[0], 0.01, R.GRID, R.THETA_RES)["status"] == 1
    assert R.response(c, None, 0.01, R.GRID, R.THETA_RES)["status"] == 2
