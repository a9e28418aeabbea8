"""cgmr_scan_transforms (include/cgmr.h), the host half of the device-pointer multi-scan matcher call: (cos, sin, tx, ty) of
(origin^-1 * v_k) * laserPose per reference scan, pure host code, against a plain Python restatement with math.cos / math.sin.

The bar is derived, not measured: both sides form the same expressions in float64, so an output differs only by the two
libm's sines and cosines (1 ulp each) carried through one product and two sums -- 4 units in the last place of the
largest term of each output.  The library compiles this file without contraction (csrc/Makefile: -ffp-contract=off) and
calls the same libm as Python does, so on top of that bar the values are expected bit-equal, and that is asserted too:
what cgmr_match_close_vset_batch computes on the host is what a caller of the _dev entry gets from cgmr_scan_transforms."""
import ctypes as C
import math

import numpy as np

import vset_cases as VC
from cg_mrslam_amd import _lib
from cg_mrslam_amd.matcher import MatcherConfig

NEW = ("cgmr_match_close_vset_batch_dev", "cgmr_scan_transforms")
LASER_POSE = (0.27, -0.11, 0.2)       # 3.1 + 0.2 crosses pi


def _config(laser_pose):
    sp = VC._sp()
    cfg = MatcherConfig()
    _lib.load_library().cgmr_matcher_config_close(C.byref(cfg), C.c_int(sp["n_beams"]), C.c_double(sp["angle_min"]),
                                                  C.c_double(sp["angle_inc"]), C.c_double(sp["max_range"]))
    for k in range(3):
        cfg.laser_pose[k] = laser_pose[k]
    return cfg


def _call(cfg, rel):
    rel = np.ascontiguousarray(rel, dtype=np.float64).reshape(-1, 3)
    out = np.full((len(rel), 4), np.nan)
    rc = _lib.load_library().cgmr_scan_transforms(C.byref(cfg), C.c_int(len(rel)), C.c_void_p(rel.ctypes.data),
                                                  C.c_void_p(out.ctypes.data))
    return rc, out


def _restated(rel, lp):
    """(the four outputs, the largest term of each) of rel o laserPose, the heading wrapped to [-pi, pi)."""
    c, s = math.cos(rel[2]), math.sin(rel[2])
    t = rel[2] + lp[2]
    if not (-math.pi <= t < math.pi):
        t = t - 2 * math.pi * math.floor((t + math.pi) / (2 * math.pi))
    out = (math.cos(t), math.sin(t), rel[0] + (c * lp[0] - s * lp[1]), rel[1] + (s * lp[0] + c * lp[1]))
    terms = (abs(out[0]), abs(out[1]), max(abs(rel[0]), abs(c * lp[0]), abs(s * lp[1]), abs(out[2])),
             max(abs(rel[1]), abs(s * lp[0]), abs(c * lp[1]), abs(out[3])))
    return out, terms, t


def _inputs():
    rel = VC.plain_sets()[1].reshape(-1, 3)
    assert rel.shape == (30, 3) and np.any(rel[:, 2] != 0)
    edge = [[1.5, -2.0, h] for h in (math.pi, -math.pi, math.pi - 1e-16, 3.1, 100.0, -100.0, 0.0)]
    return np.concatenate([rel, np.array(edge)])


def test_the_library_exports_the_device_resident_matcher_entry_points():
    lib = _lib.load_library()
    declared = _lib.declared_symbols()
    for n in NEW:
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    assert "cgmr_ctx_stream" in declared and hasattr(lib, "cgmr_ctx_stream")


# every device-pointer entry point of include/cgmr.h -> a GPU test file that runs it against its host twin
DEV_ENTRIES = {
    "cgmr_gn_optimize_dev": "test_gn_gpu.py", "cgmr_gn_optimize_robust_dev": "test_robust_gpu.py",
    "cgmr_lm_optimize_robust_dev": "test_robust_gpu.py", "cgmr_gnc_optimize_dev": "test_gnc_gpu.py",
    "cgmr_chordal_initialize_dev": "test_chordal_gpu.py", "cgmr_gn_optimize_mixture_dev": "test_mixture_gpu.py",
    "cgmr_lm_optimize_mixture_dev": "test_mixture_gpu.py", "cgmr_dl_optimize_mixture_dev": "test_mixture_gpu.py",
    "cgmr_match_close_batch_dev": "test_matcher_config_gpu.py",
    "cgmr_lm_optimize_dev": "test_device_resident_gpu.py", "cgmr_dl_optimize_dev": "test_device_resident_gpu.py",
    "cgmr_gn_optimize_typed_dev": "test_device_resident_gpu.py", "cgmr_lm_optimize_typed_dev": "test_device_resident_gpu.py",
    "cgmr_dl_optimize_typed_dev": "test_device_resident_gpu.py", "cgmr_chordal_initialize_typed_dev": "test_device_resident_gpu.py",
    "cgmr_match_close_vset_batch_dev": "test_device_resident_gpu.py",
}


def test_every_device_pointer_entry_point_has_a_gpu_test():
    """A _dev entry point added to the header without a line here fails this test: say which GPU test runs it.  The files
    named call the Python method of the entry point (the C name less cgmr_; the matcher's: closeScanMatching[VSet]_dev)."""
    import os
    lib = _lib.load_library()
    declared = [n for n in _lib.declared_symbols() if n.endswith("_dev")]
    assert sorted(declared) == sorted(DEV_ENTRIES)
    here = os.path.dirname(os.path.abspath(__file__))
    method = {"cgmr_match_close_batch_dev": "closeScanMatching_dev", "cgmr_match_close_vset_batch_dev": "closeScanMatchingVSet_dev",
              "cgmr_chordal_initialize_typed_dev": "chordal_initialize_dev"}       # (the typed entry: the same method with kinds)
    for name, where in DEV_ENTRIES.items():
        assert hasattr(lib, name), name
        text = open(os.path.join(here, where)).read()
        m = method.get(name, name[len("cgmr_"):])
        stem = m[:-len("_optimize_mixture_dev")] if m.endswith("_optimize_mixture_dev") else None
        assert ("." + m + "(") in text or (stem and '_optimize_mixture_dev")' in text), (name, where)


def test_scan_transforms_against_a_python_restatement():
    worst = 0.0
    for lp in (LASER_POSE, (0.0, 0.0, 0.0), (-0.4, 0.3, -3.0)):
        rel = _inputs()
        rc, got = _call(_config(lp), rel)
        assert rc == 0
        crossed = 0
        for k in range(len(rel)):
            want, terms, t = _restated(rel[k], lp)
            assert -math.pi <= t < math.pi, (k, t)
            crossed += not (-math.pi <= rel[k, 2] + lp[2] < math.pi)
            for q in range(4):
                ulp = float(np.spacing(terms[q])) if terms[q] > 0 else 5e-324
                err = abs(got[k, q] - want[q]) / ulp
                worst = max(worst, err)
                assert err <= 4, (lp, k, q, got[k, q], want[q], err)
            # bit-equal on top of the bar: the same expressions, no contraction, the same libm
            assert got[k].tobytes() == np.array(want).tobytes(), (lp, k, got[k], want)
        assert crossed >= 2                                     # (100, -100, and with a laser heading 3.1 + lt or -pi + lt)
    print(f"largest difference to the restatement: {worst} ulp of the largest term")


def test_the_wrap_is_into_minus_pi_pi():
    """Headings at the ends of the interval: +pi wraps to -pi (cos -1, sin -0 = sin(-pi) exactly as libm gives it), -pi stays,
    3.1 + 0.2 lands below -pi + 0.17."""
    cfg = _config((0.0, 0.0, 0.0))
    rc, got = _call(cfg, [[0.0, 0.0, math.pi], [0.0, 0.0, -math.pi]])
    assert rc == 0
    assert got[0].tobytes() == got[1].tobytes()
    assert got[1, 0] == math.cos(-math.pi) and got[1, 1] == math.sin(-math.pi)
    rc, got = _call(_config(LASER_POSE), [[0.0, 0.0, 3.1]])
    t = math.atan2(got[0, 1], got[0, 0])
    assert rc == 0 and -math.pi <= t < -math.pi + 0.17


def test_no_scans_and_null_arguments():
    lib = _lib.load_library()
    cfg = _config(LASER_POSE)
    out = np.full(4, 7.0)
    assert lib.cgmr_scan_transforms(C.byref(cfg), C.c_int(0), None, None) == 0
    assert lib.cgmr_scan_transforms(C.byref(cfg), C.c_int(0), None, C.c_void_p(out.ctypes.data)) == 0
    assert np.all(out == 7.0)
    rel = np.zeros(3)
    assert lib.cgmr_scan_transforms(None, C.c_int(1), C.c_void_p(rel.ctypes.data), C.c_void_p(out.ctypes.data)) == -1
    assert lib.cgmr_scan_transforms(C.byref(cfg), C.c_int(1), None, C.c_void_p(out.ctypes.data)) == -1
    assert lib.cgmr_scan_transforms(C.byref(cfg), C.c_int(1), C.c_void_p(rel.ctypes.data), None) == -1
    assert lib.cgmr_scan_transforms(C.byref(cfg), C.c_int(-1), C.c_void_p(rel.ctypes.data), C.c_void_p(out.ctypes.data)) == -1
    assert np.all(out == 7.0)


def test_the_staging_threshold_sits_between_two_batch_sizes():
    """vset_cases.in_bytes restates the library's layout; the GPU test runs one batch on each side of the threshold."""
    B = VC._sp()["n_beams"]
    P = VC.pairs_across_threshold(3, B)
    assert VC.in_bytes(P, 3, B) > VC.STAGING_THRESHOLD >= VC.in_bytes(P - 1, 3, B)
    assert VC.in_bytes(1, 3, 8) == 3 * 8 * 4 + 3 * 32 + 8 * 4 + 24
    assert VC.in_bytes(1, 1, 5) == 24 + 32 + 24 + 24              # (20 and 20 bytes of ranges, each rounded up to 8)
