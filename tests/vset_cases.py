"""The multi-scan reference sets the device-pointer and caller-stream matcher checks run on (tests/test_device_resident_cpu.py,
tests/test_device_resident_gpu.py, tests/test_caller_stream_gpu.py): the ten three-scan sets of
tests/test_matcher_config_gpu.py with the edits its multi-scan test makes, their oracle expectation computed once per
process and entry, and the byte count by which cgmr_match_close_vset_batch picks its staging path.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import matcher_configs as MC
from test_matcher_config_gpu import MAX_SCORE, VSET_ENTRIES, _sp, _vsets   # noqa: F401  (re-exported)

N_SETS = 10
STAGING_THRESHOLD = 4 << 20           # csrc/matcher_api.cpp, cgmr_match_close_vset_batch: in_bytes above it are copied unstaged
_CACHE = {}


def plain_sets():
    """(ref [10, 3, B], rel [10, 3, 3], cur [10, B], guess [10, 3]) as _vsets(10) makes them: shared, read-only."""
    if "plain" not in _CACHE:
        ref, rel, cur, guess = _vsets(N_SETS)
        _CACHE["plain"] = (np.ascontiguousarray(ref, dtype=np.float32), np.ascontiguousarray(rel, dtype=np.float64),
                           np.ascontiguousarray(cur, dtype=np.float32), np.ascontiguousarray(guess, dtype=np.float64))
    return _CACHE["plain"]


def sets(name):
    """(cfg, ref, rel, cur, guess) of a table entry: the ten sets with the edits of
    test_multi_scan_reference_sets_at_table_entries.  Built once per entry and shared: read-only."""
    key = ("sets", name)
    if key not in _CACHE:
        ref, rel, cur, guess = (a.copy() for a in plain_sets())
        cfg = MC.full_config(name, _sp())
        ref[7, 1] = 0.0                                                  # a set padded with a scan without a valid beam
        cur[8] = 100.0                                                   # an empty current scan
        ref[9] = cfg["max_range"] - 0.01                                 # far points in every scan of the set
        guess[6] = [cfg["ur"][0] - 0.05, cfg["ll"][1] + 0.05, 3.1]       # window off the corner, across pi
        _CACHE[key] = (cfg, ref, rel, cur, guess)
    return _CACHE[key]


def expected(oracle, name):
    """The oracle's answer for the ten sets of ``sets(name)`` in the arrays the C ABI returns: found [10] bool, xyt [10, 3],
    score [10], nres [10].  Computed once per entry and shared: read-only."""
    key = ("want", name)
    if key not in _CACHE:
        cfg, ref, rel, cur, guess = sets(name)
        want = [MC.expected_close_vset(oracle, cfg, ref[k], rel[k], cur[k], guess[k], MAX_SCORE) for k in range(N_SETS)]
        assert sum(w[0] for w in want[:6]) >= 5                          # (the parity is not about nothing)
        _CACHE[key] = (np.array([w[0] for w in want], dtype=bool), np.array([w[1][:3] for w in want]),
                       np.array([w[1][3] for w in want]), np.array([w[2] for w in want], dtype=np.int32))
    return _CACHE[key]


def in_bytes(n_pairs, n_ref_scans, n_beams):
    """The input bytes of a cgmr_match_close_vset_batch call as csrc/matcher_api.cpp lays them out: reference ranges,
    transforms, current ranges, guesses, each starting on 8 bytes."""
    def r8(v):
        return (v + 7) & ~7
    ns = n_pairs * n_ref_scans
    o_xf = r8(ns * n_beams * 4)
    o_qry = o_xf + ns * 32
    o_g = r8(o_qry + n_pairs * n_beams * 4)
    return o_g + n_pairs * 24


def pairs_across_threshold(n_ref_scans, n_beams):
    """The smallest number of pairs whose input exceeds STAGING_THRESHOLD."""
    P = 1
    while in_bytes(P, n_ref_scans, n_beams) <= STAGING_THRESHOLD:
        P += 1
    return P
