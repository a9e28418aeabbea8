"""CPU-side checks of the product library: it loads, exports every symbol include/cgmr.h declares,
its host-only symbolic analysis produces a valid elimination order, and the .g2o reader/writer
round-trips.  No compute entry point is called (no GPU here)."""
import ctypes
import os

import numpy as np
import pytest

from cg_mrslam_amd import _lib, synth
from cg_mrslam_amd.graph import PoseGraph


def test_library_exports_every_declared_symbol():
    lib = _lib.load_library()
    names = _lib.declared_symbols()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), f"libcgmr.so does not export {n}"
    assert lib.cgmr_version() >= 100


def test_ctx_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.CgmrError):
        _lib.Context(0)


@pytest.mark.parametrize("V,E,seed", [(2, 1, 1), (17, 16, 2), (300, 800, 3), (3000, 11000, 4)])
def test_symbolic_permutation_is_valid(V, E, seed):
    g = synth.make_pose_graph(V, E, seed=seed)
    info, perm = _lib.gn_symbolic_info(V, g["fixed"], g["edge_from"], g["edge_to"], want_perm=True)
    cols = perm[perm >= 0]
    # every vertex with an edge owns a column: the fixed flags are applied numerically (masked rows / columns), so
    # the analysis depends on the edge list only and can be reused whatever is fixed
    assert info["free_poses"] == V == len(cols)
    assert sorted(cols.tolist()) == list(range(V))             # a permutation of the block columns
    assert info["fronts"] >= 1 and info["levels"] >= 1
    assert info["max_border"] * 3 < 32000                      # index maps are staged as int16 on the device


def test_symbolic_handles_disconnected_and_inactive_vertices():
    # two components, one isolated vertex, one fixed vertex in each component
    ef = np.array([0, 1, 3, 4], dtype=np.int32)
    et = np.array([1, 2, 4, 5], dtype=np.int32)
    fixed = np.array([1, 0, 0, 1, 0, 0, 0], dtype=np.uint8)    # vertex 6 has no edge
    info, perm = _lib.gn_symbolic_info(7, fixed, ef, et, want_perm=True)
    assert info["free_poses"] == 6                             # the fixed vertices keep their (masked) columns
    assert perm[6] == -1 and perm[0] >= 0 and perm[3] >= 0      # only the vertex without an edge is left out


def test_symbolic_rejects_bad_indices():
    with pytest.raises(_lib.CgmrError):
        _lib.gn_symbolic_info(3, np.zeros(3, np.uint8), np.array([0], np.int32), np.array([7], np.int32))


def test_g2o_round_trip(tmp_path):
    g = synth.make_pose_graph(40, 90, seed=8, id_base=10000)
    pg = PoseGraph.from_synth(g)
    path = os.path.join(tmp_path, "a.g2o")
    pg.save_g2o(path, precision=17)
    back = PoseGraph.load_g2o(path)
    np.testing.assert_array_equal(back.ids, pg.ids)
    np.testing.assert_array_equal(back.fixed, pg.fixed)
    np.testing.assert_array_equal(back.edge_from, pg.edge_from)
    np.testing.assert_allclose(back.poses, pg.poses, rtol=0, atol=0)
    np.testing.assert_allclose(back.meas, pg.meas, rtol=0, atol=0)
    # default precision is g2o's lossy 6 significant digits
    pg.save_g2o(path)
    lossy = PoseGraph.load_g2o(path)
    assert np.abs(lossy.poses - pg.poses).max() < 1e-3


def test_g2o_robotlaser1_lines(tmp_path):
    """ROBOTLASER1 data lines (RobotLaser::read/write [g2o-recalled]): parse a line laid out
    by hand from the format, round-trip a graph with scans, and keep the solve arrays unaffected."""
    from cg_mrslam_amd.graph import PoseGraph, RobotLaser
    line = ("ROBOTLASER1 0 -1.5708 3.14159 0.785398 30 0.1 0 5 1.5 2 2.5 3 81.91 0 "
            "1.2 0.4 0.6 1 0.3 0.6 0 0 0 0 0 1234.5 robot1 1234.6")
    l = RobotLaser.read(line.split())
    assert l.laser_type == 0 and len(l.ranges) == 5 and l.ranges[4] == np.float32(81.91) and len(l.remissions) == 0
    assert l.first_beam_angle == -1.5708 and l.fov == 3.14159 and l.angular_step == 0.785398 and l.max_range == 30
    np.testing.assert_allclose(l.odom_pose, [1, 0.3, 0.6])
    # laser pose on the robot = odom^-1 * world pose: a pure forward offset of 0.2236... rotated back
    c, s = np.cos(0.6), np.sin(0.6)
    np.testing.assert_allclose(l.laser_pose, [c * 0.2 + s * 0.1, -s * 0.2 + c * 0.1, 0.0], atol=1e-12)
    assert l.hostname == "robot1" and l.timestamp == "1234.5"
    assert l.write().split()[:9] == line.split()[:9]

    g = synth.make_pose_graph(12, 20, seed=3)
    pg = PoseGraph.from_synth(g)
    rng = np.random.default_rng(0)
    for k in (0, 3, 11):
        pg.lasers[k] = RobotLaser(rng.uniform(0.5, 20, size=181).astype(np.float32), -1.57, 0.0174533, 30.0,
                                  odom_pose=pg.poses[k], laser_pose=(0.1, 0.0, 0.02))
    path = tmp_path / "with_lasers.g2o"
    pg.save_g2o(path, precision=17)
    back = PoseGraph.load_g2o(path)
    np.testing.assert_array_equal(back.poses, pg.poses)
    np.testing.assert_array_equal(back.meas, pg.meas)
    assert sorted(back.lasers) == [0, 3, 11]
    for k in (0, 3, 11):
        np.testing.assert_array_equal(back.lasers[k].ranges, pg.lasers[k].ranges)
        np.testing.assert_allclose(back.lasers[k].laser_pose, [0.1, 0.0, 0.02], atol=1e-15)
        np.testing.assert_allclose(back.lasers[k].odom_pose, pg.poses[k], atol=0)
    text = open(path).read().splitlines()
    assert text[0].startswith("VERTEX_SE2") and text[1].startswith("ROBOTLASER1") and text[2].startswith("FIX")


_SYM_HASH = r"""
import sys, ctypes as C, numpy as np, hashlib
sys.path.insert(0, sys.argv[1])
from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import load_library, gn_symbolic_info
lib = load_library()
h = hashlib.md5()
for (V, E, seed) in ((10000, 40000, 12345), (3000, 9000, 7), (800, 2000, 3), (40, 60, 1)):
    g = synth.make_pose_graph(V, E, seed=seed)
    fx = np.ascontiguousarray(g["fixed"], dtype=np.uint8)
    ef = np.ascontiguousarray(g["edge_from"], dtype=np.int32)
    et = np.ascontiguousarray(g["edge_to"], dtype=np.int32)
    out = np.zeros(20000 * 6, dtype=np.int32)
    n = lib.cgmr_debug_fronts(C.c_int(V), C.c_void_p(fx.ctypes.data), C.c_int(len(ef)), C.c_void_p(ef.ctypes.data),
                              C.c_void_p(et.ctypes.data), C.c_int(20000), C.c_void_p(out.ctypes.data))
    info, perm = gn_symbolic_info(V, fx, ef, et, want_perm=True)
    h.update(out[:6 * n].tobytes()); h.update(perm.tobytes())
    h.update(str({k: v for k, v in info.items() if not k.endswith("_us")}).encode())
print(h.hexdigest())
"""


def test_symbolic_analysis_independent_of_host_threads():
    """The parallel sections of the host analysis (ND forks, border computation per subtree, keyed assembly lists)
    must give the ordering, the front table and the sizes of the one-thread run: the thread count is read once per
    process, hence subprocesses."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hashes = []
    for nt in ("1", "3", "8"):
        env = dict(os.environ, CGMR_HOST_THREADS=nt)
        out = subprocess.run([sys.executable, "-c", _SYM_HASH, root], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        hashes.append(out.stdout.strip().splitlines()[-1])
    assert hashes[0] == hashes[1] == hashes[2], hashes


def _front_table(V, fixed, ef, et):
    import ctypes as C
    from cg_mrslam_amd._lib import load_library, gn_symbolic_info
    lib = load_library()
    fx = np.ascontiguousarray(fixed, dtype=np.uint8)
    ef = np.ascontiguousarray(ef, dtype=np.int32)
    et = np.ascontiguousarray(et, dtype=np.int32)
    out = np.zeros(60000 * 6, dtype=np.int32)
    n = lib.cgmr_debug_fronts(C.c_int(V), C.c_void_p(fx.ctypes.data), C.c_int(len(ef)), C.c_void_p(ef.ctypes.data),
                              C.c_void_p(et.ctypes.data), C.c_int(60000), C.c_void_p(out.ctypes.data))
    assert 0 <= n <= 60000
    info, perm = gn_symbolic_info(V, fx, ef, et, want_perm=True)
    return out[:6 * n].reshape(n, 6), info, perm


def _assert_valid_elimination_tree(V, fixed, ef, et, table=None):
    """Front table = (c0, nc, ns, parent, level, nchild).  The fronts tile the permuted columns, hold <= 16 poses, parents
    come later and sit on a higher level, and for every edge the front of the later column is an ancestor (or the
    front itself) of the front of the earlier one -- the property the level-by-level factorisation relies on."""
    F, info, perm = table if table is not None else _front_table(V, fixed, ef, et)
    nf = info["free_poses"]
    n = len(F)
    assert n == info["fronts"]
    if n == 0:
        return
    assert F[0, 0] == 0 and np.all(F[1:, 0] == F[:-1, 0] + F[:-1, 1]) and F[-1, 0] + F[-1, 1] == nf
    assert F[:, 1].min() >= 1 and F[:, 1].max() <= 16
    col_front = np.repeat(np.arange(n), F[:, 1])
    parent, level = F[:, 3], F[:, 4]
    has_p = parent >= 0
    assert np.all(parent[has_p] > np.nonzero(has_p)[0]) and np.all(level[parent[has_p]] > level[has_p])
    assert level.max() + 1 == info["levels"]
    assert sorted(perm[perm >= 0].tolist()) == list(range(nf))
    for a, b in zip(ef, et):
        ca, cb = perm[a], perm[b]
        if ca < 0 or cb < 0 or ca == cb:
            continue
        f, g = col_front[min(ca, cb)], col_front[max(ca, cb)]
        while f != g and 0 <= f < g:
            f = parent[f]
        assert f == g, (a, b)


@pytest.mark.parametrize("V,E,seed", [(10000, 40000, 12345), (2500, 9000, 5), (500, 1500, 4), (60, 100, 2), (17, 16, 1)])
def test_elimination_tree_valid_random_walks(V, E, seed):
    g = synth.make_pose_graph(V, E, seed=seed)
    _assert_valid_elimination_tree(V, g["fixed"], g["edge_from"], g["edge_to"])


def test_elimination_tree_valid_special_shapes():
    for g in (synth.make_hub_graph(40, 30, 3), synth.make_hub_graph(24, 40, 4), synth.make_lattice_graph(40)):
        _assert_valid_elimination_tree(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    # sub-graphs as the condensed-graph creator sees them: own edges only, gauge in the middle, foreign vertices inactive
    for seed in (46, 49, 53):
        R = synth.make_multi_robot(2, 1200, 4000, seed=seed)
        for r in range(2):
            gr = R[r]
            V, n_own = len(gr["poses_all"]), gr["n_own"]
            m = (gr["ef_all"] < n_own) & (gr["et_all"] < n_own)
            for gauge in (0, n_own // 2):
                fixed = np.zeros(V, dtype=np.uint8)
                fixed[gauge] = 1
                _assert_valid_elimination_tree(V, fixed, gr["ef_all"][m], gr["et_all"][m])
    # two disconnected components, duplicate edges, several fixed vertices
    g = synth.make_pose_graph(300, 700, seed=9)
    ef = np.concatenate([g["edge_from"], g["edge_from"][:50], g["edge_from"] + 300])
    et = np.concatenate([g["edge_to"], g["edge_to"][:50], g["edge_to"] + 300])
    fixed = np.zeros(600, dtype=np.uint8)
    fixed[[0, 17, 300, 455]] = 1
    _assert_valid_elimination_tree(600, fixed, ef, et)


def test_host_threads_info_reports_the_pool_as_it_runs():
    """cgmr_host_threads_info: thread count as CGMR_HOST_THREADS / the core count give it, a home CPU exactly when pinned, a
    home the process may run on (what the bench line carries as `host_pool`)."""
    import ctypes as C
    lib = _lib.load_library()
    out = (C.c_int32 * 5)()
    assert lib.cgmr_host_threads_info(out) == 0
    threads, pinned, home, allowed, moves = list(out)
    assert moves >= 0
    assert 1 <= threads <= 16 and allowed == len(os.sched_getaffinity(0))
    assert (home >= 0) == bool(pinned)
    if pinned:
        assert home in os.sched_getaffinity(0)
    assert lib.cgmr_host_threads_info(None) != 0


def test_symbolic_analysis_leaves_the_callers_affinity_alone():
    """The analysis holds the calling thread on its home core while it runs (the helper threads sit around it); the
    affinity mask must be the caller's own again afterwards, whatever the analysis did, and also in a child process started
    with the library's switches off."""
    import subprocess, sys
    from cg_mrslam_amd._lib import gn_symbolic_info
    g = synth.make_pose_graph(3000, 9000, seed=5)
    before = os.sched_getaffinity(0)
    for _ in range(3):
        gn_symbolic_info(3000, g["fixed"], g["edge_from"], g["edge_to"])
        assert os.sched_getaffinity(0) == before
    code = ("import os\nfrom cg_mrslam_amd import synth\nfrom cg_mrslam_amd._lib import gn_symbolic_info\n"
            "g = synth.make_pose_graph(3000, 9000, seed=5)\nb = os.sched_getaffinity(0)\n"
            "i = gn_symbolic_info(3000, g['fixed'], g['edge_from'], g['edge_to'])\nassert os.sched_getaffinity(0) == b\nprint('ok', i['levels'])\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for env in ({"CGMR_HOST_THREADS": "8"}, {"CGMR_HOST_THREADS": "8", "CGMR_HOST_PIN": "0"}, {"CGMR_HOST_THREADS": "8", "LOCAL_RANK": "1", "LOCAL_WORLD_SIZE": "2"}):
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, PYTHONPATH=root, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-1500:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] == outs[2]                      # same tree whatever the placement


def test_symbolic_analysis_survives_fork():
    """The helper threads do not exist in a forked child: the analysis must fall back to the calling thread there
    instead of queueing work for them (gloo / multiprocessing workers fork after the parent has used the library)."""
    import os
    import signal
    from cg_mrslam_amd._lib import gn_symbolic_info
    g = synth.make_pose_graph(6000, 20000, seed=21)
    want = gn_symbolic_info(6000, g["fixed"], g["edge_from"], g["edge_to"])   # creates the pool in this process
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        try:
            signal.alarm(60)
            got = gn_symbolic_info(6000, g["fixed"], g["edge_from"], g["edge_to"])
            ok = all(got[k] == want[k] for k in ("fronts", "levels", "L_doubles", "U_doubles", "max_border"))
            os.write(w, b"1" if ok else b"0")
        finally:
            os._exit(0)
    os.close(w)
    _, status = os.waitpid(pid, 0)
    assert os.read(r, 1) == b"1" and status == 0


def test_symbolic_analysis_concurrent_callers():
    """Several threads analysing different graphs at once (ctypes releases the GIL; the helper pool is shared): every
    call must return what it returns alone."""
    import threading
    from cg_mrslam_amd._lib import gn_symbolic_info
    graphs = [synth.make_pose_graph(V, E, seed=s) for (V, E, s) in ((6000, 20000, 31), (3000, 12000, 32), (9000, 30000, 33), (1500, 4000, 34))]
    keys = ("fronts", "levels", "L_doubles", "U_doubles", "max_border", "factor_flops")

    def analyse(g):
        info, perm = gn_symbolic_info(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"], want_perm=True)
        return tuple(info[k] for k in keys), perm.tobytes()

    want = [analyse(g) for g in graphs]
    got = [[None] * 4 for _ in graphs]

    def worker(i):
        for rep in range(4):
            got[i][rep] = analyse(graphs[i])

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(graphs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
        assert not t.is_alive()
    for i in range(len(graphs)):
        for rep in range(4):
            assert got[i][rep] == want[i]


def _c_calls(text, prefix="cgmr_"):
    """(name, number of arguments) of every call / prototype ``cgmr_xxx(...)`` in a C or C++ source text (comments and
    string literals removed, parentheses balanced, commas counted at depth 0)."""
    import re
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r'"(?:\\.|[^"\\])*"', '""', text)
    out = []
    for m in re.finditer(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text):
        i, depth, commas, empty = m.end(), 1, 0, True
        while i < len(text) and depth:
            ch = text[i]
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            elif ch == "," and depth == 1:
                commas += 1
            if depth and not ch.isspace():
                empty = False
            i += 1
        inner = text[m.end():i - 1].strip()
        out.append((m.group(1), 0 if (empty or inner == "void") else commas + 1))
    return out


def test_adapters_call_the_c_abi_with_the_declared_names_and_argument_counts():
    """adapters/g2o/*.cpp are the reference-side bindings a maintainer links; they need g2o + Eigen and have never seen a
    compiler here.  At least every ``cgmr_*`` call in them must name an entry point include/cgmr.h declares and pass the
    number of arguments its prototype has."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    protos = {}
    for name, n in _c_calls(open(os.path.join(root, "include", "cgmr.h")).read()):
        protos.setdefault(name, n)
    assert len(protos) > 60 and protos["cgmr_gn_optimize"] == 11 and protos["cgmr_version"] == 0
    files = sorted(glob.glob(os.path.join(root, "adapters", "g2o", "*.cpp")) + glob.glob(os.path.join(root, "adapters", "g2o", "*.h")))
    assert len(files) >= 5
    seen, bad = set(), []
    for f in files:
        for name, n in _c_calls(open(f).read()):
            if name.startswith("cgmr_g2o"):                       # the adapters' own helpers (namespace cgmr_g2o)
                continue
            seen.add(name)
            if name not in protos:
                bad.append(f"{os.path.basename(f)}: {name} is not declared in include/cgmr.h")
            elif protos[name] != n:
                bad.append(f"{os.path.basename(f)}: {name} called with {n} arguments, declared with {protos[name]}")
    assert not bad, "\n".join(bad)
    # the seven entry points SURVEY.md 8(b) lists are all bound
    for must in ("cgmr_gn_optimize", "cgmr_close_scan_matching", "cgmr_scan_matching_lc", "cgmr_global_matching", "cgmr_verify_matching",
                 "cgmr_covariance_estimate", "cgmr_condense"):
        assert must in seen, must


def _growing_graph(V, E, seed):
    """A synthetic pose graph whose edges are ordered by their later end point: every prefix of the vertex list has its
    edges as a prefix of the edge list (the key-frame pattern: a vertex and its edges are appended together)."""
    g = synth.make_pose_graph(V, E, seed=seed)
    k = np.argsort(np.maximum(g["edge_from"], g["edge_to"]), kind="stable")
    for name in ("edge_from", "edge_to", "meas", "info"):
        g[name] = np.ascontiguousarray(g[name][k])
    last = np.maximum(g["edge_from"], g["edge_to"])
    return g, last


def test_round5_entry_points_reject_a_missing_context_without_a_gpu():
    """The entry points added in round 5 (version 102) check their arguments before touching a device."""
    import ctypes as C
    lib = _lib.load_library()
    assert lib.cgmr_version() >= 102
    out = (C.c_int64 * 4)()
    E_INVALID = lib.cgmr_match_last_stats(None, out)                # (the code every entry point returns for a null context)
    assert E_INVALID < 0
    assert lib.cgmr_match_last_path_counts(None, out) == E_INVALID
    assert lib.cgmr_match_last_redo_pairs(None, out) == E_INVALID
    t, f = (C.c_double * 3)(), C.c_int(0)
    assert lib.cgmr_scan_matching_lc_hierarchical(None, None, None, None, C.c_double(0.3), t, C.byref(f)) == E_INVALID
    assert lib.cgmr_scan_matching_lc_hierarchical_batch(None, None, C.c_int(0), None, None, C.c_double(0.3), t, C.byref(f)) == E_INVALID
    assert lib.cgmr_graph_failed_batches(None) <= 0


def test_incremental_ordering_of_a_growing_graph():
    """The cached ordering extended by appended vertices (gn_symbolic.cpp: extend_order): the result is a valid elimination
    order, most steps re-use the ordering, and the tree stays close to what a from-scratch analysis of the final graph
    gives (levels, factorisation flops) -- for chunks of 50 (a multi-robot round) and of 1 (a key frame)."""
    from cg_mrslam_amd._lib import gn_symbolic_info, gn_symbolic_info_grown
    g, last = _growing_graph(3000, 11000, seed=8)
    for chunk, v0 in ((50, 600), (1, 2900)):
        nv = np.arange(v0 + chunk, 3000 + 1, chunk)
        ne = np.searchsorted(last, nv, side="left")              # edges whose later end point < nv
        ne0 = int(np.searchsorted(last, v0, side="left"))
        info, perm, n_ext = gn_symbolic_info_grown(v0, ne0, nv, ne, g["edge_from"], g["edge_to"])
        full = gn_symbolic_info(3000, g["fixed"], g["edge_from"], g["edge_to"])
        active = perm >= 0
        assert sorted(perm[active].tolist()) == list(range(int(active.sum())))          # a permutation of the active vertices
        assert info["free_poses"] == full["free_poses"] and info["offdiag_blocks"] == full["offdiag_blocks"]
        assert n_ext >= 0.7 * len(nv)                                                    # mostly extensions, a few re-orderings
        assert info["levels"] <= full["levels"] + 6
        assert info["factor_flops"] <= 1.6 * full["factor_flops"]


def test_points_of_a_scan_set_with_changing_lasers():
    """transformPointsFromVSet on the host (no GPU): the beam directions come from a per-thread table keyed by the laser
    (beam count, first angle, step); lasers alternating between calls must each get their own directions, equal to the
    libm expression of ``cgmr_scan_cartesian`` point for point."""
    import ctypes as C
    import math
    from cg_mrslam_amd._lib import load_library
    from cg_mrslam_amd.matcher import MatcherConfig, ScanSet, _se2_inv, _se2_mul
    lib = load_library()
    rng = np.random.default_rng(8)
    lasers = [(181, -1.2, 0.0133), (1081, -2.35619449, 0.00436332313), (181, -1.0, 0.0133), (361, -1.57, 0.0087)]
    for rep in range(2):
        for (B, a0, da) in lasers:
            cfg = MatcherConfig()
            cfg.n_beams, cfg.angle_min, cfg.angle_inc, cfg.max_range, cfg.min_range = B, a0, da, 20.0, 0.1
            cfg.laser_pose[0], cfg.laser_pose[1], cfg.laser_pose[2] = 0.1, -0.05, 0.2
            ranges = np.ascontiguousarray(rng.uniform(0.0, 25.0, size=(3, B)).astype(np.float32))
            poses = np.ascontiguousarray(rng.uniform(-1, 1, size=(3, 3)))
            s = ScanSet(3, C.c_void_p(ranges.ctypes.data), C.c_void_p(poses.ctypes.data), 1)
            out = np.zeros((3 * B, 2))
            n = lib.cgmr_transform_points_from_vset(C.byref(cfg), C.byref(s), C.c_void_p(out.ctypes.data), C.c_int(3 * B))
            want = []
            lp = np.array([0.1, -0.05, 0.2])
            for k in range(3):
                T = lp if k == 1 else _se2_mul(_se2_mul(_se2_inv(poses[1]), poses[k]), lp)
                c, sn = math.cos(T[2]), math.sin(T[2])
                for i in range(B):
                    r = float(ranges[k, i])
                    if r < 20.0 and r > 0.1:
                        al = a0 + i * da
                        x, y = math.cos(al) * r, math.sin(al) * r
                        want.append((T[0] + (c * x - sn * y), T[1] + (sn * x + c * y)))
            assert n == len(want)
            assert np.array_equal(out[:n], np.array(want))


def test_star_centres_are_eliminated_last():
    """The condensed graph a peer sends is a star: its gauge vertex gets 30-60 edges.  Such hubs stay out of the nested
    dissection and are eliminated last (they would tie the subtrees their ends lie in together level by level): the tree of
    a pose graph with six stars is about as tall as without them, and much taller when the rule is switched off."""
    from cg_mrslam_amd._lib import gn_symbolic_info
    from switch_contexts import environment
    g = synth.make_pose_graph(5000, 20000, seed=9, strict=True)
    ef, et = list(g["edge_from"]), list(g["edge_to"])
    plain = (np.array(ef, np.int32), np.array(et, np.int32))
    rng = np.random.default_rng(4)
    hubs = []
    for h in range(6):
        c = int(rng.integers(0, 5000)); hubs.append(c)
        for v in rng.choice(5000, size=50, replace=False):
            if int(v) != c: ef.append(min(c, int(v))); et.append(max(c, int(v)))
    out = {}
    for hub in ("32", "0"):                                          # (read by the call: the analysis has no context here)
        with environment({"CGMR_HUB_DEGREE": hub}):
            base = gn_symbolic_info(5000, g["fixed"], *plain)
            info, perm = gn_symbolic_info(5000, g["fixed"], np.array(ef, np.int32), np.array(et, np.int32), want_perm=True)
        out[hub] = [base["levels"], info["levels"], base["factor_flops"], info["factor_flops"], min(int(perm[c]) for c in hubs), len(perm)]
    base_levels, levels, base_flops, flops, first_hub_col, n = out["32"]
    assert levels <= base_levels + 2 and flops <= 1.5 * base_flops
    assert first_hub_col >= n - 64                                   # the hubs sit in the last columns
    assert out["0"][1] >= levels + 5                                 # without the rule: a much taller tree


def test_extension_is_refused_when_new_edges_join_old_vertices_of_different_subtrees():
    """A grown graph may also get edges between vertices the cached ordering already holds (a loop closure between old
    poses, a condensed edge from a peer).  If their dissection-tree nodes are not on one root path the subtrees stop being
    independent: the ordering must then be rebuilt, not extended -- the parallel border computation relied on the
    independence and produced a wrong structure with more than one host thread (round 3: Cholesky failure in round 40 of
    the two-robot C5 rounds).  Checked here as: the analysis of such a sequence is the same with 1 and with 8 threads, and
    the sequence with a far cross edge is not counted as extended while the one without it is."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import numpy as np\nfrom cg_mrslam_amd import synth\nfrom cg_mrslam_amd._lib import gn_symbolic_info_grown\n"
        "g = synth.make_pose_graph(3000, 9000, seed=21, strict=True)\n"
        "ef, et = g['edge_from'], g['edge_to']\n"
        "ko = np.argsort(np.maximum(ef, et), kind='stable'); ef, et = ef[ko], et[ko]\n"
        "v0 = 2900; e0 = int(np.searchsorted(np.maximum(ef, et), v0, side='left'))\n"
        "for cross in (0, 1):\n"
        "    tail_f, tail_t = list(ef[e0:]), list(et[e0:])\n"
        "    if cross:\n"
        "        rng = np.random.default_rng(3)\n"
        "        for _ in range(40):\n"
        "            a, b = rng.integers(1, v0, size=2)\n"
        "            tail_f.append(int(min(a, b))); tail_t.append(int(max(a, b)))\n"
        "    f2 = np.concatenate([ef[:e0], np.array(tail_f, dtype=np.int32)]).astype(np.int32)\n"
        "    t2 = np.concatenate([et[:e0], np.array(tail_t, dtype=np.int32)]).astype(np.int32)\n"
        "    info, perm, next_ = gn_symbolic_info_grown(v0, e0, [3000], [len(f2)], f2, t2)\n"
        "    print(cross, next_, info['fronts'], info['levels'], info['L_doubles'], info['U_doubles'], info['factor_flops'], int(perm.sum()), int((perm * np.arange(len(perm))).sum() % 1000003))\n")
    outs = {}
    for nt in ("1", "8"):
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, PYTHONPATH=root, CGMR_HOST_THREADS=nt),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        outs[nt] = r.stdout.strip().splitlines()
    assert outs["1"] == outs["8"], (outs["1"], outs["8"])
    plain, crossed = outs["8"][0].split(), outs["8"][1].split()
    assert plain[1] == "1" and crossed[1] == "0"             # extended without the cross edges, rebuilt with them


def test_robot_graph_rounds_extend_the_ordering_with_the_received_stars_as_hubs():
    """A robot's edge list is its own edges (appended to) followed by the stars received from the peers (replaced every
    round): never a grown prefix.  With the stars' gauge vertices named as hubs (cgmr_graph_optimize does) they live in the
    root's separator, every received edge lies on a root path, and the cached ordering is extended over the own part as for
    a robot alone.  Checked on host-only C5 rounds of three robots: most rounds extend, the last analysis is a valid
    elimination tree about as tall as a from-scratch one (the height bound of the extension), the hubs sit in the last
    columns, and the sequence gives the same analysis with 1 and with 8 host threads."""
    import subprocess, sys
    from robot_sequences import robot_sequences, run_steps
    seq = robot_sequences(3, 1500, 5000, seed=31)
    for steps in seq:
        nV, ef, et, n_own, hubs = steps[-1]
        assert len(ef) > n_own and len(hubs) >= 1                               # the peers' stars are in the list
        info, perm, n_ext, fronts, per = run_steps(steps, use_hubs=True)
        _assert_valid_elimination_tree(nV, None, ef, et, table=(fronts, info, perm))
        assert n_ext >= 0.6 * (len(steps) - 1), n_ext
        scratch = run_steps([steps[-1]], use_hubs=True)[0]
        assert info["levels"] <= scratch["levels"] + 4 and info["factor_flops"] <= 1.5 * scratch["factor_flops"]
        assert perm[hubs].min() >= info["free_poses"] - 16 * 4                   # eliminated last
        assert run_steps(steps, use_hubs=False)[2] <= n_ext                      # without the hints: (almost) nothing extends
    code = ("import sys, numpy as np\nsys.path.insert(0, 'tests')\nfrom robot_sequences import robot_sequences, run_steps\n"
            "seq = robot_sequences(3, 1500, 5000, seed=31)\n"
            "for steps in seq:\n"
            "    info, perm, n_ext, fronts, per = run_steps(steps)\n"
            "    print(n_ext, info['fronts'], info['levels'], info['L_doubles'], info['U_doubles'], int((perm * np.arange(len(perm))).sum() % 1000003), int(fronts.sum()))\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for nt in ("1", "8"):
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, PYTHONPATH=root, CGMR_HOST_THREADS=nt),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        outs.append(r.stdout)
    assert outs[0] == outs[1], outs


@pytest.mark.parametrize("shape", ["walk", "hub"])
def test_children_schedule_has_one_writer_per_panel_copy_and_launch(shape):
    """The assembled-panel hand-off (gn_symbolic.cpp): every child adds into its parent's panel during one
    update launch t with level(child) <= t < level(parent), and two children of a front never share (launch, copy) -- that
    is what makes the read-modify-write sums race-free and bit-reproducible without atomics.  On a random-walk graph and on a
    hub graph whose fronts have dozens of same-level children (the parent then moves up a level)."""
    import ctypes as C
    from cg_mrslam_amd._lib import load_library
    lib = load_library()
    if shape == "walk":
        g = synth.make_pose_graph(4000, 15000, seed=5)
        V, ef, et = 4000, g["edge_from"], g["edge_to"]
    else:                                                    # 40 chains of 30 poses hanging off one hub chain
        ef, et, V = [], [], 0
        hub = list(range(30)); V = 30
        ef += hub[:-1]; et += hub[1:]
        for k in range(40):
            chain = list(range(V, V + 30)); V += 30
            ef += chain[:-1]; et += chain[1:]
            ef.append(hub[k % 30]); et.append(chain[0])
    ef, et = np.ascontiguousarray(ef, dtype=np.int32), np.ascontiguousarray(et, dtype=np.int32)
    fx = np.zeros(V, dtype=np.uint8)
    cap = 20000
    fr = np.zeros(cap * 6, dtype=np.int32)
    n = lib.cgmr_debug_fronts(C.c_int(V), C.c_void_p(fx.ctypes.data), C.c_int(len(ef)), C.c_void_p(ef.ctypes.data),
                              C.c_void_p(et.ctypes.data), C.c_int(cap), C.c_void_p(fr.ctypes.data))
    sc = np.zeros(cap * 4, dtype=np.int32)
    n2 = lib.cgmr_debug_schedule(C.c_int(V), C.c_int(len(ef)), C.c_void_p(ef.ctypes.data), C.c_void_p(et.ctypes.data), C.c_int(cap),
                                 C.c_void_p(sc.ctypes.data))
    assert n == n2 and 0 < n < cap
    fr, sc = fr[:6 * n].reshape(n, 6), sc[:4 * n].reshape(n, 4)
    parent, level = fr[:, 3], fr[:, 4]
    seen = set()
    for f in range(n):
        p = int(parent[f])
        if p < 0:
            continue
        assert level[p] > level[f] and p > f                  # parents after children, strictly higher
        if not sc[f, 3]:
            continue                                         # child of the top block: whole update matrix through Ubuf
        t, slot = int(sc[f, 0]), int(sc[f, 1])
        assert level[f] <= t < level[p]
        assert 0 <= slot < sc[p, 2] <= 3                      # kMaxPanSlots
        assert (p, t, slot) not in seen
        seen.add((p, t, slot))
    assert len(seen) > 10


def test_dead_reckoning_chain_equals_se2_compose_bit_for_bit():
    """mrslam._dead_reckon (scalar steps) against synth.se2_compose pose by pose, angles that wrap included."""
    from cg_mrslam_amd.mrslam import _dead_reckon
    rng = np.random.default_rng(5)
    inc = np.stack([rng.normal(0, 1.0, 400), rng.normal(0, 0.3, 400), rng.normal(0.4, 1.5, 400)], axis=1)
    start = np.array([0.3, -2.0, 3.0])
    got = np.array(_dead_reckon(start, inc))
    prev, want = start, []
    for k in range(len(inc)):
        prev = synth.se2_compose(prev[None], inc[k][None])[0]
        want.append(prev)
    assert np.array_equal(got, np.array(want))


def test_launch_shape_query_rejects_a_missing_context_without_a_gpu():
    import ctypes as C
    lib = _lib.load_library()
    out = (C.c_int64 * 4)()
    assert lib.cgmr_match_last_launch_shape(None, out) == lib.cgmr_match_last_stats(None, out) < 0
