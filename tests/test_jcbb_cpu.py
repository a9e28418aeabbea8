"""The joint-compatibility data association (cgmr_jcbb_dense, cgmr_joint_compatibility) as the header, the library and the
Python layers declare it, and the float64 reference of tests/ref_jcbb.py against itself on the cases of tests/jcbb_cases.py:
the exhaustive enumerator, the sequential branch and bound and the two d2 methods; no GPU needed.  tests/test_jcbb_gpu.py
checks what the entry points compute."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import jcbb_cases as JC
import ref_jcbb as RJ
from cg_mrslam_amd import _lib
from cg_mrslam_amd.graph import GraphSLAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cgmr_jcbb_dense": 19, "cgmr_joint_compatibility": 27}      # name: arguments


def _header():
    return open(os.path.join(ROOT, "include", "cgmr.h")).read()


def test_symbols_declared_listed_and_exported_version_105():
    lib = _lib.load_library()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    assert lib.cgmr_version() == 105


def test_header_argument_counts_and_constants():
    hdr = _header()
    for n, count in NAMES.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == count, (n, args)
        assert "int64_t node_limit" in args and "const double* gamma_by_dof" in args
        assert args[args.index("int64_t node_limit") + 1:][:7] == ["double* ic_d2_out", "int32_t* assign_out", "int32_t* count_out",
                                                                   "double* d2_out", "int32_t* dof_out", "int32_t* proven_out",
                                                                   "int64_t* nodes_out"]
    obs = [a.strip() for a in re.search(r"\bint\s+cgmr_observation_covariance\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")]
    jc = [a.strip() for a in re.search(r"\bint\s+cgmr_joint_compatibility\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")]
    assert jc[:9] == obs[:9] and jc[-2:] == obs[-2:] == ["const cgmr_factor_types* types", "const cgmr_robust* rk"]
    for name, value in (("CGMR_JC_MAX_OBS", _lib.JC_MAX_OBS), ("CGMR_JC_MAX_LANDMARKS", _lib.JC_MAX_LANDMARKS),
                        ("CGMR_JC_DEFAULT_NODE_LIMIT", _lib.JC_DEFAULT_NODE_LIMIT)):
        d = re.search(r"#define\s+" + name + r"\s+(\d+)", hdr)
        assert d and int(d.group(1)) == value, name
    assert (_lib.JC_MAX_OBS, _lib.JC_MAX_LANDMARKS) == (32, 256)
    lim = _lib.JC_DEFAULT_NODE_LIMIT
    assert lim > 0 and lim & (lim - 1) == 0                          # a power of two
    r = re.search(r"#define\s+CGMR_JC_ROUNDS\s+(\d+)", open(os.path.join(ROOT, "cg_mrslam_amd", "csrc", "jcbb_device.h")).read())
    assert r and int(r.group(1)) == _lib.JC_ROUNDS == 2


def test_null_context_is_invalid():
    lib = _lib.load_library()
    e_invalid = int(re.search(r"#define\s+CGMR_E_INVALID\s+\((-?\d+)\)", _header()).group(1))
    null = ctypes.c_void_p(0)
    dense = [null, ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)] + [null] * 7 + [ctypes.c_int64(1)] + [null] * 7
    assert len(dense) == NAMES["cgmr_jcbb_dense"] and lib.cgmr_jcbb_dense(*dense) == e_invalid
    graph = [null, ctypes.c_int(1), null, null, ctypes.c_int(0), null, null, null, null]
    args = graph + [ctypes.c_int(0), null, null, null, null, ctypes.c_int(0), null, null, ctypes.c_int64(1)] + [null] * 9
    assert len(args) == NAMES["cgmr_joint_compatibility"] and lib.cgmr_joint_compatibility(*args) == e_invalid


def test_python_layers_expose_the_calls():
    for n in ("jcbb_dense", "joint_compatibility"):
        assert callable(getattr(_lib.Context, n, None)), n
        assert inspect.signature(getattr(_lib.Context, n)).parameters["node_limit"].default == _lib.JC_DEFAULT_NODE_LIMIT
    for n in ("associateObservations", "addAssociatedObservations"):
        sig = inspect.signature(getattr(GraphSLAM, n)).parameters
        assert list(sig)[1:] == ["pose_idx", "landmark_idxs", "z", "info", "kind", "gamma_by_dof", "node_limit", "robust"], n
        assert (sig["kind"].default, sig["gamma_by_dof"].default, sig["node_limit"].default, sig["robust"].default) == (1, None, None, False)


def test_gamma_table_is_the_chi2_quantile():
    from scipy.stats import chi2
    g = _lib.JC_GAMMA_99
    assert len(g) == 65 and g[0] == 0.0 and g[3] == GraphSLAM.GAMMA_99
    for k in range(1, 65):
        assert g[k] == pytest.approx(float(chi2.ppf(0.99, k)), rel=1e-12), k
    assert all(g[k] > g[k - 1] for k in range(1, 65))


# ------------------------------------------------------------------------------------------------ the reference
def test_crossed_numbers():
    """The issue's worked case: nearest neighbour pairs both measurements with the wrong landmarks, the sequential heuristic one
    of two and wrongly, JCBB both and rightly; the closest test lies 0.90 (relative) from its threshold."""
    P = JC.case("crossed")
    assert RJ.crossed_nearest_neighbour(P) == [1, 0] and not RJ.admissible(P, [1, 0])[0]
    assert P["greedy"][0] == [1, -1] and P["greedy"][1] == 1
    assert P["answer"][0] == [0, 1] and P["answer"][1] == 2 and P["answer"][3] == 4
    assert P["run"].margin == pytest.approx(0.90, abs=0.005)
    ic = RJ.individual(P)
    assert ic[0, 1] < ic[0, 0] and np.all(ic < JC.GAMMA[2])          # every pairing passes on its own


@pytest.mark.parametrize("name", JC.SMALL)
def test_enumerator_sequential_search_and_both_d2_methods_agree(name):
    P = JC.case(name)
    run = RJ.Run()
    hyps = RJ.enumerate_all(P, run)
    best = RJ.best_of(hyps, run)
    assert [-1] * P["M"] in [h[0] for h in hyps]
    assert best[1] == P["answer"][1] and best[3] == P["answer"][3]
    assert best[2] == pytest.approx(P["answer"][2], rel=1e-12, abs=0)
    if run.gap >= JC.GAP_MIN:
        assert best[0] == P["answer"][0]
    assert run.gap == pytest.approx(P["run"].gap, rel=1e-9) or (np.isinf(run.gap) and np.isinf(P["run"].gap))
    assert run.margin >= JC.MARGIN_MIN and run.dis <= JC.D2_BAR / 10
    for h, count, d2, dof in hyps:                                  # every listed hypothesis is admissible, by both d2 methods
        ok, d, f = RJ.admissible(P, h)
        assert ok and f == dof and (count == 0 or d == d2)
        e, C = RJ.joint(P, h)
        assert count == 0 or RJ.d2_solve(e, C) == pytest.approx(d2, rel=JC.D2_BAR / 10)
    # no admissible hypothesis has more pairings than the sequential search's, and the greedy one is among them
    assert max(h[1] for h in hyps) == P["answer"][1] and P["greedy"][0] in [h[0] for h in hyps]


@pytest.mark.parametrize("name", list(JC.CASES))
def test_case_reaches_its_gap_with_margin(name):
    P = JC.case(name)
    assert JC.CASES[name][2](P), JC.CASES[name][1]
    assert P["run"].margin >= JC.MARGIN_MIN, P["run"].margin
    ok, d2, dof = RJ.admissible(P, P["answer"][0])
    assert ok and dof == P["answer"][3] and (dof == 0 or d2 == P["answer"][2])
    assert RJ.admissible(P, P["greedy"][0])[0]
    assert not RJ._better((P["greedy"][1], P["greedy"][2]), (P["answer"][1], P["answer"][2]))
    assert P["M"] <= _lib.JC_MAX_OBS and P["L"] <= _lib.JC_MAX_LANDMARKS and P["answer"][3] <= 64


def test_row_has_many_maximum_count_hypotheses():
    P = JC.case("row")
    shifted = [[j + s for j in P["truth"]] for s in (-2, -1, 1, 2)]
    assert all(RJ.admissible(P, h)[0] for h in shifted)
    assert all(RJ.admissible(P, h)[1] > P["answer"][2] for h in shifted)
    assert JC.GAP_MIN <= P["run"].gap < 1.0


def test_decoy_row_traps_the_greedy_hypothesis():
    """The timing tool's worst family does what it is built for, at a size the reference can search: the greedy hypothesis
    keeps the decoy alone, the search pairs everything with the row."""
    P = JC.decoy_row(8, 24)
    run = RJ.Run()
    g, best = RJ.greedy(P, run), RJ.jcbb(P, run)
    assert g[0] == [23] + [-1] * 7 and g[1] == 1
    assert best[0] == list(range(7, 15)) and best[1] == 8 and run.margin >= JC.MARGIN_MIN


def test_graph_problem_takes_sigma_from_the_typed_reference():
    """graph_problem's Sigma -- marginal_blocks' system and refined solves for the scan's columns alone -- is marginal_blocks'
    own, block for block, and the scan of jcbb_cases.graph_scene is what the GPU test says it is."""
    import assoc_cases as AC
    import ref_assoc as A
    g = AC.case("mixed5_256")
    sc = JC.graph_scene(g)
    p = g["truth"]
    M, lms = len(sc["kinds"]), sc["lms"]
    assert M == 7 and len(lms) == 8 and len(set(lms.tolist())) == 8 and np.all(g["vk"][lms] == 1) and g["vk"][sc["pose"]] == 0
    assert sc["kinds"].tolist() == [1, 1, 1, 1, 1, 2, 1] and sc["truth"][-1] == -1 and sc["truth"][:6] == lms[:6].tolist()
    P, err = RJ.graph_problem(g, p, [sc["pose"]] * M, sc["kinds"], sc["meas"], sc["info"], lms, JC.GAMMA)
    verts = [sc["pose"]] + lms.tolist()
    diag, cross, err2 = A.marginal_blocks(p, *AC.args(g)[1:], *AC.kinds(g), pairs=[(a, b) for a in verts for b in verts])
    assert err <= AC.REF_ERR_MAX and err2 <= AC.REF_ERR_MAX
    off, dim = [0] + [3 + 2 * j for j in range(8)], [3] + [2] * 8
    for x in range(9):
        for y in range(9):
            blk = cross[9 * x + y][:dim[x], :dim[y]]
            mine = P["sigma"][off[x]:off[x] + dim[x], off[y]:off[y] + dim[y]]
            assert np.abs(mine - blk).max() <= 1e-14 * np.abs(blk).max(), (x, y)
    # at the truth every generated measurement is closest to its own landmark, and the spurious one passes nowhere
    ic = RJ.individual(P)
    assert np.array_equal(np.argmin(ic[:6], axis=1), np.arange(6)) and np.all(ic[6] > JC.GAMMA[2])
    z, J = A.predict(p, sc["pose"], int(lms[2]), 1)
    assert np.array_equal(P["J"][2, 2], J) and np.array_equal(P["e"][2, 2], z[:2] - sc["meas"][2, :2])


def test_reference_d2_disagreement():
    """Re-measures jcbb_cases.REF_D2_DISAGREEMENT_MEASURED: the two float64 d2 methods over every hypothesis the reference
    evaluates; the bar that follows stays a hundredth of the cases' margin."""
    worst = max(JC.case(n)["run"].dis for n in JC.CASES)
    for n in JC.SMALL:
        run = RJ.Run()
        RJ.enumerate_all(JC.case(n), run)
        worst = max(worst, run.dis)
    print(f"largest relative disagreement of the two d2 methods: {worst:.3g}")
    assert worst <= JC.REF_D2_DISAGREEMENT_MEASURED
    assert JC.D2_BAR == max(1e-9, 10 * JC.REF_D2_DISAGREEMENT_MEASURED) and JC.D2_BAR <= 1e-5 <= JC.MARGIN_MIN / 100
