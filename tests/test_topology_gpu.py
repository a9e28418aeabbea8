"""The solve paths on graphs outside the synthetic families (tests/topology_cases.py: cliques, forests, stars, trees,
fixed-fixed edges, one-pose systems, a self edge, a component without a fixed vertex), against the yardsticks the rest of the
suite already trusts -- ref_numpy.step_backward_error, the C oracle, the dense inverse and refined columns of H^-1, ref_lm,
ref_dogleg, condense_ref -- at their existing bars.  tests/test_topology_cpu.py proves on the CPU that every case reaches
its branch and that the yardsticks resolve a real error on it.  Everything runs in the default launch configuration (and on
a context that merges only the certainly resident levels)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import ref_dogleg
import ref_lm
import ref_numpy as R
import reference_cases as C
import test_dogleg_gpu as DL
import test_lm_gpu as LM
import topology_cases as T
from reference_cases import EST_ATOL, INFO_RTOL, OMEGA_MAX
from test_gn_gpu import ANG_ATOL, CHI_RTOL, POS_ATOL, _asm_lists, _check, _work_records
from test_marginals_all_gpu import _check_against_reference
from test_reference_gpu import MARG_TAU, _check_marginals, _condense_case, _top_vertices
from test_reference_gpu import ctx_resident_only  # noqa: F401  (a fixture)
from cg_mrslam_amd import synth

pytestmark = pytest.mark.gpu

GN_ITERS = 5
DENSE_UP_TO = 300      # every vertex and every edge against the dense inverse up to this many vertices
_OPT = {}


def _optimised(ctx, name):
    """(poses, chi2) of gn_optimize(GN_ITERS) on the session's context, once per case."""
    if name not in _OPT:
        rc, p, chi = ctx.gn_optimize(*C.args(T.graph(name)), GN_ITERS)
        assert rc == 0
        _OPT[name] = (p, chi)
    return _OPT[name]


def _dead(g):
    return R.active_fixed(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"]) != 0


# ------------------------------------------------------------------------------------------------ A. Gauss-Newton step
@pytest.mark.parametrize("name", T.SOLVED)
def test_gn_step_backward_error(ctx, ctx_resident_only, name):
    """The step from the initial guess and from the GPU's own 3rd iterate, on both contexts; fixed vertices keep their bits."""
    g = T.graph(name)
    s = T.assert_branch(name, g)
    a = C.args(g)
    dead = _dead(g)
    worst = 0.0
    for c in (ctx, ctx_resident_only):
        rc, p3, _ = c.gn_optimize(*a, 3)
        assert rc == 0 and np.array_equal(p3[dead], g["poses"][dead])
        for start, p0 in ((0, g["poses"]), (3, p3)):
            rc, p1, _ = c.gn_optimize(p0, *a[1:], 1)
            assert rc == 0
            w = R.step_backward_error(p0, p1, *a[1:])
            worst = max(worst, w)
            assert w <= OMEGA_MAX, (name, start, w / R.U)
            assert np.array_equal(p1[dead], p0[dead])
    print(f"{name}: largest omega {worst / R.U:.1f} u; " + " ".join(f"{k} {s[k]}" for k in (
        "fronts", "levels", "launch_levels", "max_border", "max_children", "top_block_cols", "roots", "zero_borders")))


# ------------------------------------------------------------------------------------------------- B. Gauss-Newton run
@pytest.mark.parametrize("name", T.SOLVED)
def test_gn_run_matches_the_oracle_and_repeats(ctx, oracle, name):
    g = T.graph(name)
    a = C.args(g)
    p, chi = _optimised(ctx, name)
    st, p2, chi2, _ = oracle.gn_optimize(*a, GN_ITERS)
    assert st == 0
    if name in T.ZERO_RESIDUAL:
        # a tree from one fixed vertex: the optimum's chi2 is rounded residuals only -- against the rounding floor, not relatively
        floor = LM.rounding_floor(g)
        assert np.all(np.abs(chi - chi2) <= CHI_RTOL * chi2 + floor), (chi, chi2)
        assert chi[-1] <= floor and chi2[-1] <= floor, (chi[-1], chi2[-1], floor)
        assert np.abs(p[:, :2] - p2[:, :2]).max() <= POS_ATOL
        assert np.abs(synth.normalize_theta(p[:, 2] - p2[:, 2])).max() <= ANG_ATOL
    else:
        _check(p, chi, p2, chi2)
    rc, p_again, chi_again = ctx.gn_optimize(*a, GN_ITERS)
    assert rc == 0 and np.array_equal(p, p_again) and np.array_equal(chi, chi_again)


# ---------------------------------------------------------------------------------------------------------- C. marginals
def _inverse_blocks(g, p):
    """blk(i, j): the block of H^-1 (H at p) of two free vertices, from np.linalg.inv of the dense H -- or, where fixed vertices
    cut every edge (H is block diagonal), of its 3x3 blocks."""
    a = C.args(g)
    dead = _dead(g)
    H, _, hidx = R.build_system(p, dead.astype(np.uint8), *a[2:])
    ef, et = g["edge_from"], g["edge_to"]
    if not np.any(~dead[ef] & ~dead[et] & (ef != et)):
        B = sp.bsr_matrix(H, blocksize=(3, 3))
        B.sort_indices()
        assert np.array_equal(B.indices, np.arange(H.shape[0] // 3)) and len(B.data) == H.shape[0] // 3
        inv = np.linalg.inv(B.data)
        return hidx, lambda i, j: inv[hidx[i]] if i == j else np.zeros((3, 3))
    assert len(p) <= DENSE_UP_TO
    Hinv = np.linalg.inv(H.toarray())
    return hidx, lambda i, j: Hinv[3 * hidx[i]:3 * hidx[i] + 3, 3 * hidx[j]:3 * hidx[j] + 3]


def _spd(cov, live):
    assert np.all(np.isfinite(cov))
    assert np.array_equal(cov[live], np.transpose(cov[live], (0, 2, 1)))
    assert np.linalg.eigvalsh(cov[live]).min() > 0


# (every case of up to DENSE_UP_TO vertices, and the star with the fixed centre, whose H is block diagonal)
DENSE_CASES = ["clique60", "clique150_rev", "barbell", "two_components", "bipartite", "fixed_fixed_edge", "all_neighbours_fixed",
               "self_edge", "star3000"]


@pytest.mark.parametrize("name", DENSE_CASES)
def test_marginals_against_the_dense_inverse(ctx, name):
    """Every vertex and every edge: marginals_all and the query path against np.linalg.inv of H (check 3 of
    tests/test_marginals_all_gpu.py); fixed vertices and edges that touch one give exact zeros; every free block is SPD."""
    g = T.graph(name)
    a = C.args(g)
    p, _ = _optimised(ctx, name)
    V = len(p)
    ef, et = g["edge_from"], g["edge_to"]
    hidx, blk = _inverse_blocks(g, p)
    cov, cross = ctx.marginals_all(p, g["fixed"], *a[2:], cross=True)
    query = np.arange(V, dtype=np.int32) if V <= DENSE_UP_TO else np.linspace(0, V - 1, 300).astype(np.int32)
    q = ctx.marginals(p, g["fixed"], *a[2:], query)
    worst = 0.0
    for v in range(V):
        if hidx[v] < 0:
            assert np.all(cov[v] == 0), v
            continue
        worst = max(worst, np.linalg.norm(cov[v] - blk(v, v)) / np.linalg.norm(blk(v, v)))
    for k, v in enumerate(query):
        if hidx[v] < 0:
            assert np.all(q[k] == 0), v
            continue
        worst = max(worst, np.linalg.norm(q[k] - blk(v, v)) / np.linalg.norm(blk(v, v)))
    for k in range(len(ef)):
        if hidx[ef[k]] < 0 or hidx[et[k]] < 0:
            assert np.all(cross[k] == 0), k                       # (a fixed-fixed edge among them)
            continue
        scale = np.sqrt(np.linalg.norm(blk(ef[k], ef[k])) * np.linalg.norm(blk(et[k], et[k])))
        worst = max(worst, np.linalg.norm(cross[k] - blk(ef[k], et[k])) / scale)
    print(f"{name}: largest error against the dense inverse {worst:.2e}")
    assert worst <= MARG_TAU
    _spd(cov, hidx >= 0)


def _sample(g, n_spread=60):
    """The top-block vertices, the highest-degree vertices, the fixed vertices and their neighbours, one vertex of every
    component, a spread of the rest."""
    V = len(g["poses"])
    ef, et = g["edge_from"], g["edge_to"]
    deg = np.bincount(np.r_[ef, et], minlength=V)
    fixed = np.flatnonzero(g["fixed"])
    near = np.unique(np.r_[et[np.isin(ef, fixed)], ef[np.isin(et, fixed)]])[:20]
    lab = T.components(g)
    one_each = [int(np.flatnonzero(lab == c)[0]) for c in np.unique(lab[lab >= 0])]
    pick = np.r_[fixed, _top_vertices(g, 12), np.argsort(-deg, kind="stable")[:12], near, one_each,
                 np.linspace(0, V - 1, n_spread).astype(int)]
    return np.unique(pick).astype(np.int32)


@pytest.mark.parametrize("name", ["three_components_mixed", "star3000_free_centre", "bintree"])
def test_marginals_against_refined_columns(ctx, name):
    """The larger cases: marginals_all (diagonal blocks, and the blocks of the edges into the sampled vertices) and the query
    path against refined columns of H^-1 at MARG_TAU, the reference's own error estimate gated at REF_ERR_MAX."""
    g = T.graph(name)
    p, _ = _optimised(ctx, name)
    verts = np.arange(len(p), dtype=np.int32) if len(p) <= 600 else _sample(g)
    wd, wc, nc, cov, _ = _check_against_reference(ctx, g, p, verts)
    wq = _check_marginals(ctx, g, p, verts)
    assert nc >= 50
    _spd(cov, ~_dead(g))
    print(f"{name}: {len(verts)} vertices, {nc} edge blocks; largest error diagonal {wd:.2e}, cross {wc:.2e}, query path {wq:.2e}")


@pytest.mark.parametrize("name", ["two_components", "three_components_mixed"])
def test_marginals_of_a_component_do_not_depend_on_the_others(ctx, name):
    """Forests: no edge joins two components (so no block across them is ever asked for), and the blocks of a component are
    those of the component solved alone, at MARG_TAU."""
    g = T.graph(name)
    a = C.args(g)
    p, _ = _optimised(ctx, name)
    V = len(p)
    ef, et = g["edge_from"], g["edge_to"]
    lab = connected_components(sp.coo_matrix((np.ones(len(ef)), (ef, et)), shape=(V, V)), directed=False)[1]
    assert np.array_equal(lab[ef], lab[et]) and lab.max() + 1 == (2 if name == "two_components" else 3)
    cov, cross = ctx.marginals_all(p, g["fixed"], *a[2:], cross=True)
    nd = np.linalg.norm(cov, axis=(1, 2))
    worst = 0.0
    for c in range(lab.max() + 1):
        vs = np.flatnonzero(lab == c)
        new = -np.ones(V, dtype=np.int64)
        new[vs] = np.arange(len(vs))
        ks = np.flatnonzero(lab[ef] == c)
        cov1, cross1 = ctx.marginals_all(p[vs], g["fixed"][vs], new[ef[ks]].astype(np.int32), new[et[ks]].astype(np.int32),
                                         g["meas"][ks], g["info"][ks], cross=True)
        live = g["fixed"][vs] == 0
        assert np.all(cov1[~live] == 0) and np.all(cov[vs][~live] == 0)
        worst = max(worst, (np.linalg.norm(cov1[live] - cov[vs][live], axis=(1, 2)) / nd[vs][live]).max())
        scale = np.sqrt(nd[ef[ks]] * nd[et[ks]])
        ok = scale > 0
        assert np.all(cross1[~ok] == 0) and np.all(cross[ks][~ok] == 0)
        worst = max(worst, (np.linalg.norm(cross1[ok] - cross[ks][ok], axis=(1, 2)) / scale[ok]).max())
    print(f"{name}: largest difference to a component solved alone {worst:.2e}")
    assert worst <= MARG_TAU


# --------------------------------------------------------------------------------- D. Levenberg-Marquardt and dogleg
TRACE_CASES = ["clique150_rev", "three_components_mixed", "star3000_free_centre"]


@pytest.mark.parametrize("name", TRACE_CASES)
def test_levenberg_trace_matches_reference(ctx, name):
    g = T.graph(name)
    a = C.args(g)
    ref = ref_lm.lm_optimize(*a, LM.ITERS)
    rc, poses, chi, lam, tri, done = ctx.lm_optimize(*a, LM.ITERS)
    assert rc == 0
    k = LM.check_trace(name, ref, chi, lam, tri, done, LM.rounding_floor(g))
    assert k >= 1, (name, "nothing compared")
    assert np.array_equal(poses[_dead(g)], g["poses"][_dead(g)])


@pytest.mark.parametrize("name", TRACE_CASES)
def test_dogleg_trace_matches_reference(ctx, name):
    g = T.graph(name)
    a = C.args(g)
    ref = ref_dogleg.dl_optimize(*a, DL.ITERS)
    rc, poses, chi, dlt, tri, stp, done = ctx.dl_optimize(*a, DL.ITERS)
    assert rc == 0
    k = DL.check_trace(name, ref, chi, dlt, tri, stp, done, LM.rounding_floor(g))
    assert k >= 1, (name, "nothing compared")
    assert np.array_equal(poses[_dead(g)], g["poses"][_dead(g)])


# ------------------------------------------------------------------------ E. condensed graph and covariance estimate
@pytest.mark.parametrize("name,n_query", [("clique60", 12), ("star3000_free_centre", 20)])
def test_condense_and_covariance_estimate(ctx, oracle, name, n_query):
    """Gauge 0 (the star's centre: with it fixed, every leaf is a system of its own), queries inside its component."""
    g = T.graph(name)
    a = C.args(g)
    p, _ = _optimised(ctx, name)
    V, gauge = len(p), 0
    query = np.unique(np.r_[np.linspace(1, V - 1, n_query).astype(np.int32), gauge]).astype(np.int32)
    assert len(query) == n_query + 1
    ref = _condense_case(oracle, g, gauge, query, p)
    cov = ctx.covariance_estimate(p, *a[2:], gauge, query)
    for k, v in enumerate(query):
        if v == gauge:
            assert np.all(cov[k] == 0)
            continue
        j = int(np.flatnonzero(ref["to"] == v)[0])
        assert np.linalg.norm(cov[k] - ref["cov"][j]) <= MARG_TAU * np.linalg.norm(ref["cov"][j]), int(v)
    to, est, iu, cov2 = ctx.condense(p, *a[2:], gauge, query)
    assert np.array_equal(to, ref["to"]) and not ref["not_pd"].any()
    np.testing.assert_allclose(est, ref["est"], rtol=0, atol=EST_ATOL)
    for k in range(len(to)):
        assert np.linalg.norm(cov2[k] - ref["cov"][k]) <= MARG_TAU * np.linalg.norm(ref["cov"][k])
        assert np.linalg.norm(iu[k] - ref["iu"][k]) <= INFO_RTOL * np.linalg.norm(ref["iu"][k]), int(to[k])
    d = C.check_labels_on_own_step(ctx, *a[2:], gauge, ref, to, est, iu)
    print(f"{name}: est against the own step's labels {d:.1e}")


# ----------------------------------------------------------------------------- F. a singular system beside a healthy one
def test_free_component_fails_whole_and_leaves_nothing_behind(ctx):
    """tests/test_gn_gpu.py::test_cholesky_failure_leaves_poses's contract on a component without a fixed vertex beside a
    healthy one: either the solve goes through and chi2 does not rise, or it is abandoned as a whole (g2o's early return) with
    every pose as it came, the healthy component's included.  A solve of clique60 on the same context gives the bits it gave
    before the failing call: nothing of it stays behind in the context or in the analysis cache."""
    gc = T.graph("clique60")
    ac = C.args(gc)
    before = ctx.gn_optimize(*ac, GN_ITERS)
    cov_before = ctx.marginals_all(before[1], *ac[1:])
    g = T.graph("free_component")
    T.assert_branch("free_component", g)
    rc, p, chi = ctx.gn_optimize(*C.args(g), 3, raise_on_cholesky=False)
    print(f"free_component: rc {rc}, chi2 {chi}")
    if rc == 0:
        assert chi[-1] <= chi[0] * (1 + 1e-9)
    else:
        assert rc <= -100
        np.testing.assert_array_equal(p, g["poses"])
    after = ctx.gn_optimize(*ac, GN_ITERS)
    assert before[0] == after[0] == 0
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    assert np.array_equal(cov_before, ctx.marginals_all(after[1], *ac[1:]))


# --------------------------------------------------------------------------------------------- G. device-built structure
def _maps(lib, ctx_h, nV, ef, et):
    cap = 40 * (nV + len(ef)) + 1024
    out = np.zeros(cap, dtype=np.int32)
    ef = np.ascontiguousarray(ef, dtype=np.int32)
    et = np.ascontiguousarray(et, dtype=np.int32)
    lib.cgmr_debug_maps.restype = ctypes.c_int
    n = lib.cgmr_debug_maps(ctx_h, ctypes.c_int(nV), ctypes.c_int(len(ef)), ctypes.c_void_p(ef.ctypes.data),
                            ctypes.c_void_p(et.ctypes.data), ctypes.c_int(cap), ctypes.c_void_p(out.ctypes.data))
    assert 0 < n <= cap
    return out[:n].copy()


@pytest.mark.parametrize("name", ["three_components_mixed", "star3000_free_centre", "clique150_rev", "self_edge"])
def test_structure_built_on_the_device_equals_the_hosts(ctx, name):
    """The assembly lists (k_asm_*) and the row maps, block destinations and work records (k_build_maps) of the device against
    the host's, entry for entry: lists of thousands of entries (the star's centre), reversed and shuffled edges, several
    roots, a self edge (in no list)."""
    from cg_mrslam_amd import load_library
    lib = load_library()
    g = T.graph(name)
    nV = len(g["poses"])
    ctx.set_symbolic_cache(False)
    try:
        rc, _, _ = ctx.gn_optimize(*C.args(g), 1)
    finally:
        ctx.set_symbolic_cache(True)
    assert rc == 0
    ptr_d, src_d = _asm_lists(lib, ctx.h, nV, g["edge_from"], g["edge_to"])
    ptr_h, src_h = _asm_lists(lib, None, nV, g["edge_from"], g["edge_to"])
    assert len(src_h) > 0 and np.array_equal(ptr_d, ptr_h) and np.array_equal(src_d, src_h)
    if name == "star3000_free_centre":
        assert np.diff(ptr_h).max() == 3000                       # the centre's diagonal block: the workgroup's sort
    if name == "self_edge":
        assert not np.any(src_d >> 2 == len(g["edge_from"]) - 1)
    assert np.array_equal(_maps(lib, ctx.h, nV, g["edge_from"], g["edge_to"]), _maps(lib, None, nV, g["edge_from"], g["edge_to"]))
    w_d, w_h = _work_records(lib, ctx.h)
    assert np.array_equal(w_d, w_h)
