"""The graphs of tests/topology_cases.py on the CPU, before tests/test_topology_gpu.py trusts them on the GPU: each reaches the
shape of the elimination forest it is there for (the host analysis needs no GPU), the C oracle's steps on it are backward
stable by ref_numpy.step_backward_error, that yardstick resolves a real error on it (tests/test_reference_cpu.py's
mutations: one edge left out of the assembly, or one block of H off by 1e-9), and the oracle, ref_numpy and the host's
assembly lists mean the same thing by a self edge: the chain rule's term, which is zero."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import ref_numpy as R
import reference_cases as C
import test_reference_cpu as TR
import topology_cases as T
from reference_cases import OMEGA_MAX

CHECKED = [n for n in T.CASES if n not in ("self_edge", "free_component")]


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_reaches_its_branch(name):
    T.assert_branch(name, T.graph(name))


@pytest.mark.parametrize("name", CHECKED)
def test_oracle_steps_are_backward_stable(oracle, name):
    """The step from the initial guess and from the oracle's own 3rd iterate (measured: 0.0 u on every case)."""
    g = T.graph(name)
    a = C.args(g)
    st, p3, _, _ = oracle.gn_optimize(*a, 3)
    assert st == 0
    for p0 in (g["poses"], p3):
        st, p1, _, _ = oracle.gn_optimize(p0, *a[1:], 1)
        assert st == 0
        w = R.step_backward_error(p0, p1, *a[1:])
        assert w <= OMEGA_MAX, (name, w / R.U)
    fx = g["fixed"] != 0
    assert np.array_equal(p1[fx], g["poses"][fx])


def _solvable_without(g, k):
    """Every free vertex still reaches a fixed one when edge k is left out."""
    V = len(g["poses"])
    keep = np.ones(len(g["edge_from"]), dtype=bool)
    keep[k] = False
    A = sp.coo_matrix((np.ones(int(keep.sum())), (g["edge_from"][keep], g["edge_to"][keep])), shape=(V, V))
    _, lab = connected_components(A, directed=False)
    anchored = np.zeros(lab.max() + 1, dtype=bool)
    anchored[lab[g["fixed"] != 0]] = True
    return bool(np.all(anchored[lab]))


def mutation(g):
    """(kind, argument of test_reference_cpu._perturbed_step): the first edge with a free end point that can be left out
    without making H singular; on a tree (every edge is a bridge) one block of H scaled by 1 + 1e-9 instead -- the block of
    the first edge between two free vertices, or, where a fixed vertex cuts every edge, a diagonal block."""
    ef, et, fixed = g["edge_from"], g["edge_to"], g["fixed"]
    free_end = np.flatnonzero(((fixed[ef] == 0) | (fixed[et] == 0)) & (ef != et))
    for k in free_end[:40]:
        if _solvable_without(g, int(k)):
            return "drop_edge", int(k)
    fx = R.active_fixed(len(fixed), fixed, ef, et)
    hidx = np.cumsum(fx == 0) - 1
    both = np.flatnonzero((fx[ef] == 0) & (fx[et] == 0) & (ef != et))
    if len(both):
        k = int(both[0])
        return "scale_block", (int(hidx[ef[k]]), int(hidx[et[k]]), 1 + 1e-9)
    h = int(hidx[np.flatnonzero(fx == 0)[0]])
    return "scale_block", (h, h, 1 + 1e-9)            # (applied to the diagonal block twice: (1 + 1e-9)^2)


@pytest.mark.parametrize("name", CHECKED)
def test_omega_resolves_a_real_error(name):
    g = T.graph(name)
    a = C.args(g)
    p0, p1 = TR._perturbed_step(g)
    assert R.step_backward_error(p0, p1, *a[1:]) <= OMEGA_MAX
    kind, arg = mutation(g)
    q0, q1 = TR._perturbed_step(g, **{kind: arg})
    w = R.step_backward_error(q0, q1, *a[1:])
    print(f"{name}: {kind} {arg}: omega {w / R.U:.3g} u")
    assert w > OMEGA_MAX, (name, kind, w / R.U)


def test_mutations_cover_both_kinds():
    kinds = {name: mutation(T.graph(name))[0] for name in CHECKED}
    assert kinds["clique60"] == "drop_edge" and kinds["bintree"] == "scale_block" and kinds["star3000"] == "scale_block"


def test_self_edge_is_the_chain_rule_term(oracle):
    """The oracle and ref_numpy agree on the self edge at OMEGA_MAX, and both mean the chain rule's term by it: the system
    is that of the chain without the edge, chi2 is larger by the edge's constant."""
    g = T.graph("self_edge")
    a = C.args(g)
    assert g["edge_from"][-1] == g["edge_to"][-1] == 7
    st, p3, _, _ = oracle.gn_optimize(*a, 3)
    assert st == 0
    for p0 in (g["poses"], p3):
        st, p1, _, _ = oracle.gn_optimize(p0, *a[1:], 1)
        assert st == 0
        w = R.step_backward_error(p0, p1, *a[1:])
        assert w <= OMEGA_MAX, w / R.U
    chain = tuple(x[:-1] for x in a[2:])
    H, b, _ = R.build_system(g["poses"], g["fixed"], *a[2:])
    H0, b0, _ = R.build_system(g["poses"], g["fixed"], *chain)
    assert abs(H - H0).max() == 0 and np.array_equal(b, b0)
    st, p5, chi, _ = oracle.gn_optimize(*a, 5)
    st0, q5, chi0, _ = oracle.gn_optimize(g["poses"], g["fixed"], *chain, 5)
    assert st == 0 and st0 == 0 and np.array_equal(p5, q5)
    e = R.edge_errors(g["poses"], g["edge_from"][-1:], g["edge_to"][-1:], g["meas"][-1:])[0]
    const = float(e @ R.info_full(g["info"][-1:])[0] @ e)
    assert const > 100                                           # (a non-identity measurement: the edge shows in chi2)
    np.testing.assert_allclose(chi - chi0, const, rtol=1e-12)
    np.testing.assert_allclose(R.chi2(p5, *a[2:]), chi[-1], rtol=1e-12)
    # the mutation the yardstick must catch here: the self edge summed as one diagonal contribution, Ji^T Omega Ji
    Ji = R.jacobians(g["poses"], np.array([7]), np.array([8]), g["meas"][-1:])[0][0]
    Ji[:, 2] = [0, 0, -1]                                        # (linearizeOplus at xj = xi: no lever arm)
    Hw = sp.lil_matrix(H)
    Hw[18:21, 18:21] = Hw[18:21, 18:21].toarray() + Ji.T @ R.info_full(g["info"][-1:])[0] @ Ji      # vertex 7 is free vertex 6
    dx = np.linalg.solve(Hw.toarray(), b).reshape(-1, 3)
    pw = g["poses"].copy()
    pw[1:, :2] += dx[:, :2]
    pw[1:, 2] = R.normalize_theta(pw[1:, 2] + dx[:, 2])
    assert R.step_backward_error(g["poses"], pw, *a[1:]) > OMEGA_MAX


def test_self_edge_is_in_no_assembly_list():
    """The host's assembly lists (per block of H the edge terms that add up to it): the self edge is in none of them, every
    other edge in its two or three."""
    from cg_mrslam_amd import load_library
    from test_gn_gpu import _asm_lists
    g = T.graph("self_edge")
    E = len(g["edge_from"])
    ptr, src = _asm_lists(load_library(), None, len(g["poses"]), g["edge_from"], g["edge_to"])
    assert len(src) == 3 * (E - 1) and not np.any(src >> 2 == E - 1)
    assert np.array_equal(np.bincount(src >> 2, minlength=E)[:-1], np.full(E - 1, 3))
