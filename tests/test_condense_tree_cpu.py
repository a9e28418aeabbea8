"""The float64 reference of the condensed tree (tests/ref_condense_tree.py) and the cases the device is run on
(tests/condense_tree_cases.py), without a GPU: the chain's known answers, the tie rule of the total order, and on the loop
graphs the preconditions that make an exact comparison of trees fair and KL(tree) < KL(star) for the reference's own edges.

The chain.  With first-order labels every edge of the tree carries the odometry's information in closed form, asserted at
CHAIN_ATOL (absolute, on entries up to 1e3) on the 6-chain and on the 60-chain with 10 vertices requested.  An error dS of the
relative pose's covariance moves the information by I dS I: with ||I|| = 270 .. 1e3 and blocks of H^-1 of size 10 on the
60-chain, a float64 inverse of H alone leaves 1.3e-11 there (8.0e-13 and 1.4e-14 on the 6-chain), so this check takes the
reference's H^-1, the propagation and the 3x3 inverse in long double (ref_condense_tree.joint_extended): measured 1.3e-16,
1.4e-14 and 5.7e-14, the last two being what condense_tree_cases.chain_edge_information's own 3x3 inverse carries (against
the closed form in exact rational arithmetic: 1.3e-16, 1.3e-18 and 0).
With the unscented labels, which are the contract, the information differs from the closed form by
the transform's own second-order terms: measured 2.48e-4 (6-chain, gauge 0), 5.54e-5 (gauge 3) and 1.50e-2 (60-chain) of the
information's norm; condense_tree_cases.UT_GAP holds these figures and the bar is twice each."""
import numpy as np
import pytest

import condense_tree_cases as CC
import ref_condense_tree as T

from condense_tree_cases import UT_GAP, UT_MARGIN
from condense_tree_cases import info_full as _full

CHAIN_ATOL = 1e-12              # test_joint_marginals_gpu.py: the closed form of the chain


def _chain_ref(name, labels, refined=False):
    _, mk, gauge, q = next(c for c in CC.CHAINS if c[0] == name)
    g = mk()
    return T.condense_tree(g["poses"], g["edge_from"], g["edge_to"], g["meas"], g["info"], gauge, q, refined=refined, labels=labels), gauge, q


# --------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("name", [c[0] for c in CC.CHAINS])
def test_chain_tree_is_the_chain_and_first_order_labels_are_the_odometry(name):
    assert np.finfo(np.longdouble).eps < 1e-18                    # (the extended evaluation needs a long double that is one)
    ref, gauge, q = _chain_ref(name, "first", refined="extended")
    tree = ref["tree"]
    assert {int(t): int(f) for f, t in zip(tree["fr"], tree["to"])} == CC.chain_parent_vertices(gauge, q)
    assert np.array_equal(tree["to"], ref["nodes"][1:]) and not tree["flags"].any()
    worst = 0.0
    for f, t, z, iu in zip(tree["fr"], tree["to"], tree["est"], tree["iu"]):
        assert np.abs(z - [t - f, 0.0, 0.0]).max() <= CHAIN_ATOL
        worst = max(worst, np.abs(_full(iu) - CC.chain_edge_information(f, t)).max())
    print(f"{name}: first-order labels, information against the closed form {worst:.2e} absolute")
    assert worst <= CHAIN_ATOL
    # exact on a chain: the tree's Gaussian is the joint marginal, the star's is not
    kl_tree, kl_star = T.kl_of_edges(ref, tree), T.kl_of_edges(ref, ref["star"])
    print(f"{name}: KL tree {kl_tree:.2e}, star {kl_star:.3f} nats")
    assert abs(kl_tree) <= 1e-10 and kl_star > 1.0
    # the float64 evaluation picks the same tree
    ref64, _, _ = _chain_ref(name, "first")
    assert np.array_equal(ref64["parent"], ref["parent"])


@pytest.mark.parametrize("name", [c[0] for c in CC.CHAINS])
def test_chain_unscented_labels_within_twice_the_measured_gap(name):
    ref, gauge, q = _chain_ref(name, "ut")
    tree = ref["tree"]
    assert {int(t): int(f) for f, t in zip(tree["fr"], tree["to"])} == CC.chain_parent_vertices(gauge, q)
    assert not tree["flags"].any()
    gap = max(np.linalg.norm(_full(iu) - CC.chain_edge_information(f, t)) / np.linalg.norm(CC.chain_edge_information(f, t))
              for f, t, iu in zip(tree["fr"], tree["to"], tree["iu"]))
    print(f"{name}: unscented against first-order information {gap:.3e} of its norm")
    assert 0.5 * UT_GAP[name] <= gap <= UT_GAP[name] * 1.01        # (the figure written down is the figure measured)
    assert gap <= UT_MARGIN * UT_GAP[name]


# --------------------------------------------------------------------------------------- the tie rule
def _prim(W, root):
    """Prim under the same total order, written apart from the Kruskal reference: the set of tree edges."""
    n = W.shape[0]
    inside = {root}
    edges = set()
    while len(inside) < n:
        best = None
        for u in inside:
            for v in range(n):
                if v in inside:
                    continue
                w = W[max(u, v), min(u, v)]
                key = (np.inf if np.isnan(w) else w, max(u, v), min(u, v))
                if best is None or key < best:
                    best = key
        edges.add((best[1], best[2]))
        inside.add(best[1] if best[2] in inside else best[2])
    return edges


def _edge_set(parent):
    return {(max(v, int(p)), min(v, int(p))) for v, p in enumerate(parent) if p >= 0}


def test_equal_weights_give_a_star_on_node_0():
    for n in (2, 3, 7, 50):
        parent = T.kruskal(np.ones((n, n)))
        assert parent[0] == -1 and np.all(parent[1:] == 0)


@pytest.mark.parametrize("n", [2, 3, 7, 50])
def test_integer_weights_with_ties_tree_is_unique(n):
    """The keys (w, max, min) are distinct, so the tree is one set of edges: the same whichever root it is oriented from,
    whichever order the candidate edges are listed in before sorting, and whichever algorithm finds it (Prim, written apart)."""
    rng = np.random.default_rng(n)
    W = rng.integers(0, 4, (n, n)).astype(np.float64)
    W = np.tril(W, -1) + np.tril(W, -1).T
    base = T.kruskal(W)
    want = _edge_set(base)
    assert len(want) == n - 1 and want == _prim(W, 0)
    for root in range(0, n, max(1, n // 5)):
        p = T.kruskal(W, root=root, enumeration=rng.permutation(n * (n - 1) // 2))
        assert p[root] == -1 and _edge_set(p) == want
        assert _prim(W, root) == want
    # only the lower triangle is read
    assert np.array_equal(T.kruskal(np.tril(W, -1) + 99.0 * np.triu(np.ones((n, n)), 1)), base)


def test_an_infinite_row_and_a_nan_hang_on_the_root():
    rng = np.random.default_rng(5)
    n = 9
    W = rng.integers(0, 4, (n, n)).astype(np.float64)
    W = np.tril(W, -1) + np.tril(W, -1).T
    W[4, :] = W[:, 4] = np.inf
    W[7, :] = W[:, 7] = np.nan
    parent = T.kruskal(W)
    assert parent[4] == 0 and parent[7] == 0
    keep = [v for v in range(n) if v not in (4, 7)]
    sub = T.kruskal(W[np.ix_(keep, keep)])
    assert [keep[p] if p >= 0 else -1 for p in sub] == [int(parent[v]) for v in keep]


def test_decision_margin_is_the_smallest_swap():
    W = np.array([[np.inf, 1.0, 5.0, 9.0], [1.0, np.inf, 2.0, 9.0], [5.0, 2.0, np.inf, 2.5], [9.0, 9.0, 2.5, np.inf]])
    parent = T.kruskal(W)
    assert list(parent) == [-1, 0, 1, 2]
    # (2, 0): 5 - max(1, 2) = 3; (3, 0): 9 - 2.5; (3, 1): 9 - 2.5
    assert T.decision_margin(W, parent) == 3.0


# --------------------------------------------------------------------------------------- the loop cases
@pytest.mark.parametrize("name", [c[0] for c in CC.LOOPS])
def test_loop_case_preconditions_and_tree_beats_star(name):
    ref = CC.loop_reference(name)
    margin, own = T.decision_margin(ref["W"], ref["parent"]), CC.ref_own_error(ref)
    kl_tree, kl_star = T.kl_of_edges(ref, ref["tree"]), T.kl_of_edges(ref, ref["star"])
    print(f"{name}: decision margin {margin:.2e} nats, reference's own error {own:.1e}, KL tree {kl_tree:.3f} star {kl_star:.3f} nats")
    assert margin >= CC.MARGIN_MIN
    assert own <= CC.REF_ERR_MAX
    assert not ref["tree"]["flags"].any() and not ref["star"]["flags"].any()
    assert np.all(np.isfinite(ref["W"][np.tril_indices(len(ref["nodes"]), -1)]))
    assert kl_tree < kl_star


def test_a_requested_vertex_no_edge_touches_hangs_on_the_gauge_unlabelled():
    g, gauge, q, iso = CC.isolated_case()
    ref = T.condense_tree(g["poses"], g["edge_from"], g["edge_to"], g["meas"], g["info"], gauge, q, refined=True)
    base = CC.loop_reference("rw120_k8")
    tree = ref["tree"]
    k = int(np.flatnonzero(tree["to"] == iso)[0])
    assert k == 4 and tree["fr"][k] == gauge and tree["flags"][k] == 2 and np.isinf(ref["weight"][k])
    assert list(tree["iu"][k]) == [1, 0, 0, 1, 0, 1]
    rest = np.arange(len(q) - 1) != k                              # (the gauge is in q: one edge fewer than queries)
    assert np.array_equal(tree["fr"][rest], base["tree"]["fr"]) and np.array_equal(tree["to"][rest], base["tree"]["to"])
    assert not tree["flags"][rest].any() and np.allclose(tree["iu"][rest], base["tree"]["iu"], rtol=1e-9, atol=0)


def test_kl_is_zero_for_the_same_gaussian_and_grows_with_a_dropped_correlation():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6))
    S = A @ A.T + 6 * np.eye(6)
    assert abs(T.kl(S, np.linalg.inv(S))) <= 1e-12
    D = S.copy()
    D[:3, 3:] = D[3:, :3] = 0
    assert T.kl(S, np.linalg.inv(D)) > 1e-3


def test_entry_points_are_declared_and_exported():
    from cg_mrslam_amd import _lib
    declared = _lib.declared_symbols()
    lib = _lib.load_library()
    for n in ("cgmr_condense_tree", "cgmr_min_spanning_tree"):
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "cgmr.h")).read()
    assert f"#define CGMR_TREE_MAX_NODES {_lib.TREE_MAX_NODES}\n" in hdr
