"""cgmr_max_clique_exact / cgmr_closure_consistency_exact against yardsticks that are not the code under test: the bit-set
branch and bound of ref_clique.py (held to Bron-Kerbosch in test_clique_exact_cpu.py), ref_pcm.greedy_clique for what the
greedy call finds, and the dense float64 consistency reference for the end-to-end candidates.

Integer work: sizes are compared exactly, the members are checked to be a clique (ascending, distinct, pairwise adjacent) --
which of several maximum cliques comes back is the search's rule (include/cgmr.h), not the reference's --, and two calls must
give identical bytes, proven and the node count included.  Every case but the node-limit one is far inside the default limit
(the reference needs at most 7 595 nodes in all on any of them; the limit is per root) and must come back proven."""
import numpy as np
import pytest

import ref_clique as R
import ref_pcm as P
import test_pcm_gpu as T
from cg_mrslam_amd import Context
from cg_mrslam_amd._lib import EXACT_ROUNDS, PCM_MAX_CLOSURES, CgmrError
from cg_mrslam_amd.graph import GraphSLAM, PoseGraph

pytestmark = pytest.mark.gpu

E_INVALID = -1
GAMMA = P.GAMMA_99

_REF = {}


def _omega(key, A):
    """The reference's clique number of a named graph, computed once."""
    if key not in _REF:
        _REF[key] = R.omega(A)[0]
    return _REF[key]


def _exact_twice(ctx, A, **kw):
    """(clique, proven, nodes) of two calls that must agree in every byte."""
    c1, p1, n1 = ctx.max_clique_exact(A, **kw)
    c2, p2, n2 = ctx.max_clique_exact(A, **kw)
    assert c1.dtype == c2.dtype and c1.tobytes() == c2.tobytes() and p1 == p2 and n1 == n2, (c1, c2, p1, p2, n1, n2)
    return c1, p1, n1


# --------------------------------------------------------------------------------------- 1. size equals the reference
@pytest.mark.parametrize("n", [1, 2, 3, 20, 63, 64, 65, 127, 128, 130, 200])
def test_size_equals_the_reference_across_word_boundaries(ctx, n):
    rng = np.random.default_rng(n)
    for dens in (0.1, 0.5, 0.9):                                     # (drawn in this order, as the greedy test draws them)
        A = P.random_graph(n, dens, rng)
        if dens == 0.9 and n > 65:                                   # the dense large graphs: the node limit's ground
            continue
        want = _omega(("G", n, dens), A)
        clique, proven, nodes = _exact_twice(ctx, A)
        print(f"n = {n}, density {dens}: omega {want}, device {len(clique)}, proven {proven}, {nodes} nodes")
        assert proven and len(clique) == want and R.is_clique(A, clique), (n, dens, clique, want)
        assert n <= nodes


# --------------------------------------------------------------------------------------- 2. the cases the greedy misses
def _second_draw_of_200():
    rng = np.random.default_rng(200)
    for dens in (0.1, 0.5):
        A = P.random_graph(200, dens, rng)
    return A


MISSED = {
    "G(20, 0.5) 20187": (lambda: P.random_graph(20, 0.5, np.random.default_rng(20187)), 4, 5),
    "G(130, 0.5) 10011": (lambda: P.random_graph(130, 0.5, np.random.default_rng(10011)), 9, 10),
    "G(130, 0.7) 10010": (lambda: P.random_graph(130, 0.7, np.random.default_rng(10010)), 16, 17),
    "G(200, 0.5) 15402": (lambda: P.random_graph(200, 0.5, np.random.default_rng(15402)), 10, 11),
    "G(200, 0.5) 15405": (lambda: P.random_graph(200, 0.5, np.random.default_rng(15405)), 10, 11),
    "G(200, 0.5) second draw of 200": (_second_draw_of_200, 10, 11),
}


@pytest.mark.parametrize("name", list(MISSED))
def test_exact_finds_what_the_greedy_misses(ctx, name):
    make, greedy, omega = MISSED[name]
    A = make()
    # the reference first: were numpy's generator ever to draw differently, this fails instead of testing nothing
    want = _omega(name, A)
    assert P.greedy_clique(A)[1] == greedy < want == omega, name
    if len(A) <= 20:
        assert len(P.max_clique_exact(A)) == omega
    got, _ = ctx.max_clique_greedy(A)
    assert len(got) == greedy
    clique, proven, nodes = _exact_twice(ctx, A)
    print(f"{name}: greedy {len(got)}, exact {len(clique)}, {nodes} nodes")
    assert proven and len(clique) == omega and R.is_clique(A, clique), (name, clique)


# --------------------------------------------------------------------------------------- 3. trivial, tied, planted, the cap
def test_trivial_tied_and_complete_graphs(ctx):
    for n in (1, 5, 64, 65):
        clique, proven, _ = _exact_twice(ctx, np.zeros((n, n), dtype=bool))         # no edge: size 1
        assert proven and len(clique) == 1
    for n in (1, 5, 64, 65, PCM_MAX_CLOSURES):                       # complete: everything; 1024 is W = 16 and the cap
        clique, proven, _ = _exact_twice(ctx, ~np.eye(n, dtype=bool))
        assert proven and clique.tolist() == list(range(n)), n
    A = P.two_triangles()
    clique, proven, _ = _exact_twice(ctx, A)
    assert proven and len(clique) == 3 and R.is_clique(A, clique)
    clique, proven, nodes = ctx.max_clique_exact(np.zeros((0, 0), dtype=bool))
    assert len(clique) == 0


@pytest.mark.parametrize("n,p,k", [(1024, 0.05, 40), (1023, 0.1, 30)])
def test_planted_clique_at_the_cap(ctx, n, p, k):
    rng = np.random.default_rng(n)
    planted = sorted(rng.choice(n, k, replace=False).tolist())
    A = P.planted_clique(n, p, planted, rng)
    assert _omega(("planted", n), A) == k
    clique, proven, nodes = _exact_twice(ctx, A)
    assert proven and clique.tolist() == planted, (clique, planted, nodes)


def test_exact_rejects_what_the_greedy_call_rejects_and_a_bad_limit(ctx):
    A = P.random_graph(70, 0.5, np.random.default_rng(2))
    words, n = Context._adj_words(A)
    ctx.max_clique_exact(words)                                      # (the words themselves are fine)
    diag = words.copy()
    diag[66, 1] |= np.uint64(1) << np.uint64(66 - 64)
    asym = words.copy()
    asym[3, 1] ^= np.uint64(1) << np.uint64(69 - 64)                  # bit (3, 69) without (69, 3)
    pad = words.copy()
    pad[10, 1] |= np.uint64(1) << np.uint64(70 - 64)                  # column 70 of a 70-vertex graph
    big = np.zeros((PCM_MAX_CLOSURES + 1, (PCM_MAX_CLOSURES + 64) // 64), dtype=np.uint64)
    for bad, kw in ((diag, {}), (asym, {}), (pad, {}), (big, {}), (words, {"node_limit": 0}), (words, {"node_limit": -5})):
        with pytest.raises(CgmrError) as ei:
            ctx.max_clique_exact(bad, **kw)
        assert ei.value.code == E_INVALID
        assert "cgmr_max_clique_exact" in str(ei.value)


# --------------------------------------------------------------------------------------- 4. the node limit
def test_node_limit_stops_the_search_and_keeps_a_clique(ctx):
    """G(200, 0.9): the greedy clique has 41 members and the search is far beyond one node per root.  (Not run with the default
    limit: that is the benchmark's ground, not a test's.)"""
    A = P.random_graph(200, 0.9, np.random.default_rng(5))
    assert P.greedy_clique(A)[1] == 41
    got, _ = ctx.max_clique_greedy(A)
    assert len(got) == 41
    clique, proven, nodes = _exact_twice(ctx, A, node_limit=1)
    print(f"node_limit 1: {len(clique)} members, {nodes} nodes")
    assert not proven and R.is_clique(A, clique) and len(clique) >= 41
    assert 200 <= nodes <= 200 * EXACT_ROUNDS
    clique, proven, nodes = _exact_twice(ctx, A, node_limit=8)
    assert R.is_clique(A, clique) and len(clique) >= 41 and nodes <= 8 * 200 * EXACT_ROUNDS


# --------------------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("seed", [3, 4, 5])
def test_end_to_end_returns_the_inliers_and_leaves_the_plain_call_alone(ctx, seed):
    g, p = T._optimised(ctx, "pg120")
    ca, cb, z, ci, out, ref, A, (want, size, want_seed) = T._pg120_reference(ctx, seed)
    inl = sorted(set(range(len(ca))) - set(out.tolist()))
    assert want == inl and size == 26 and _omega(("pg120", seed), A) == 26
    before = ctx.closure_consistency(p, *T._a(g), ca, cb, z, ci, GAMMA)
    d2, adj, clique, proven = ctx.closure_consistency_exact(p, *T._a(g), ca, cb, z, ci, GAMMA)
    assert proven is True and clique.tolist() == inl
    assert d2.tobytes() == before[0].tobytes() and adj.tobytes() == before[1].tobytes() and np.array_equal(adj, A)
    again = ctx.closure_consistency_exact(p, *T._a(g), ca, cb, z, ci, GAMMA)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip((d2, adj, clique, proven), again))
    after = ctx.closure_consistency(p, *T._a(g), ca, cb, z, ci, GAMMA)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(before, after))
    assert before[2].tolist() == inl and before[3] == want_seed
    # a limit the call refuses, before anything is queued
    with pytest.raises(CgmrError) as ei:
        ctx.closure_consistency_exact(p, *T._a(g), ca, cb, z, ci, GAMMA, node_limit=0)
    assert ei.value.code == E_INVALID and "cgmr_closure_consistency_exact" in str(ei.value)


def test_wrappers_and_driver_use_the_exact_clique(ctx):
    g, p = T._optimised(ctx, "pg120")
    ca, cb, z, ci, out, ref, A, (want, size, want_seed) = T._pg120_reference(ctx, 3)
    gs = GraphSLAM(PoseGraph.from_synth(dict(g, poses=p.copy())), ctx)
    closures = [(int(ca[k]), int(cb[k]), z[k], ci[k]) for k in range(len(ca))]
    r = gs.closureConsistency(closures, GAMMA, exact=True)
    r0 = ctx.closure_consistency_exact(p, *T._a(g), ca, cb, z, ci, GAMMA)
    assert len(r) == 4 and all(np.array_equal(x, y) for x, y in zip(r, r0)) and r[3] is True
    assert gs.consistentClosures(closures, exact=True).tolist() == want
    assert gs.consistentClosures(closures).tolist() == want            # (the default: the greedy call, as before)
    assert gs.closureConsistency(closures, GAMMA, exact=True, node_limit=1)[2].tolist() == want     # no smaller than the greedy one
    plain = gs.closureConsistency(closures, GAMMA)
    assert plain[3] == want_seed and not isinstance(plain[3], bool)
    # the driver: the same edges as ("pcm", gamma) adds on these candidates, and the log says how they were found
    nE = len(g["edge_from"])
    slam, edges = T._driver(ctx, g, p, ca, cb, z, closure_check=("pcm-exact", GAMMA))
    T._feed(slam, edges)
    assert [e for e in slam.log if e[0].startswith("pcm")] == [("pcm-exact", 26, 40, True)]
    lc = [k for k, kind in enumerate(slam.edge_kind) if kind == "lc"]
    assert lc == list(range(nE, nE + 26))
    assert [k for k, e in enumerate(edges) if e["added"]] == want
