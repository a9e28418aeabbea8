"""cgmr_closure_consistency / cgmr_max_clique_greedy against yardsticks that are not the code under test: the numpy reference
of ref_pcm.py -- the greedy clique written out from its definition, an exact maximum-clique search, the pairwise Mahalanobis
distance on the dense inverse of H -- and, for the arithmetic alone, the same numpy formula fed the device's own joint
covariance.

The bars.  The d2 arithmetic: the one test_relative_covariance_arithmetic holds d2 to (test_joint_marginals_gpu.py), the terms'
size generalised to the sum over the 16 blocks of ||J_i|| ||J_j|| ||Sigma_ij||.  End to end, adjacency, clique and seed equal
the reference's exactly, on candidate sets whose reference d2 stays 1 % clear of gamma; d2 itself is held to four times what
cgmr_relative_covariance's d2 reaches in the same run on the same candidates taken singly, against the same dense inverse
(a pair has four poses and two measurement terms where a single hypothesis has two and one).

The end-to-end candidates (generators 3, 4, 5; 26 inliers, 14 outliers), on the float64 reference: the clique is the 26
inliers from seed 1, 0, 1; smallest d2 of a pair with an outlier 109.9, 60.0, 41.5; largest d2 among the inliers 8.5, 5.4, 4.9;
nearest d2 to gamma 25 %, 52 %, 57 % away.

Measured on an MI355X: d2 arithmetic, largest error 1.0e-5 of its bar; end to end, pairwise d2 against the
dense reference 1.54e-13 / 1.69e-13 / 2.34e-13 of max(d2, 1) for generators 3 / 4 / 5, where relative_covariance's d2 of the
same candidates taken singly reaches 5.98e-14 / 1.40e-13 / 1.50e-13 (bars 2.39e-13 / 5.60e-13 / 5.99e-13); Cauchy against the
scaled information 2.6e-12 (the unweighted call differs by 0.66)."""
import copy

import numpy as np
import pytest

import ref_joint_marginals as J
import ref_pcm as P
import ref_robust as RR
import reference_cases as C
from cg_mrslam_amd import Context, synth
from cg_mrslam_amd._lib import PCM_MAX_CLOSURES, CgmrError
from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
from cg_mrslam_amd.slam import GraphSLAMDriver, LoopClosureChecker

pytestmark = pytest.mark.gpu

AGREE_TAU = 1e-9                # two paths on the same factor (test_joint_marginals_gpu.py)
GN_ITERS = 5
E_INVALID = -1
GAMMA = P.GAMMA_99
IU = np.array([500.0, 0, 0, 500.0, 0, 5000.0])

_CACHE = {}


def _optimised(ctx, name):
    """(graph, optimised poses) of a named case, computed once and shared (never modified)."""
    if name not in _CACHE:
        g = synth.make_pose_graph(120, 300, seed=48) if name == "pg120" else C.CASES[name][0]()
        rc, p, _ = ctx.gn_optimize(*C.args(g), GN_ITERS)
        assert rc == 0
        p.setflags(write=False)
        _CACHE[name] = (g, p)
    return _CACHE[name]


def _a(g):
    return g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"]


# --------------------------------------------------------------------------------------- 1. the clique kernels alone
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 127, 128, 130, 200])
def test_clique_equals_the_reference_across_word_boundaries(ctx, n):
    rng = np.random.default_rng(n)
    for dens in (0.1, 0.5, 0.9):
        A = P.random_graph(n, dens, rng)
        want, size, seed = P.greedy_clique(A)
        got, s = ctx.max_clique_greedy(A)
        assert got.tolist() == want and len(got) == size and s == seed, (n, dens, got, want, s, seed)


def test_clique_on_trivial_tied_and_planted_graphs(ctx):
    for n in (1, 5, 64, 65):
        got, s = ctx.max_clique_greedy(np.zeros((n, n), dtype=bool))            # no edge: size 1 from seed 0
        assert got.tolist() == [0] and s == 0
        got, s = ctx.max_clique_greedy(~np.eye(n, dtype=bool))                  # complete
        assert got.tolist() == list(range(n)) and s == 0
    got, s = ctx.max_clique_greedy(P.two_triangles())
    assert got.tolist() == [0, 2, 4] and s == 0
    planted = [1, 4, 6, 9, 12, 13, 17, 19]
    A = P.planted_clique(20, 0.2, planted, np.random.default_rng(0))
    assert P.max_clique_exact(A) == planted
    got, s = ctx.max_clique_greedy(A)
    assert got.tolist() == planted and s == planted[0]
    got, s = ctx.max_clique_greedy(np.zeros((0, 0), dtype=bool))
    assert len(got) == 0


def test_clique_rejects_diagonal_asymmetric_and_padding_bits(ctx):
    A = P.random_graph(70, 0.5, np.random.default_rng(2))
    words, n = Context._adj_words(A)
    ctx.max_clique_greedy(words)                                     # (the words themselves are fine)
    diag = words.copy()
    diag[66, 1] |= np.uint64(1) << np.uint64(66 - 64)
    asym = words.copy()
    asym[3, 1] ^= np.uint64(1) << np.uint64(69 - 64)                  # bit (3, 69) without (69, 3)
    pad = words.copy()
    pad[10, 1] |= np.uint64(1) << np.uint64(70 - 64)                  # column 70 of a 70-vertex graph
    big = np.zeros((PCM_MAX_CLOSURES + 1, (PCM_MAX_CLOSURES + 64) // 64), dtype=np.uint64)
    for bad in (diag, asym, pad, big):
        with pytest.raises(CgmrError) as ei:
            ctx.max_clique_greedy(bad)
        assert ei.value.code == E_INVALID


# --------------------------------------------------------------------------------------- 2. the d2 arithmetic
def _pg500_closures(g, p):
    """30 candidates on pg500: random ends; 1 shares a with 0; 3 starts where 2 ends; 4 starts at the fixed vertex; 6 repeats 5;
    correlated x / y information on every other one."""
    rng = np.random.default_rng(7)
    V, N = len(p), 30
    ca = rng.integers(0, V, N).astype(np.int32)
    cb = ((ca + rng.integers(1, V, N)) % V).astype(np.int32)
    ca[1] = ca[0]
    ca[3] = cb[2]
    ca[4] = int(np.flatnonzero(g["fixed"])[0])
    ca[6], cb[6] = ca[5], cb[5]
    z = J.relative_pose(p[ca], p[cb]) + rng.normal(0, 1, (N, 3)) * [0.05, 0.05, 0.02]
    z[6] = z[5]
    z[8] += [1.5, -2.0, 0.7]                                         # (and two that are far off)
    z[20] += [-3.0, 0.5, -2.0]
    ci = np.tile(IU, (N, 1))
    ci[::2, 1] = 100.0
    ci[6] = ci[5]
    return ca, cb, z, ci


def test_d2_arithmetic_on_the_device_own_joint_covariance(ctx):
    """The device's propagation against ref_pcm.pair_terms fed the blocks ctx.marginals_joint returns for the unique endpoints.
    Bar per pair, as test_relative_covariance_arithmetic's: 1e-12 of the terms' size -- the sum over the 16 block terms of
    ||J_i|| ||J_j|| ||Sigma_ij|| -- times ||S^-1 eps||^2, plus cond(S) d2 at the same 1e-12."""
    g, p = _optimised(ctx, "pg500")
    ca, cb, z, ci = _pg500_closures(g, p)
    N = len(ca)
    d2, adj, clique, seed = ctx.closure_consistency(p, *_a(g), ca, cb, z, ci, GAMMA)
    assert d2.shape == (N, N) and np.array_equal(d2, d2.T) and np.all(np.diag(d2) == 0)
    assert np.all(np.isfinite(d2)) and np.all(d2 >= 0)
    uq, pa, pb = P.unique_endpoints(ca, cb)
    Sq = ctx.marginals_joint(p, *_a(g), uq)
    worst = 0.0
    for k in range(N):
        for l in range(k):
            S12 = P.gather12(Sq, (pa[k], pb[k], pa[l], pb[l]))
            eps, S, scale = P.pair_terms(S12, p[ca[k]], p[cb[k]], p[ca[l]], p[cb[l]], z[k], z[l], ci[k], ci[l])
            S = 0.5 * (S + S.T)
            if (k, l) == (6, 5):
                # the repeated candidate closes an empty loop: eps is exactly 0, and what either side computes is its own
                # rounding of four compositions (the reference's eps here is ~1e-14 as well), which the bar below -- relative
                # to the reference's d2 -- does not describe.  Held instead to an eps within 1e-12 max(1, |p|) of zero, the bar
                # test_relative_covariance_arithmetic holds z to: d2 <= |d eps|^2 ||S^-1||.
                assert d2[k, l] <= (1e-12 * max(1.0, np.abs(p).max())) ** 2 * np.linalg.norm(np.linalg.inv(S), 2), (d2[k, l], eps)
                continue
            ref = float(eps @ np.linalg.solve(S, eps))
            bar =1e-12 * (scale * np.linalg.norm(np.linalg.solve(S, eps)) ** 2 + np.linalg.cond(S) * ref)
            worst = max(worst, abs(d2[k, l] - ref) / bar if bar > 0 else 0.0)
            assert abs(d2[k, l] - ref) <= bar, (k, l, d2[k, l], ref, bar)
    print(f"d2 arithmetic: largest error / bar {worst:.2e}; d2 from {d2[d2 > 0].min():.2e} to {d2.max():.2e}")
    rows = np.delete(np.arange(N), [5, 6])
    assert np.array_equal(d2[5, rows], d2[6, rows])
    # the adjacency and the clique are the reference's on the device's own d2
    A = P.adjacency(d2, GAMMA)
    assert np.array_equal(adj, A) and not adj[8].any() and not adj[20].any()
    want, size, s = P.greedy_clique(A)
    assert clique.tolist() == want and seed == s and size >= 20
    # an indefinite information: NaN in that candidate's row and column, no adjacency, the rest untouched
    bad = ci.copy()
    bad[9] = [-1e-6, 0, 0, 1.0, 0, 1.0]
    d2n, adjn, cln, _ = ctx.closure_consistency(p, *_a(g), ca, cb, z, bad, GAMMA)
    others = np.delete(np.arange(N), 9)
    assert np.all(np.isnan(d2n[9, others])) and np.all(np.isnan(d2n[others, 9])) and d2n[9, 9] == 0
    assert not adjn[9].any() and not adjn[:, 9].any() and 9 not in cln.tolist()
    assert np.array_equal(d2n[np.ix_(others, others)], d2[np.ix_(others, others)])


# --------------------------------------------------------------------------------------- 3. end to end
def _pg120_candidates(p, seed, N=40, n_out=14):
    """N candidates between random distinct vertices: the relative pose at the estimate plus noise of the information IU; n_out
    of them, picked by a permutation, moved per coordinate by +-([1, 1, 0.3] + U(0, 1) [4, 4, 1.5])."""
    rng = np.random.default_rng(seed)
    V = len(p)
    ca = rng.integers(0, V, N).astype(np.int32)
    cb = ((ca + rng.integers(1, V, N)) % V).astype(np.int32)
    z = J.relative_pose(p[ca], p[cb]) + rng.normal(0, 1, (N, 3)) / np.sqrt(IU[[0, 3, 5]])
    out = np.sort(rng.permutation(N)[:n_out])
    sign = rng.choice([-1.0, 1.0], (n_out, 3))
    z[out] += sign * (np.array([1, 1, 0.3]) + rng.random((n_out, 3)) * np.array([4, 4, 1.5]))
    return ca, cb, z, out


def _pg120_reference(ctx, seed):
    """The candidates of a generator and the reference's answers on them, computed once and shared."""
    key = ("pg120", seed)
    if key not in _CACHE:
        g, p = _optimised(ctx, "pg120")
        ca, cb, z, out = _pg120_candidates(p, seed)
        ci = np.tile(IU, (len(ca), 1))
        d2 = P.consistency_dense(p, *_a(g), ca, cb, z, ci)
        A = P.adjacency(d2, GAMMA)
        _CACHE[key] = (ca, cb, z, ci, out, d2, A, P.greedy_clique(A))
    return _CACHE[key]


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_end_to_end_against_the_dense_reference(ctx, seed):
    g, p = _optimised(ctx, "pg120")
    ca, cb, z, ci, out, ref, A, (want, size, want_seed) = _pg120_reference(ctx, seed)
    N = len(ca)
    inl = sorted(set(range(N)) - set(out.tolist()))
    # what the reference must show before the device is looked at
    is_out = np.zeros(N, dtype=bool)
    is_out[out] = True
    off = ~np.eye(N, dtype=bool)
    with_out = (is_out[:, None] | is_out[None, :]) & off
    assert want == inl and size == 26
    assert not A[with_out].any()
    assert np.min(np.abs(ref[off] - GAMMA)) > 0.01 * GAMMA
    print(f"generator {seed}: smallest d2 with an outlier {ref[with_out].min():.1f}, largest among the inliers "
          f"{ref[~with_out & off].max():.1f}, nearest to gamma {np.min(np.abs(ref[off] - GAMMA)) / GAMMA:.0%} away")
    d2, adj, clique, s = ctx.closure_consistency(p, *_a(g), ca, cb, z, ci, GAMMA)
    assert np.array_equal(adj, A) and clique.tolist() == want and s == want_seed
    # d2: four times what a single hypothesis reaches against the same dense inverse, measured here
    uq, pa, pb = P.unique_endpoints(ca, cb)
    Sq = J.joint_dense(p, *_a(g), uq)
    blk = lambda i, j: Sq[3 * i:3 * i + 3, 3 * j:3 * j + 3]   # noqa: E731
    Sz = np.array([J.relative_cov(p[ca[k]], p[cb[k]], blk(pa[k], pa[k]), blk(pa[k], pb[k]), blk(pb[k], pb[k])) for k in range(N)])
    one_ref, _ = J.mahalanobis(J.relative_pose(p[ca], p[cb]), Sz, z, ci)
    one = ctx.relative_covariance(p, *_a(g), ca, cb, z, ci)[2]
    e_one = np.max(np.abs(one - one_ref) / np.maximum(one_ref, 1))
    e_pair = np.max(np.abs(d2 - ref) / np.maximum(ref, 1))
    print(f"generator {seed}: pairwise d2 against the dense reference {e_pair:.2e}; single hypotheses "
          f"(relative_covariance) {e_one:.2e}, bar {4 * e_one:.2e}")
    assert np.array_equal(d2, d2.T) and np.all(np.diag(d2) == 0)
    assert e_pair <= 4 * e_one


# --------------------------------------------------------------------------------------- 4. behaviour
def test_repeatable_cached_poses_untouched_and_limits():
    g = C.CASES["pg500"][0]()
    a = C.args(g)
    c = Context(0)
    rc, p, _ = c.gn_optimize(*a, 4)
    assert rc == 0
    p_in = p.copy()
    ca, cb, z, ci = _pg500_closures(g, p)
    hits = c.symbolic_cache_stats()["hits"]
    r1 = c.closure_consistency(p, *a[1:], ca, cb, z, ci, GAMMA)
    assert c.symbolic_cache_stats()["hits"] == hits + 1          # right after gn_optimize on the same edge list: a hit
    r2 = c.closure_consistency(p, *a[1:], ca, cb, z, ci, GAMMA)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(r1, r2))
    assert c.symbolic_cache_stats()["misses"] == 1 and np.array_equal(p, p_in)
    # nothing queued, nothing written
    d2, adj, clique, seed = c.closure_consistency(p, *a[1:], [], [], np.zeros((0, 3)), np.zeros((0, 6)), GAMMA)
    assert d2.shape == (0, 0) and adj.shape == (0, 0) and len(clique) == 0
    V = len(p)
    over = np.zeros(PCM_MAX_CLOSURES + 1, dtype=np.int32)
    for call in (lambda: c.closure_consistency(p, *a[1:], over, over + 1, np.zeros((len(over), 3)), np.tile(IU, (len(over), 1)), GAMMA),
                 lambda: c.closure_consistency(p, *a[1:], [3], [V], z[:1], ci[:1], GAMMA),
                 lambda: c.closure_consistency(p, *a[1:], [-1], [3], z[:1], ci[:1], GAMMA),
                 lambda: c.closure_consistency(p, *a[1:], ca, cb, z, ci, 0.0),
                 lambda: c.closure_consistency(p, *a[1:], ca, cb, z, ci, float("nan"))):
        with pytest.raises(CgmrError) as ei:
            call()
        assert ei.value.code == E_INVALID
    rc1, p1, chi1 = c.gn_optimize(*a, 6)
    rc2, p2, chi2 = Context(0).gn_optimize(*a, 6)
    assert rc1 == rc2 == 0 and np.array_equal(p1, p2) and np.array_equal(chi1, chi2)


# --------------------------------------------------------------------------------------- 5. robust kernels
def test_robust_equals_the_plain_call_with_scaled_information(ctx):
    g, p = _optimised(ctx, "pg500")
    ef, et, meas, info = g["edge_from"], g["edge_to"], g["meas"], g["info"]
    kinds = np.where(np.abs(ef - et) > 1, RR.KINDS["cauchy"], 0).astype(np.uint8)      # Cauchy on the closures
    w_ref = RR.weights(p, ef, et, meas, info, kinds, 1.0)
    assert (w_ref < 0.9).sum() > 10
    ca, cb, z, ci = _pg500_closures(g, p)
    d2, adj, clique, seed, e2, w = ctx.closure_consistency(p, g["fixed"], ef, et, meas, info, ca, cb, z, ci, GAMMA, kind=kinds, delta=1.0)
    d20 = ctx.closure_consistency(p, g["fixed"], ef, et, meas, info * w_ref[:, None], ca, cb, z, ci, GAMMA)[0]
    plain = ctx.closure_consistency(p, *_a(g), ca, cb, z, ci, GAMMA)[0]
    assert np.abs(w - w_ref).max() <= 1e-12
    err = np.max(np.abs(d2 - d20) / np.maximum(d20, 1))
    diff = np.max(np.abs(plain - d20) / np.maximum(d20, 1))
    print(f"robust d2 vs scaled information: {err:.2e} (the unweighted call differs by {diff:.2e})")
    assert err <= AGREE_TAU and diff > 1e-3


# --------------------------------------------------------------------------------------- 6. wrappers and driver
def test_graph_slam_wrappers_return_the_context_call(ctx):
    g, p = _optimised(ctx, "pg120")
    ca, cb, z, ci, out, ref, A, (want, size, want_seed) = _pg120_reference(ctx, 3)
    gg = dict(g, poses=p.copy())
    gs = GraphSLAM(PoseGraph.from_synth(gg), ctx)
    closures = [(int(ca[k]), int(cb[k]), z[k], ci[k]) for k in range(len(ca))]
    r = gs.closureConsistency(closures, GAMMA)
    r0 = ctx.closure_consistency(p, *_a(g), ca, cb, z, ci, GAMMA)
    assert len(r) == 4 and all(np.array_equal(x, y) for x, y in zip(r, r0))
    assert gs.consistentClosures(closures).tolist() == want
    assert np.array_equal(gs.closureConsistency(closures, GAMMA, robust=True)[0], r[0])      # no kernel set: the plain result
    pg = PoseGraph.from_synth(gg)
    lm = pg.add_vertex(10 ** 6, [1.0, 2.0, 0.0], kind=1)
    pg.add_edge(0, lm, [1.0, 2.0, 0.0], [100.0, 0, 0, 100.0, 0, 0], kind=1)
    with pytest.raises(ValueError):
        GraphSLAM(pg, ctx).consistentClosures(closures)


def _driver(ctx, g, p, ca, cb, z, **kw):
    """A driver whose graph is the 120-vertex graph at its optimum, built by hand, and the candidates as buffer edges."""
    slam = GraphSLAMDriver(ctx, None, None, windowLoopClosure=len(ca), **kw)
    for v in range(len(p)):
        slam._add_vertex(int(g["ids"][v]) if "ids" in g else v, p[v], bool(g["fixed"][v]), np.zeros(4, dtype=np.float32))
    for k in range(len(g["edge_from"])):
        slam._add_edge(int(g["edge_from"][k]), int(g["edge_to"][k]), g["meas"][k], g["info"][k], "odom", k)
    edges = [{"from": int(ca[k]), "to": int(cb[k]), "meas": z[k].copy(), "info": IU, "id": 10000 + k, "added": False}
             for k in range(len(ca))]
    return slam, edges


def _feed(slam, edges):
    """One candidate per key frame, its ``to`` vertex the frame's; the check fires when the first frame's age fills the window."""
    for e in edges:
        slam._last_vertex = e["to"]
        slam.addClosures([e])
        slam.checkClosures()
        slam.updateClosures()


def test_driver_pcm_adds_the_clique_and_voting_is_unchanged(ctx):
    g, p = _optimised(ctx, "pg120")
    ca, cb, z, ci, out, ref, A, (want, size, want_seed) = _pg120_reference(ctx, 3)
    nE = len(g["edge_from"])
    slam, edges = _driver(ctx, g, p, ca, cb, z, closure_check=("pcm", GAMMA))
    _feed(slam, edges)
    assert [e for e in slam.log if e[0] == "pcm"] == [("pcm", 26, 40)]
    lc = [k for k, kind in enumerate(slam.edge_kind) if kind == "lc"]
    assert lc == list(range(nE, nE + 26))
    assert [(int(slam.g.edge_from[k]), int(slam.g.edge_to[k])) for k in lc] == [(int(ca[k]), int(cb[k])) for k in want]
    assert [slam.edge_ids[k] for k in lc] == [10000 + k for k in want]
    assert [k for k, e in enumerate(edges) if e["added"]] == want
    # "voting": the log and the edges of LoopClosureChecker run directly on the same buffer
    kw = dict(inlierThreshold=30.0, minInliers=3)
    slam, edges = _driver(ctx, g, p, ca, cb, z, **kw)
    mine = copy.deepcopy(edges)
    _feed(slam, edges)
    lcc = LoopClosureChecker()
    lcc.init(slam.g.poses, [e["to"] for e in mine], mine, kw["inlierThreshold"])
    lcc.check()
    assert [e for e in slam.log if e[0] in ("lcc", "pcm")] == [("lcc", lcc.inliers(), lcc.chi2())]
    added = [k for k, (e, chi) in enumerate(lcc.closures()) if chi < kw["inlierThreshold"]] if lcc.inliers() >= kw["minInliers"] else []
    assert [k for k, e in enumerate(edges) if e["added"]] == added
    lc = [k for k, kind in enumerate(slam.edge_kind) if kind == "lc"]
    assert [slam.edge_ids[k] for k in lc] == [10000 + k for k in added]
    print(f"voting on the same candidates: {lcc.inliers()} inliers, {len(added)} edges added")
