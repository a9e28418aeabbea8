"""cgmr_closure_consistency_inter[_exact] against yardsticks that are not the code under test: the single-graph call on the
union of the two graphs (existing code: the union's joint covariance is block diagonal), the numpy reference of
ref_pcm_inter.py -- fed the device's own joint covariance for the arithmetic alone, the dense inverse of H end to end --, and
for the driver the same call made directly.  The graphs and candidate sets are tests/pcm_inter_cases.py's; what the end-to-end
sets show on the reference alone is checked in tests/test_pcm_inter_cpu.py.

The bars.  Equivalence: d2 against the single-graph call on the union to the bar test_end_to_end_against_the_dense_reference
holds d2 to (tests/test_pcm_gpu.py) -- four times what cgmr_relative_covariance's d2 reaches in the same run on the same
candidates taken singly, against the dense inverse --, because the two calls factor different matrices; with every peer vertex
fixed in the union both calls factor the own graph alone, and the bar is AGREE_TAU.  Arithmetic: the bar of
test_d2_arithmetic_on_the_device_own_joint_covariance, the terms' size taken over the blocks of both covariances.  End to end:
adjacency, clique and seed equal the reference's on sets whose reference d2 stays 10 % clear of gamma.

Measured on an MI355X: DESIGN.md 2.14."""
import ctypes as C

import numpy as np
import pytest

import pcm_inter_cases as K
import ref_joint_marginals as J
import ref_pcm as P
import ref_pcm_inter as PI
import ref_robust as RR
from cg_mrslam_amd._lib import PCM_MAX_CLOSURES, CgmrError, _ptr
from cg_mrslam_amd.condensed import RobotGraph
from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
from cg_mrslam_amd.mr_graph_slam import INTER_ROBOT_INFO, MRGraphSLAMDriver, team_peer_covariance

pytestmark = pytest.mark.gpu

AGREE_TAU = 1e-9                # two paths on the same factor (test_joint_marginals_gpu.py)
E_INVALID = -1
GAMMA = P.GAMMA_99
PEER_BASE = 10000               # the peer's vertex ids (robot 1)

_CACHE = {}


def _set(seed):
    """A candidate set of the cases module with its peer poses: (ca, pv, peer_pose, z, ci, out)."""
    own, p_own, peer, p_peer = K.graphs()
    ca, pv, z, ci, out = K.candidates(p_own, p_peer, seed)
    return ca, pv, p_peer[pv], z, ci, out


def _device_peer_cov(ctx, pv):
    """The peer graph's joint covariance of the candidates' peer vertices as the device returns it, per candidate."""
    own, p_own, peer, p_peer = K.graphs()
    uq = np.unique(pv).astype(np.int32)
    return K.expand(ctx.marginals_joint(p_peer, *K.args(peer), uq), np.searchsorted(uq, pv))


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(b, 1)))


# --------------------------------------------------------------------------------------- 1. the single-graph call as yardstick
def test_equals_the_single_graph_call_on_the_union_of_the_two_graphs(ctx):
    own, p_own, peer, p_peer = K.graphs()
    seed = K.SEEDS[0]
    ca, pv, pp, z, ci, out = _set(seed)
    N, nO = len(ca), len(p_own)
    pu = np.vstack([p_own, p_peer])
    cb = (pv + nO).astype(np.int32)
    un = K.union(own, peer)
    one = ctx.closure_consistency(pu, *un, ca, cb, z, ci, GAMMA)
    two = ctx.closure_consistency_inter(p_own, *K.args(own), ca, pp, z, ci, GAMMA, peer_cov=_device_peer_cov(ctx, pv))
    # the bar: what a single hypothesis reaches against the dense inverse of the union, measured here, times four
    uq, pa, pb = P.unique_endpoints(ca, cb)
    Sq = J.joint_dense(pu, *un, uq)
    blk = lambda i, j: Sq[3 * i:3 * i + 3, 3 * j:3 * j + 3]   # noqa: E731
    Sz = np.array([J.relative_cov(pu[ca[k]], pu[cb[k]], blk(pa[k], pa[k]), blk(pa[k], pb[k]), blk(pb[k], pb[k])) for k in range(N)])
    one_ref, _ = J.mahalanobis(J.relative_pose(pu[ca], pu[cb]), Sz, z, ci)
    single = ctx.relative_covariance(pu, *un, ca, cb, z, ci)[2]
    e_one = _rel(single, one_ref)
    e_pair = _rel(two[0], one[0])
    off = ~np.eye(N, dtype=bool)
    print(f"generator {seed}: inter d2 against the single-graph call on the union {e_pair:.2e}; single hypotheses "
          f"(relative_covariance) against the dense inverse {e_one:.2e}, bar {4 * e_one:.2e}; nearest d2 to gamma "
          f"{np.min(np.abs(one[0][off] - GAMMA)) / GAMMA:.0%} away")
    assert np.array_equal(two[0], two[0].T) and np.all(np.diag(two[0]) == 0)
    assert e_pair <= 4 * e_one
    assert np.array_equal(two[1], one[1]) and two[2].tolist() == one[2].tolist() and two[3] == one[3]
    assert two[2].tolist() == sorted(set(range(N)) - set(out.tolist()))
    # every peer vertex fixed in the union: its covariance is zero there, and both calls factor the own graph alone
    one_f = ctx.closure_consistency(pu, *K.union(own, peer, peer_all_fixed=True), ca, cb, z, ci, GAMMA)
    two_n = ctx.closure_consistency_inter(p_own, *K.args(own), ca, pp, z, ci, GAMMA)
    e_fixed = _rel(two_n[0], one_f[0])
    print(f"generator {seed}: peer_cov None against the union with every peer vertex fixed {e_fixed:.2e}; None against the peer's "
          f"covariance {_rel(two_n[0], two[0]):.2e}")
    assert e_fixed <= AGREE_TAU
    assert np.array_equal(two_n[1], one_f[1]) and two_n[2].tolist() == one_f[2].tolist() and two_n[3] == one_f[3]
    assert _rel(two_n[0], two[0]) > 1e-3                              # (the covariance does enter)
    # None and an all-zero covariance: identical bytes
    two_0 = ctx.closure_consistency_inter(p_own, *K.args(own), ca, pp, z, ci, GAMMA, peer_cov=np.zeros((3 * N, 3 * N)))
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(two_n, two_0))


# --------------------------------------------------------------------------------------- 2. the d2 arithmetic
def _mixed_set(g, p):
    """30 candidates on the own graph, to 10 peer vertices at random poses with a random positive semidefinite covariance
    (rank 20 of 30): 1 shares its own vertex with 0; 3 ends at the peer vertex 2 ends at; 4 starts at the fixed vertex; 6 repeats
    5 exactly; correlated x / y information on every other one; two far off."""
    rng = np.random.default_rng(17)
    V, N, M = len(p), 30, 10
    peer = rng.uniform(-6, 6, (M, 3)) * [1, 1, 0.5]
    B = rng.normal(0, 1, (3 * M, 20)) * 0.03
    ca = rng.integers(0, V, N).astype(np.int32)
    pv = rng.integers(0, M, N)
    ca[1] = ca[0]
    pv[3] = pv[2]
    ca[4] = int(np.flatnonzero(g["fixed"])[0])
    ca[6], pv[6] = ca[5], pv[5]
    z = J.relative_pose(p[ca], K.se2_mul(K.FRAME, peer[pv])) + rng.normal(0, 1, (N, 3)) * [0.05, 0.05, 0.02]
    z[6] = z[5]
    z[8] += [1.5, -2.0, 0.7]
    z[20] += [-3.0, 0.5, -2.0]
    ci = np.tile(K.IU, (N, 1))
    ci[::2, 1] = 100.0
    ci[6] = ci[5]
    return ca, peer[pv], K.expand(B @ B.T, pv), z, ci


def _one_vertex_set(g, p):
    """12 candidates, all from one own vertex (findInterRobotConstraints matches every peer vertex against one reference
    vertex), to 12 peer vertices with a full-rank covariance."""
    rng = np.random.default_rng(18)
    N = 12
    peer = rng.uniform(-6, 6, (N, 3)) * [1, 1, 0.5]
    B = rng.normal(0, 1, (3 * N, 3 * N)) * 0.02
    ca = np.full(N, 77, dtype=np.int32)
    z = J.relative_pose(p[ca], K.se2_mul(K.FRAME, peer)) + rng.normal(0, 1, (N, 3)) * [0.05, 0.05, 0.02]
    return ca, peer, B @ B.T, z, np.tile(K.IU, (N, 1))


@pytest.mark.parametrize("which", ["mixed", "one_own_vertex"])
def test_d2_arithmetic_on_the_device_own_joint_covariance(ctx, which):
    """The device's propagation against ref_pcm_inter.pair_terms_inter fed the blocks ctx.marginals_joint returns for the unique
    own endpoints and the caller's peer_cov.  Bar per pair, as tests/test_pcm_gpu.py's: 1e-12 of the terms' size -- the sum over
    the block terms of both covariances of ||J_i|| ||J_j|| ||Sigma_ij|| -- times ||S^-1 eps||^2, plus cond(S) d2 at the same
    1e-12."""
    own, p, _, _ = K.graphs()
    ca, pp, pc, z, ci = (_mixed_set if which == "mixed" else _one_vertex_set)(own, p)
    N = len(ca)
    d2, adj, clique, seed = ctx.closure_consistency_inter(p, *K.args(own), ca, pp, z, ci, GAMMA, peer_cov=pc)
    assert d2.shape == (N, N) and np.array_equal(d2, d2.T) and np.all(np.diag(d2) == 0)
    assert np.all(np.isfinite(d2)) and np.all(d2 >= 0)
    uq, pa = PI.unique_own(ca)
    Sq = ctx.marginals_joint(p, *K.args(own), uq)
    worst = 0.0
    for k in range(N):
        for l in range(k):
            eps, S, scale = PI.pair_terms_inter(PI.gather6(Sq, (pa[k], pa[l])), PI.gather6(pc, (k, l)), p[ca[k]], pp[k], p[ca[l]], pp[l],
                                                z[k], z[l], ci[k], ci[l])
            S = 0.5 * (S + S.T)
            if which == "mixed" and (k, l) == (6, 5):
                # the repeated candidate closes an empty loop: eps is exactly 0, and what either side computes is its own
                # rounding of four compositions.  Held, as in tests/test_pcm_gpu.py, to an eps within 1e-12 max(1, |p|) of zero:
                # d2 <= |d eps|^2 ||S^-1||.
                big = max(1.0, np.abs(p).max(), np.abs(pp).max())
                assert d2[k, l] <= (1e-12 * big) ** 2 * np.linalg.norm(np.linalg.inv(S), 2), (d2[k, l], eps)
                continue
            ref = float(eps @ np.linalg.solve(S, eps))
            bar = 1e-12 * (scale * np.linalg.norm(np.linalg.solve(S, eps)) ** 2 + np.linalg.cond(S) * ref)
            worst = max(worst, abs(d2[k, l] - ref) / bar if bar > 0 else 0.0)
            assert abs(d2[k, l] - ref) <= bar, (k, l, d2[k, l], ref, bar)
    print(f"{which}: d2 arithmetic, largest error / bar {worst:.2e}; d2 from {d2[d2 > 0].min():.2e} to {d2.max():.2e}")
    A = P.adjacency(d2, GAMMA)
    want, size, s = P.greedy_clique(A)
    assert np.array_equal(adj, A) and clique.tolist() == want and seed == s
    if which != "mixed":
        return
    rows = np.delete(np.arange(N), [5, 6])
    assert np.array_equal(d2[5, rows], d2[6, rows])
    assert not adj[8].any() and not adj[20].any() and size >= 20
    # an indefinite information: NaN in that candidate's row and column, no adjacency, the rest untouched
    bad = ci.copy()
    bad[9] = [-1e-6, 0, 0, 1.0, 0, 1.0]
    d2n, adjn, cln, _ = ctx.closure_consistency_inter(p, *K.args(own), ca, pp, z, bad, GAMMA, peer_cov=pc)
    others = np.delete(np.arange(N), 9)
    assert np.all(np.isnan(d2n[9, others])) and np.all(np.isnan(d2n[others, 9])) and d2n[9, 9] == 0
    assert not adjn[9].any() and not adjn[:, 9].any() and 9 not in cln.tolist()
    assert np.array_equal(d2n[np.ix_(others, others)], d2[np.ix_(others, others)])


# --------------------------------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("with_cov", [True, False])
@pytest.mark.parametrize("seed", K.SEEDS)
def test_end_to_end_against_the_dense_reference(ctx, seed, with_cov):
    """26 inliers, 14 outliers; the peer's covariance the float64 one of the peer graph, or none.  What the reference shows on
    these sets (clique = the inliers, proven, every d2 10 % clear of gamma): tests/test_pcm_inter_cpu.py."""
    own, p_own, peer, p_peer = K.graphs()
    ca, pv, pp, z, ci, out = _set(seed)
    N = len(ca)
    pc = K.peer_cov_dense(seed) if with_cov else None
    ref = PI.consistency_dense_inter(p_own, *K.args(own), ca, pp, z, ci, pc)
    A = P.adjacency(ref, GAMMA)
    want, size, want_seed = P.greedy_clique(A)
    assert want == sorted(set(range(N)) - set(out.tolist())) and size == 26
    d2, adj, clique, s = ctx.closure_consistency_inter(p_own, *K.args(own), ca, pp, z, ci, GAMMA, peer_cov=pc)
    print(f"generator {seed}, peer_cov {'given' if with_cov else 'None'}: d2 against the dense reference {_rel(d2, ref):.2e}")
    assert np.array_equal(d2, d2.T) and np.all(np.diag(d2) == 0)
    assert np.array_equal(adj, A) and clique.tolist() == want and s == want_seed
    d2x, adjx, cliquex, proven = ctx.closure_consistency_inter_exact(p_own, *K.args(own), ca, pp, z, ci, GAMMA, peer_cov=pc)
    assert proven is True and cliquex.tolist() == want
    assert d2x.tobytes() == d2.tobytes() and np.array_equal(adjx, adj)


# --------------------------------------------------------------------------------------- 4. sizes
def _raw(ctx, g, p, ca, pp, pc, z, ci):
    """The call made on the binding's own arrays, for the adjacency words as the library writes them, padding included."""
    n = len(ca)
    a, pp, pc, cm, ci = ctx._inter_arrays(ca, pp, pc, z, ci)
    W = (n + 63) // 64
    d2, words = np.full((n, n), -1.0), np.full((n, W), ~np.uint64(0), dtype=np.uint64)
    clique, size, seed = np.full(n, -7, dtype=np.int32), np.zeros(1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
    ctx._joint_call("cgmr_closure_consistency_inter", p, *K.args(g),
                    (C.c_int(n), _ptr(a), _ptr(pp), _ptr(pc), _ptr(cm), _ptr(ci), C.c_double(GAMMA), _ptr(d2), _ptr(words), _ptr(clique),
                     _ptr(size), _ptr(seed)), None, 1.0)
    return d2, words, clique, int(size[0]), int(seed[0])


def _sized_set(p_own, p_peer):
    """130 candidates on the cases' graphs, a quarter of them outliers, with the peer graph's float64 covariance."""
    if "sized" not in _CACHE:
        ca, pv, z, ci, out = K.candidates(p_own, p_peer, 21, N=130, n_out=32)
        uq = np.unique(pv)
        cov = J.joint_dense(p_peer, *K.args(K.graphs()[2]), uq.astype(np.int32))
        _CACHE["sized"] = (ca, pv, z, ci, cov, np.searchsorted(uq, pv))
    return _CACHE["sized"]


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 130])
def test_sizes_across_the_pair_mapping_and_the_word_boundaries(ctx, n):
    """The first n of 130 candidates: pair (k, l) is computed from the same poses, measurements and factor whatever n is, so d2
    is the leading block of the 130-candidate call's -- the pair index taken apart rightly at every n -- to AGREE_TAU (the Gram
    tiles of another endpoint set are summed in another order); the adjacency words carry no padding bit, the clique is the
    reference's on the device's own d2."""
    own, p_own, peer, p_peer = K.graphs()
    ca, pv, z, ci, cov, where = _sized_set(p_own, p_peer)
    if "sized_d2" not in _CACHE:
        _CACHE["sized_d2"] = ctx.closure_consistency_inter(p_own, *K.args(own), ca, p_peer[pv], z, ci, GAMMA, peer_cov=K.expand(cov, where))[0]
    full = _CACHE["sized_d2"]
    d2, words, clique, size, seed = _raw(ctx, own, p_own, ca[:n], p_peer[pv[:n]], K.expand(cov, where[:n]), z[:n], ci[:n])
    assert np.array_equal(d2, d2.T) and np.all(np.diag(d2) == 0) and np.all(d2 >= 0)
    assert _rel(d2, full[:n, :n]) <= AGREE_TAU
    if n & 63:
        assert not np.any(words[:, -1] >> np.uint64(n & 63))
    A = P.adjacency(d2, GAMMA)
    assert np.array_equal(ctx._adj_bool(words, n), A)
    want, wsize, wseed = P.greedy_clique(A)
    assert clique[:size].tolist() == want and size == wsize and seed == wseed and np.all(clique[size:] == -1)


# --------------------------------------------------------------------------------------- 5. behaviour
def test_repeatable_poses_untouched_plain_call_unchanged_and_refusals(ctx):
    own, p_own, peer, p_peer = K.graphs()
    a = K.args(own)
    ca, pv, pp, z, ci, out = _set(K.SEEDS[1])
    N = len(ca)
    pc = K.peer_cov_dense(K.SEEDS[1])
    p = p_own.copy()
    cb = ((ca + 1 + pv) % len(p)).astype(np.int32)
    plain = ctx.closure_consistency(p, *a, ca, cb, z, ci, GAMMA)
    for call, kw in ((ctx.closure_consistency_inter, {}), (ctx.closure_consistency_inter, dict(peer_cov=pc)),
                     (ctx.closure_consistency_inter_exact, dict(peer_cov=pc))):
        r1 = call(p, *a, ca, pp, z, ci, GAMMA, **kw)
        r2 = call(p, *a, ca, pp, z, ci, GAMMA, **kw)
        assert len(r1) == 4 and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(r1, r2))
    assert np.array_equal(p, p_own)
    again = ctx.closure_consistency(p, *a, ca, cb, z, ci, GAMMA)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(plain, again))
    # nothing queued, nothing written
    d2, adj, clique, seed = ctx.closure_consistency_inter(p, *a, [], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 6)), GAMMA)
    assert d2.shape == (0, 0) and adj.shape == (0, 0) and len(clique) == 0
    assert len(ctx.closure_consistency_inter_exact(p, *a, [], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 6)), GAMMA)[2]) == 0
    # refused before anything is queued, the candidate named
    V = len(p)
    over = np.zeros(PCM_MAX_CLOSURES + 1, dtype=np.int32)
    nan_pp, inf_pc, neg_pc, up_pc = pp.copy(), pc.copy(), pc.copy(), pc.copy()
    nan_pp[7, 1] = np.nan
    inf_pc[3 * 9 + 1, 3 * 4] = np.inf
    neg_pc[3 * 11 + 2, 3 * 11 + 2] = -1e-9
    up_pc[3 * 4, 3 * 9 + 1] = np.nan                                 # (above the diagonal: never read)
    inter = ctx.closure_consistency_inter
    for call, text in ((lambda: inter(p, *a, over, np.zeros((len(over), 3)), np.zeros((len(over), 3)), np.tile(K.IU, (len(over), 1)), GAMMA), "CGMR_PCM_MAX_CLOSURES"),
                       (lambda: inter(p, *a, [3, V], pp[:2], z[:2], ci[:2], GAMMA), "closure 1"),
                       (lambda: inter(p, *a, [-1], pp[:1], z[:1], ci[:1], GAMMA), "closure 0"),
                       (lambda: inter(p, *a, ca, pp, z, ci, 0.0), "gamma"),
                       (lambda: inter(p, *a, ca, pp, z, ci, float("nan")), "gamma"),
                       (lambda: inter(p, *a, ca, nan_pp, z, ci, GAMMA), "closure 7"),
                       (lambda: inter(p, *a, ca, pp, z, ci, GAMMA, peer_cov=inf_pc), "closures 9 and 4"),
                       (lambda: inter(p, *a, ca, pp, z, ci, GAMMA, peer_cov=neg_pc), "closure 11"),
                       (lambda: ctx.closure_consistency_inter_exact(p, *a, ca, nan_pp, z, ci, GAMMA), "closure 7"),
                       (lambda: ctx.closure_consistency_inter_exact(p, *a, ca, pp, z, ci, GAMMA, node_limit=0), "node_limit")):
        with pytest.raises(CgmrError) as ei:
            call()
        assert ei.value.code == E_INVALID and text in str(ei.value), (text, str(ei.value))
    assert inter(p, *a, ca, pp, z, ci, GAMMA, peer_cov=up_pc)[0].tobytes() == inter(p, *a, ca, pp, z, ci, GAMMA, peer_cov=pc)[0].tobytes()


def test_robust_equals_the_plain_call_with_scaled_information(ctx):
    own, p, _, _ = K.graphs()
    ef, et, meas, info = own["edge_from"], own["edge_to"], own["meas"], own["info"]
    kinds = np.where(np.abs(ef - et) > 1, RR.KINDS["cauchy"], 0).astype(np.uint8)      # Cauchy on the closures
    w_ref = RR.weights(p, ef, et, meas, info, kinds, 1.0)
    assert (w_ref < 0.9).sum() > 10
    ca, pv, pp, z, ci, out = _set(K.SEEDS[2])
    pc = K.peer_cov_dense(K.SEEDS[2])
    inter = ctx.closure_consistency_inter
    d2, adj, clique, seed, e2, w = inter(p, own["fixed"], ef, et, meas, info, ca, pp, z, ci, GAMMA, peer_cov=pc, kind=kinds, delta=1.0)
    d20 = inter(p, own["fixed"], ef, et, meas, info * w_ref[:, None], ca, pp, z, ci, GAMMA, peer_cov=pc)[0]
    plain = inter(p, *K.args(own), ca, pp, z, ci, GAMMA, peer_cov=pc)[0]
    assert np.abs(w - w_ref).max() <= 1e-12
    err, diff = _rel(d2, d20), _rel(plain, d20)
    print(f"robust d2 vs scaled information: {err:.2e} (the unweighted call differs by {diff:.2e})")
    assert err <= AGREE_TAU and diff > 1e-3


# --------------------------------------------------------------------------------------- 6. wrappers and driver
def test_graph_slam_wrapper_returns_the_context_call(ctx):
    own, p_own, peer, p_peer = K.graphs()
    ca, pv, pp, z, ci, out = _set(K.SEEDS[0])
    pc = K.peer_cov_dense(K.SEEDS[0])
    gg = dict(own, poses=p_own.copy())
    gs = GraphSLAM(PoseGraph.from_synth(gg), ctx)
    cands = [(int(ca[k]), pp[k], z[k], ci[k]) for k in range(len(ca))]
    for kw in ({}, dict(peer_cov=pc)):
        r = gs.interRobotConsistency(cands, GAMMA, **kw)
        r0 = ctx.closure_consistency_inter(p_own, *K.args(own), ca, pp, z, ci, GAMMA, **kw)
        assert len(r) == 4 and all(np.array_equal(x, y) for x, y in zip(r, r0))
        rx = gs.interRobotConsistency(cands, peer_cov=kw.get("peer_cov"), exact=True)
        assert len(rx) == 4 and rx[3] is True and rx[2].tolist() == r0[2].tolist()
    pg = PoseGraph.from_synth(gg)
    lm = pg.add_vertex(10 ** 6, [1.0, 2.0, 0.0], kind=1)
    pg.add_edge(0, lm, [1.0, 2.0, 0.0], [100.0, 0, 0, 100.0, 0, 0], kind=1)
    with pytest.raises(ValueError):
        GraphSLAM(pg, ctx).interRobotConsistency(cands)


def _robot(ctx, robot, g, p, **kw):
    """A robot of two whose graph is built by hand (ids from robot * PEER_BASE), as tests/test_mr_graph_slam_gpu.py makes its
    drivers; the inter-robot window is 1, so a buffer is checked as soon as it is filled."""
    slam = MRGraphSLAMDriver(ctx, None, None, RobotGraph(ctx, robot, 2), robot, 2, windowLoopClosure=5, minInliers=4, **kw)
    slam.setInterRobotClosureParams(0.15, 3, 1)
    for v in range(len(p)):
        slam._add_vertex(robot * PEER_BASE + v, p[v], bool(g["fixed"][v]), np.zeros(4, dtype=np.float32))
    for k in range(len(g["edge_from"])):
        slam._add_edge(int(g["edge_from"][k]), int(g["edge_to"][k]), g["meas"][k], g["info"][k], "odom", k)
    return slam


def _fill(slam, ca, pv, pp, z):
    """The candidates into robot 0's buffer for robot 1, as findInterRobotConstraints leaves them: the peer's vertices known by
    the poses it sent, every candidate a closure of its own."""
    for k in range(len(ca)):
        vid = PEER_BASE + int(pv[k])
        slam.peer[vid] = {"pose": pp[k].copy(), "ranges": np.zeros(4, dtype=np.float32)}
        slam.interRobotClosures.insert(slam._closure(int(ca[k]), vid, z[k]), 1)
    return slam.interRobotClosures.mrClosures[1].edges


def _mr_edges(slam):
    return [(int(slam.g.ids[slam.g.edge_from[k]]), int(slam.g.ids[slam.g.edge_to[k]]), slam.edge_ids[k])
            for k, kind in enumerate(slam.edge_kind) if kind == "mr"]


@pytest.mark.parametrize("how", ["pcm", "pcm-exact"])
def test_driver_pcm_adds_exactly_the_clique(ctx, how):
    own, p_own, peer, p_peer = K.graphs()
    ca, pv, pp, z, ci, out = _set(K.SEEDS[0])
    N = len(ca)
    slam = _robot(ctx, 0, own, p_own, mr_closure_check=(how, GAMMA))
    edges = _fill(slam, ca, pv, pp, z)
    assert len(edges) == N
    want = ctx.closure_consistency_inter(p_own, *K.args(own), ca, pp, z, np.tile(INTER_ROBOT_INFO, (N, 1)), GAMMA)[2].tolist()
    assert 3 <= len(want) < N and set(want).isdisjoint(out.tolist())
    first = slam._running_edge_id
    slam.checkInterRobotClosures()
    assert [e for e in slam.log if e[0].startswith("mr_")] == [("mr_" + how, 1, len(want), N) + ((True,) if how == "pcm-exact" else ())]
    assert [k for k, e in enumerate(edges) if e["added"]] == want
    assert _mr_edges(slam) == [(int(ca[k]), PEER_BASE + int(pv[k]), first + 1 + j + slam.baseId) for j, k in enumerate(want)]
    assert slam._running_edge_id == first + len(want)
    assert slam.rg.closures(1, "in").tolist() == sorted({PEER_BASE + int(pv[k]) for k in want})
    assert sorted(int(v) for v in slam.g.ids[len(p_own):]) == sorted({PEER_BASE + int(pv[k]) for k in want})
    # a clique below minInliersMR: logged, nothing added
    slam = _robot(ctx, 0, own, p_own, mr_closure_check=(how, GAMMA))
    slam.setInterRobotClosureParams(0.15, len(want) + 1, 1)
    edges = _fill(slam, ca, pv, pp, z)
    slam.checkInterRobotClosures()
    assert [e[:4] for e in slam.log if e[0].startswith("mr_")] == [("mr_" + how, 1, len(want), N)]
    assert not _mr_edges(slam) and not any(e["added"] for e in edges) and len(slam.rg.closures(1, "in")) == 0


def test_driver_voting_is_the_default_and_unchanged(ctx):
    own, p_own, peer, p_peer = K.graphs()
    ca, pv, pp, z, ci, out = _set(K.SEEDS[0])
    runs = []
    for kw in ({}, dict(mr_closure_check="voting")):
        slam = _robot(ctx, 0, own, p_own, inlierThreshold=30.0, **kw)
        edges = _fill(slam, ca, pv, K.se2_mul(K.FRAME, pp), z)        # (voting reads the peer's poses in the own frame)
        slam.checkInterRobotClosures()
        runs.append((slam.log, _mr_edges(slam), slam.g.ids.tolist(), slam.edge_kind, [e["added"] for e in edges],
                     slam.rg.closures(1, "in").tolist(), slam._running_edge_id))
    assert runs[0] == runs[1]
    log = [e for e in runs[0][0] if e[0].startswith("mr_")]
    assert len(log) == 1 and log[0][0] == "mr_lcc" and log[0][1] == 1
    print(f"voting on the same candidates: {log[0][2]} inliers, {len(runs[0][1])} edges added")


def test_team_peer_covariance_is_the_peers_joint_marginal(ctx):
    """Two robots in one process: robot 0 asks robot 1's driver for the covariance of the vertices its candidates end at."""
    own, p_own, peer, p_peer = K.graphs()
    ca, pv, pp, z, ci, out = _set(K.SEEDS[0])
    N = len(ca)
    slams = {}
    cov = team_peer_covariance(slams)
    slams[0] = _robot(ctx, 0, own, p_own, mr_closure_check=("pcm", GAMMA), mr_peer_covariance=cov)
    slams[1] = _robot(ctx, 1, peer, p_peer)
    vids = [PEER_BASE + int(v) for v in pv]
    got = cov(1, vids)
    uq = np.unique(pv)
    joint = slams[1].jointMarginal([slams[1]._index_of_id(PEER_BASE + int(v)) for v in uq])
    assert got.shape == (3 * N, 3 * N) and got.tobytes() == K.expand(joint, np.searchsorted(uq, pv)).tobytes()
    assert np.array_equal(joint, ctx.marginals_joint(p_peer, *K.args(peer), uq.astype(np.int32)))
    assert cov(1, vids[:3] + [PEER_BASE + len(p_peer)]) is None       # (a vertex the sender does not hold)
    edges = _fill(slams[0], ca, pv, pp, z)
    want = ctx.closure_consistency_inter(p_own, *K.args(own), ca, pp, z, np.tile(INTER_ROBOT_INFO, (N, 1)), GAMMA, peer_cov=got)[2].tolist()
    slams[0].checkInterRobotClosures()
    assert [e for e in slams[0].log if e[0].startswith("mr_")] == [("mr_pcm", 1, len(want), N)]
    assert [k for k, e in enumerate(edges) if e["added"]] == want and len(want) >= 3
