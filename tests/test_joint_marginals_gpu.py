"""cgmr_marginals_joint / cgmr_marginals_pairs / cgmr_relative_covariance against yardsticks that are not the code under test:
a hand-worked chain, the dense inverse on tiny graphs, refined columns of H^-1 on larger ones (ref_joint_marginals.py), the
existing marginals paths (cgmr_marginals, cgmr_marginals_all) on the same factor, and the numpy formulas for the relative
pose's covariance and Mahalanobis distance.

The bars are the ones the existing paths are held to on the same graphs with the same factor (test_marginals_all_gpu.py):
MARG_TAU against the dense inverse and the refined columns (CASE_TAU for the 1500/5000 graph, where the error is the factor's
own, cond(H) u), AGREE_TAU between two paths on one factor.  A refined-columns case that misses its bar measures, in the same
run, the error of the diagonal blocks cgmr_marginals returns for the same queries against the same reference, and holds the
new blocks to four times that.

Measured on an MI355X (largest block error, nK = 5 / 64): dense inverse 3.6e-13 on the 60-vertex graph; refined columns pg500
1.08e-10 / 1.09e-10, hub40 3.2e-12 / 3.2e-12, lat40 7.8e-13 / 7.8e-13, the 1500/5000 graph 1.50e-9 / 1.50e-9 (the value
marginals_all measures there: the factor's own error) -- every case met its bar, the fall-back never ran.  Pairs over every
edge against marginals_all 8.7e-15, joint diagonal blocks against cgmr_marginals 1.9e-16, the relative covariance against
the numpy formula 2.2e-17 of its terms' size, Cauchy against the scaled information 8.5e-12."""
import numpy as np
import pytest

import ref_joint_marginals as J
import ref_numpy as R
import ref_robust as RR
import reference_cases as C
from cg_mrslam_amd import Context, synth
from cg_mrslam_amd._lib import JOINT_MAX_QUERIES, CgmrError, gn_symbolic_info

pytestmark = pytest.mark.gpu

MARG_TAU = 1e-9                 # per block, ||.||_F / sqrt(||Sigma_ii||_F ||Sigma_jj||_F) (test_marginals_all_gpu.py)
CASE_TAU = {"pg1500": 6e-9}     # test_marginals_all_gpu.py's bar for the 1500/5000 graph
AGREE_TAU = 1e-9                # two paths on the same factor
REF_ERR_MAX = 1e-11             # the reference blocks' own error estimate: a case above it is invalid
CHAIN_ATOL = 1e-12              # the closed form of the chain (test_condense_matches_oracle_and_chain_closed_form's bar)
GN_ITERS = 5
E_INVALID = -1


def _graph(name):
    if name == "pg1500":
        return synth.make_pose_graph(1500, 5000, seed=47)
    if name == "small60":
        return synth.make_pose_graph(60, 110, seed=48)
    return C.CASES[name][0]()


_CACHE = {}


def _optimised(ctx, name):
    """(graph, optimised poses) of a named case, computed once and shared (never modified)."""
    if name not in _CACHE:
        g = _graph(name)
        rc, p, _ = ctx.gn_optimize(*C.args(g), GN_ITERS)
        assert rc == 0
        p.setflags(write=False)
        _CACHE[name] = (g, p)
    return _CACHE[name]


def _a(g):
    return g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"]


def _blk(S, k, l):
    return S[3 * k:3 * k + 3, 3 * l:3 * l + 3]


def _queries(g, nK):
    """nK distinct vertices: spread over the whole graph (different subtrees of the elimination tree), plus the vertices
    eliminated last (the root front / top block)."""
    V = len(g["poses"])
    ntop = 2 if nK <= 5 else 12
    _, perm = gn_symbolic_info(V, g["fixed"], g["edge_from"], g["edge_to"], want_perm=True)
    dead = R.active_fixed(V, g["fixed"], g["edge_from"], g["edge_to"]) != 0       # (zeros: checks 1 and 5)
    pick = [int(v) for v in np.argsort(perm) if not dead[v]][-ntop:]
    for v in np.linspace(1, V - 1, 4 * nK).astype(int)[::-1]:
        if len(pick) >= nK:
            break
        if int(v) not in pick and not dead[v]:
            pick.append(int(v))
    assert len(pick) == nK
    return np.array(pick[::-1], dtype=np.int32)                  # (unsorted: spread first, descending, then the top block)


# --------------------------------------------------------------------------------------- 1. the hand-worked chain
def test_chain_closed_form_orientation_zeros_and_relative_covariance(ctx):
    g = J.chain_graph()
    p = g["poses"]
    q = [4, 0, 2, 5, 2, 1, 3]                                    # unsorted, one duplicate, the fixed vertex
    S = ctx.marginals_joint(p, *_a(g), q)
    assert S.shape == (21, 21)
    blk = lambda j, k: _blk(S, q.index(j), q.index(k))   # noqa: E731
    for j in range(1, 6):
        for k in range(1, 6):
            assert abs(blk(j, k)[0, 0] - min(j, k) / 100) <= CHAIN_ATOL, (j, k)
            assert abs(blk(j, k)[2, 2] - min(j, k) / 1000) <= CHAIN_ATOL, (j, k)
    # the A/B-orientation check: an off-diagonal block is not symmetric
    assert abs(blk(2, 4)[1, 2] - 0.001) <= CHAIN_ATOL and abs(blk(2, 4)[2, 1] - 0.005) <= CHAIN_ATOL
    ref = J.joint_dense(p, *_a(g), q)
    print(f"chain: largest difference to the dense inverse {np.abs(S - ref).max():.2e}")
    assert np.abs(S - ref).max() <= CHAIN_ATOL
    assert np.array_equal(blk(4, 2), blk(2, 4).T)
    i0 = 3 * q.index(0)
    assert np.all(S[i0:i0 + 3] == 0) and np.all(S[:, i0:i0 + 3] == 0)
    assert np.array_equal(S, S.T)
    assert np.array_equal(S[6:9], S[12:15]) and np.array_equal(S[:, 6:9], S[:, 12:15])      # vertex 2, listed twice
    # relative covariance: 3 steps apart is the same matrix wherever the pair sits, the fixed vertex included.
    # Bar: CHAIN_ATOL on each block, times the 4 terms' ||J_a|| ||J_b|| <= 1 + 1 + 1 + 3^2 = 12 (Frobenius, |dx| <= 3)
    pa, pb = [1, 2, 0, 3, 3], [4, 5, 3, 4, 3]
    z, Sz, d2 = ctx.relative_covariance(p, *_a(g), pa, pb)
    assert d2 is None
    assert np.array_equal(z, J.relative_pose(p[pa], p[pb]))
    want = np.array([[.03, 0, 0], [0, .035, .003], [0, .003, .003]])
    tol = 4 * 12 * CHAIN_ATOL
    for k in range(3):
        assert np.abs(Sz[k] - want).max() <= tol, (k, Sz[k])
    assert np.abs(Sz[3] - np.diag([.01, .01, .001])).max() <= tol
    assert np.abs(Sz[4]).max() <= tol                            # (a, a): zero to rounding
    print(f"chain: (a, a) relative covariance, largest element {np.abs(Sz[4]).max():.2e}")


# --------------------------------------------------------------------------------------- 2. the dense inverse
DENSE = [("v2e1", None), ("v5e4", None), ("small60", None)] + [("small60", n) for n in (1, 3, 4, 5, 17)]


@pytest.mark.parametrize("name,nK", DENSE)
def test_joint_against_the_dense_inverse(ctx, name, nK):
    """Every vertex, and on the 60-vertex graph subsets that fill a 16-column tile partly (1, 3), exactly (4) and reach into
    a second (5) and a fifth (17) tile."""
    g, p = _optimised(ctx, name)
    V = len(p)
    q = np.arange(V, dtype=np.int32) if nK is None else np.random.default_rng(nK).permutation(V)[:nK].astype(np.int32)
    S = ctx.marginals_joint(p, *_a(g), q)
    ref = J.joint_dense(p, *_a(g), q)
    err = J.block_errors(S, ref)
    print(f"{name} nK={len(q)}: largest block error against the dense inverse {err.max():.2e}")
    assert np.array_equal(S, S.T)
    assert err.max() <= MARG_TAU


# --------------------------------------------------------------------------------------- 3. refined columns
@pytest.mark.parametrize("nK", [5, 64])
@pytest.mark.parametrize("name", ["pg500", "hub40", "lat40", "pg1500"])
def test_joint_against_refined_columns(ctx, name, nK):
    g, p = _optimised(ctx, name)
    q = _queries(g, nK)
    S = ctx.marginals_joint(p, *_a(g), q)
    ref, rerr = J.joint_refined(p, *_a(g), q)
    nd = np.array([np.linalg.norm(_blk(ref, k, k)) for k in range(nK)])
    assert nd.min() > 0
    own = max(np.linalg.norm(_blk(rerr, k, l)) / np.sqrt(nd[k] * nd[l]) for k in range(nK) for l in range(nK))
    assert own <= REF_ERR_MAX, ("the reference itself is not accurate enough here", own)
    err = J.block_errors(S, ref)
    off = err[~np.eye(nK, dtype=bool)].max()
    tau = CASE_TAU.get(name, MARG_TAU)
    print(f"{name} nK={nK}: largest block error {err.max():.2e} (off-diagonal {off:.2e}), reference's own {own:.2e}, bar {tau:.1e}")
    assert np.array_equal(S, S.T)
    if err.max() > tau:
        # the factor's own error: what do the parent path's diagonal blocks reach for the same queries, same reference?
        d = ctx.marginals(p, *_a(g), q)
        perr = max(np.linalg.norm(d[k] - _blk(ref, k, k)) / nd[k] for k in range(nK))
        print(f"{name} nK={nK}: cgmr_marginals' diagonal blocks reach {perr:.2e}; new blocks held to four times that")
        assert err.max() <= 4 * perr


# --------------------------------------------------------------------------------------- 4. agreement with existing paths
def test_pairs_over_every_edge_agree_with_marginals_all(ctx):
    g, p = _optimised(ctx, "pg1500")
    ef, et = g["edge_from"], g["edge_to"]
    cov, cross = ctx.marginals_all(p, *_a(g), cross=True)
    aa, ab, bb = ctx.marginals_pairs(p, *_a(g), ef, et)
    nd = np.linalg.norm(cov, axis=(1, 2))
    live = (nd[ef] > 0) & (nd[et] > 0)
    assert live.sum() > 4900 and np.all(ab[~live] == 0) and np.all(cross[~live] == 0)
    e_ab = np.linalg.norm(ab - cross, axis=(1, 2))[live] / np.sqrt(nd[ef] * nd[et])[live]
    la, lb = nd[ef] > 0, nd[et] > 0
    e_aa = np.linalg.norm(aa - cov[ef], axis=(1, 2))[la] / nd[ef][la]
    e_bb = np.linalg.norm(bb - cov[et], axis=(1, 2))[lb] / nd[et][lb]
    print(f"pairs vs marginals_all on {len(ef)} edges: ab {e_ab.max():.2e}, aa {e_aa.max():.2e}, bb {e_bb.max():.2e}")
    assert max(e_ab.max(), e_aa.max(), e_bb.max()) <= AGREE_TAU
    assert np.all(aa[~la] == 0) and np.all(bb[~lb] == 0)


def test_joint_diagonal_blocks_agree_with_marginals(ctx):
    g, p = _optimised(ctx, "pg1500")
    q = _queries(g, 64)
    S = ctx.marginals_joint(p, *_a(g), q)
    d = ctx.marginals(p, *_a(g), q)
    err = max(np.linalg.norm(_blk(S, k, k) - d[k]) / np.linalg.norm(d[k]) for k in range(len(q)))
    print(f"joint diagonal blocks vs cgmr_marginals: {err:.2e}")
    assert err <= AGREE_TAU


# --------------------------------------------------------------------------------------- 5. zeros and duplicates
def test_pairs_zeros_and_duplicates(ctx):
    g, p = _optimised(ctx, "fixed_dup_iso")
    fixed = g["fixed"].copy()
    fixed[[5, 77]] = 1
    ef, et = g["edge_from"], g["edge_to"]
    dead = R.active_fixed(len(p), fixed, ef, et) != 0
    assert dead[[0, 5, 40, 77, 119, 120, 121]].all() and not dead[[10, 20, 60]].any()
    pa = np.array([5, 10, 10, 10, 0, 120, 60, 77], dtype=np.int32)
    pb = np.array([10, 77, 10, 20, 5, 10, 60, 77], dtype=np.int32)
    aa, ab, bb = ctx.marginals_pairs(p, fixed, ef, et, g["meas"], g["info"], pa, pb)
    for k in range(len(pa)):
        if dead[pa[k]] or dead[pb[k]]:
            assert np.all(ab[k] == 0), k                          # a fixed / inactive end: zero cross block
        assert np.all(aa[k] == 0) == bool(dead[pa[k]]) and np.all(bb[k] == 0) == bool(dead[pb[k]]), k
    for k in (2, 6):                                              # (a, a)
        assert np.array_equal(aa[k], ab[k]) and np.array_equal(ab[k], bb[k]) and np.array_equal(ab[k], ab[k].T)
    assert ab[3].any() and np.array_equal(aa[3], aa[2]) and np.array_equal(aa[1], aa[2])
    S = ctx.marginals_joint(p, fixed, ef, et, g["meas"], g["info"], [10, 5, 20, 120, 10])
    scale = np.sqrt(np.linalg.norm(aa[3]) * np.linalg.norm(bb[3]))
    assert np.linalg.norm(_blk(S, 0, 2) - ab[3]) <= AGREE_TAU * scale and np.array_equal(_blk(S, 2, 0), _blk(S, 0, 2).T)
    assert np.all(S[3:6] == 0) and np.all(S[9:12] == 0) and np.array_equal(S[0:3], S[12:15]) and np.array_equal(S, S.T)
    ref = J.joint_dense(p, fixed, ef, et, g["meas"], g["info"], [10, 5, 20, 120, 10])
    assert J.block_errors(S, ref).max() <= MARG_TAU


# --------------------------------------------------------------------------------------- 6. relative-covariance arithmetic
def test_relative_covariance_arithmetic(ctx):
    """The device's propagation against the numpy formula on the device's own pair blocks.  Bar: 1e-12 (about 1e4 unit
    round-offs, on a sum of roughly a hundred terms) of the size of the terms, ||J_a||^2 ||Saa|| + 2 ||J_a|| ||J_b|| ||Sab||
    + ||J_b||^2 ||Sbb|| -- not of the result, which for nearby poses is far smaller than its terms.  d2 = e^T S^-1 e moves by
    -e^T S^-1 dS S^-1 e under an error dS of S: the same 1e-12 of the terms' size times ||S^-1 e||^2, plus what solving
    with S costs in itself, cond(S) d2, at the same 1e-12."""
    g, p = _optimised(ctx, "pg500")
    rng = np.random.default_rng(6)
    V = len(p)
    pa = np.r_[rng.integers(0, V, 40), g["edge_from"][:20], [7, 0]].astype(np.int32)
    pb = np.r_[rng.integers(0, V, 40), g["edge_to"][:20], [7, 300]].astype(np.int32)
    n = len(pa)
    z_ref = J.relative_pose(p[pa], p[pb])
    zh = z_ref + rng.normal(0, 1, (n, 3)) * [0.05, 0.05, 0.02]
    hi = np.tile([1000.0, 0, 0, 1000.0, 0, 10000.0], (n, 1))
    hi[::2, 1] = 100.0                                           # (correlated x / y noise in every other hypothesis)
    aa, ab, bb = ctx.marginals_pairs(p, *_a(g), pa, pb)
    z, Sz, d2 = ctx.relative_covariance(p, *_a(g), pa, pb, zh, hi)
    z0, Sz0, d20 = ctx.relative_covariance(p, *_a(g), pa, pb, zh)
    assert np.array_equal(z, z0) and np.array_equal(Sz, Sz0)
    assert np.abs(z - z_ref).max() <= 1e-12 * max(1.0, np.abs(p).max())
    want = J.relative_cov(p[pa], p[pb], aa, ab, bb)
    scale = J.relative_cov_scale(p[pa], p[pb], aa, ab, bb)
    e_cov = np.linalg.norm(Sz - want, axis=(1, 2))
    print(f"relative covariance: largest error / terms' size {np.max(e_cov / scale):.2e}; smallest ||Sigma_z|| / terms' size "
          f"{np.min(np.linalg.norm(want, axis=(1, 2))[:-2] / scale[:-2]):.2e}")
    assert np.all(e_cov <= 1e-12 * scale)
    assert np.array_equal(Sz, np.transpose(Sz, (0, 2, 1)))
    for got, info in ((d2, hi), (d20, None)):
        ref, S = J.mahalanobis(z_ref, want, zh, info)
        e, _ = J.hypothesis_error(z_ref, zh)
        for k in range(n):
            if info is None and pa[k] == pb[k]:                  # (a, a) without measurement noise: S is zero to rounding
                continue
            assert np.isfinite(ref[k]), k
            Sk = 0.5 * (S[k] + S[k].T)
            bar = 1e-12 * (scale[k] * np.linalg.norm(np.linalg.solve(Sk, e[k])) ** 2 + np.linalg.cond(Sk) * ref[k])
            assert abs(got[k] - ref[k]) <= bar, (k, got[k], ref[k], bar)
    assert np.all(np.isfinite(d2)) and np.all(d2 >= 0)
    # not positive definite: NaN
    _, _, dn = ctx.relative_covariance(p, *_a(g), pa[:4], pb[:4], zh[:4], np.tile([-1e-6, 0, 0, 1.0, 0, 1.0], (4, 1)))
    assert np.all(np.isnan(dn))


# --------------------------------------------------------------------------------------- 7. robust kernels
def test_robust_equals_the_plain_call_with_scaled_information(ctx):
    g, p = _optimised(ctx, "pg500")
    ef, et, meas, info = g["edge_from"], g["edge_to"], g["meas"], g["info"]
    kinds = np.where(np.abs(ef - et) > 1, RR.KINDS["cauchy"], 0).astype(np.uint8)      # Cauchy on the closures
    w_ref = RR.weights(p, ef, et, meas, info, kinds, 1.0)
    assert (w_ref < 0.9).sum() > 10
    info_w = info * w_ref[:, None]
    q = _queries(g, 17)
    S, e2, w = ctx.marginals_joint(p, g["fixed"], ef, et, meas, info, q, kind=kinds, delta=1.0)
    S0 = ctx.marginals_joint(p, g["fixed"], ef, et, meas, info_w, q)
    assert np.abs(w - w_ref).max() <= 1e-12
    err = J.block_errors(S, S0)
    plain = J.block_errors(ctx.marginals_joint(p, *_a(g), q), S0)
    print(f"robust joint vs scaled information: {err.max():.2e} (the unweighted call differs by {plain.max():.2e})")
    assert err.max() <= AGREE_TAU and plain.max() > 1e-3
    pa, pb = q[:8], q[8:16]
    r = ctx.marginals_pairs(p, g["fixed"], ef, et, meas, info, pa, pb, kind=kinds, delta=1.0)
    r0 = ctx.marginals_pairs(p, g["fixed"], ef, et, meas, info_w, pa, pb)
    nd = lambda x: np.linalg.norm(x, axis=(1, 2))   # noqa: E731
    for k in range(3):
        assert np.max(nd(r[k] - r0[k]) / np.sqrt(nd(r0[0]) * nd(r0[2]))) <= AGREE_TAU
    z, Sz, _, _, w2 = ctx.relative_covariance(p, g["fixed"], ef, et, meas, info, pa, pb, kind=kinds, delta=1.0)
    z0, Sz0, _ = ctx.relative_covariance(p, g["fixed"], ef, et, meas, info_w, pa, pb)
    assert np.array_equal(z, z0) and np.array_equal(w2, w)
    assert np.max(nd(Sz - Sz0) / J.relative_cov_scale(p[pa], p[pb], *r0)) <= AGREE_TAU


# --------------------------------------------------------------------------------------- 8. behaviour
def test_repeatable_cached_and_poses_untouched():
    g = _graph("pg500")
    a = C.args(g)
    c = Context(0)
    rc, p, _ = c.gn_optimize(*a, 4)
    assert rc == 0
    p_in = p.copy()
    q = _queries(g, 64)
    hits = c.symbolic_cache_stats()["hits"]
    S1 = c.marginals_joint(p, *a[1:], q)
    assert c.symbolic_cache_stats()["hits"] == hits + 1          # right after gn_optimize on the same edge list: a hit
    S2 = c.marginals_joint(p, *a[1:], q)
    assert S1.tobytes() == S2.tobytes()
    r1 = c.marginals_pairs(p, *a[1:], g["edge_from"], g["edge_to"])
    r2 = c.marginals_pairs(p, *a[1:], g["edge_from"], g["edge_to"])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r1, r2))
    t1 = c.relative_covariance(p, *a[1:], q[:32], q[32:], p[q[:32]] * 0.01)
    t2 = c.relative_covariance(p, *a[1:], q[:32], q[32:], p[q[:32]] * 0.01)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(t1, t2))
    assert c.symbolic_cache_stats()["misses"] == 1 and np.array_equal(p, p_in)
    # the dense layout (macro-tiles) and the tile list split the rows differently: the same blocks to AGREE_TAU
    k, l = np.tril_indices(len(q))
    aa, ab, bb = c.marginals_pairs(p, *a[1:], q[k], q[l])
    nd = np.sqrt(np.linalg.norm(aa, axis=(1, 2)) * np.linalg.norm(bb, axis=(1, 2)))
    dense = np.array([_blk(S1, k[n], l[n]) for n in range(len(k))])
    assert np.max(np.linalg.norm(ab - dense, axis=(1, 2)) / nd) <= AGREE_TAU
    # nothing queued, nothing written
    assert c.marginals_joint(p, *a[1:], []).shape == (0, 0)
    assert all(x.shape[0] == 0 for x in c.marginals_pairs(p, *a[1:], [], []))
    rc1, p1, chi1 = c.gn_optimize(*a, 6)
    rc2, p2, chi2 = Context(0).gn_optimize(*a, 6)
    assert rc1 == rc2 == 0 and np.array_equal(p1, p2) and np.array_equal(chi1, chi2)


def test_limits_and_bad_indices(ctx):
    g = _graph("pg2500")
    a = C.args(g)
    V = len(g["poses"])
    assert V > JOINT_MAX_QUERIES
    over = np.arange(JOINT_MAX_QUERIES + 1, dtype=np.int32)
    for call in (lambda: ctx.marginals_joint(*a, over),
                 lambda: ctx.marginals_pairs(*a, over, over[::-1]),
                 lambda: ctx.relative_covariance(*a, over, over),
                 lambda: ctx.marginals_joint(*a, [3, V]),
                 lambda: ctx.marginals_joint(*a, [-1]),
                 lambda: ctx.marginals_pairs(*a, [3], [V]),
                 lambda: ctx.relative_covariance(*a, [V], [3])):
        with pytest.raises(CgmrError) as ei:
            call()
        assert ei.value.code == E_INVALID
    # the limit counts unique vertices: twice as many queries over half as many vertices pass it
    q = np.r_[np.arange(8), np.arange(8)].astype(np.int32)
    assert ctx.marginals_joint(*a, q).shape == (48, 48)


def test_graph_slam_wrappers_return_the_context_calls(ctx):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = synth.make_pose_graph(300, 900, seed=21)
    pg = PoseGraph.from_synth(g)
    loops = np.flatnonzero(np.abs(pg.edge_from - pg.edge_to) > 1)
    pg.edge_level[loops[::7]] = 1                               # not active in the optimisation: left out
    gs = GraphSLAM(pg, ctx)
    gs.optimize(3)
    lv0 = (pg.poses, pg.fixed, *pg.level0())
    pairs = [(10, 250), (250, 10), (0, 5), (40, 40), (17, 18)]
    blocks = gs.computeMarginalBlocks(pairs)
    aa, ab, bb = ctx.marginals_pairs(*lv0, [p[0] for p in pairs], [p[1] for p in pairs])
    assert list(blocks) == pairs and all(np.array_equal(blocks[p], ab[k]) for k, p in enumerate(pairs))
    assert np.array_equal(blocks[(10, 250)], blocks[(250, 10)].T) and blocks[(10, 250)].any()
    d40 = gs.computeMarginals()[40]                              # (selected inversion: another path on the same factor)
    assert np.linalg.norm(blocks[(40, 40)] - d40) <= AGREE_TAU * np.linalg.norm(d40)
    verts = [250, 10, 40]
    assert np.array_equal(gs.jointMarginal(verts), ctx.marginals_joint(*lv0, verts))
    zh = np.array([[1.0, 0.5, 0.1]] * len(pairs))
    hi = np.tile([500.0, 0, 0, 500.0, 0, 5000.0], (len(pairs), 1))
    z, Sz, d2 = gs.relativeCovariance(pairs, (zh, hi))
    z0, Sz0, d20 = ctx.relative_covariance(*lv0, [p[0] for p in pairs], [p[1] for p in pairs], zh, hi)
    assert np.array_equal(z, z0) and np.array_equal(Sz, Sz0) and np.array_equal(d2, d20)
    assert len(gs.relativeCovariance(pairs)) == 2
    # robust=True without a kernel set is the plain result; with Cauchy on every edge it is the Context's robust call
    assert np.array_equal(gs.jointMarginal(verts, robust=True), gs.jointMarginal(verts))
    gs.setRobustKernel("Cauchy", 1.0)
    Sr = gs.jointMarginal(verts, robust=True)
    assert np.array_equal(Sr, ctx.marginals_joint(*lv0, verts, kind="cauchy", delta=1.0)[0])
    assert not np.array_equal(Sr, gs.jointMarginal(verts))
