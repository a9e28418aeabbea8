"""Robust kernels in the marginals and the condensed graphs on the device (include/cgmr.h: cgmr_marginals_robust,
cgmr_marginals_all_robust, cgmr_covariance_estimate_robust, cgmr_condense_robust, cgmr_graph_set_condensed_robust) against
the float64 contract of tests/ref_robust_marginals.py.  Every call runs on the session context."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_numpy as R
import ref_robust as RR
import ref_robust_marginals as RM
from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import CgmrError
from reference_cases import EST_ATOL, INFO_RTOL

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the plain paths' bars (test_marginals_gpu.py): covariance blocks 1e-6 of the largest entry, condensed measurements EST_ATOL,
# condensed information 1e-4 of the largest entry -- set by cond(H) times rounding, which the weights do not change much
COV_RTOL = 1e-6
IU_RTOL = 1e-4
W_RTOL = 1e-12            # rho1 of the device's own e2: the kernel formulas, rounding only
E2_RTOL = 1e-6            # e2 at the linearisation point against numpy's: the two sides' poses differ by rounding
KINDS = {"huber": (1, 1.0), "cauchy": (3, 3.0), "dcs": (7, 5.0)}
_CACHE = {}


def fixture(name):
    """(graph dict, poses to linearise at): the golden graphs at their stored optimum, the outlier graph at its Cauchy(3)
    optimum."""
    if name not in _CACHE:
        if name == "outlier":
            g, bad, _ = RR.outlier_graph()
            x, _, _, failed = RR.gn_optimize(g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"], 3, 3.0, 10)
            assert failed is None
            _CACHE[name] = (dict(g, bad=bad), x)
        else:
            d = np.load(os.path.join(GOLDEN, name + ".npz"))
            g = {k: d[k] for k in ("fixed", "edge_from", "edge_to", "meas", "info")}
            g["poses"] = d["poses0"]
            _CACHE[name] = (g, np.array(d["poses"]))
    return _CACHE[name]


def _a(g):
    return g["edge_from"], g["edge_to"], g["meas"], g["info"]


def _query(g, V):
    q = np.linspace(0, V - 1, 24).astype(np.int32)
    if "bad" in g:
        q = np.r_[q, g["edge_from"][g["bad"][:6]], g["edge_to"][g["bad"][:6]]]
    return np.unique(q).astype(np.int32)


def check_weights(poses, g, kind, delta, e2, w):
    ref = RR.edge_chi2(poses, *_a(g))
    assert np.all(np.abs(e2 - ref) <= E2_RTOL * np.abs(ref) + 1e-12), float(np.max(np.abs(e2 - ref)))
    np.testing.assert_allclose(w, RR.rho(kind, delta, e2)[1], rtol=W_RTOL, atol=1e-300)
    np.testing.assert_allclose(w, RR.rho(kind, delta, ref)[1], rtol=1e-5, atol=1e-12)


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


# ------------------------------------------------------------------------------------------------------------------- 1
def test_plain_descriptions_are_bit_identical(ctx):
    """rk = NULL and every edge CGMR_RK_NONE give exactly the plain calls' bytes, for all four entry points."""
    g, p = fixture("gn_v300")
    a = _a(g)
    ef, et, meas, info = (np.ascontiguousarray(x) for x in a)
    V, nE = len(p), len(ef)
    q = np.arange(0, V, 7, dtype=np.int32)
    gauge = V - 1
    lib = ctx.lib
    plain_m = ctx.marginals(p, g["fixed"], *a, q)
    plain_all, plain_cross = ctx.marginals_all(p, g["fixed"], *a, cross=True)
    plain_ce = ctx.covariance_estimate(p, *a, gauge, q)
    plain_c = ctx.condense(p, *a, gauge, q)
    # rk = NULL through the C entry points
    fx = np.ascontiguousarray(g["fixed"], np.uint8)
    cov = np.zeros((len(q), 3, 3))
    assert lib.cgmr_marginals_robust(ctx.h, V, _p(p), _p(fx), nE, _p(ef), _p(et), _p(meas), _p(info), len(q), _p(q), _p(cov), None) == 0
    assert cov.tobytes() == plain_m.tobytes()
    cov, cr = np.zeros((V, 3, 3)), np.zeros((nE, 3, 3))
    assert lib.cgmr_marginals_all_robust(ctx.h, V, _p(p), _p(fx), nE, _p(ef), _p(et), _p(meas), _p(info), _p(cov), _p(cr), None) == 0
    assert cov.tobytes() == plain_all.tobytes() and cr.tobytes() == plain_cross.tobytes()
    cov = np.zeros((len(q), 3, 3))
    assert lib.cgmr_covariance_estimate_robust(ctx.h, V, _p(p), nE, _p(ef), _p(et), _p(meas), _p(info), gauge, len(q), _p(q), _p(cov),
                                               None) == 0
    assert cov.tobytes() == plain_ce.tobytes()
    to, est, iu, cv = np.zeros(len(q), np.int32), np.zeros((len(q), 3)), np.zeros((len(q), 6)), np.zeros((len(q), 3, 3))
    n = lib.cgmr_condense_robust(ctx.h, V, _p(p), nE, _p(ef), _p(et), _p(meas), _p(info), gauge, len(q), _p(q), _p(to), _p(est), _p(iu),
                                 _p(cv), None)
    assert n == len(plain_c[0])
    for x, y in zip((to[:n], est[:n], iu[:n], cv[:n]), plain_c):
        assert x.tobytes() == y.tobytes()
    # every edge "none" (per-edge arrays): the robust instance, weight 1 everywhere
    none = np.zeros(nE, np.uint8)
    m, _, w = ctx.marginals_robust(p, g["fixed"], *a, q, none, np.ones(nE))
    assert m.tobytes() == plain_m.tobytes() and np.all(w == 1.0)
    cov, cr, _, _ = ctx.marginals_all_robust(p, g["fixed"], *a, True, none, np.ones(nE))
    assert cov.tobytes() == plain_all.tobytes() and cr.tobytes() == plain_cross.tobytes()
    assert ctx.covariance_estimate_robust(p, *a, gauge, q, "none")[0].tobytes() == plain_ce.tobytes()
    got = ctx.condense_robust(p, *a, gauge, q, none, 1.0)
    for x, y in zip(got[:4], plain_c):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kname", sorted(KINDS))
@pytest.mark.parametrize("name", ["gn_v300", "gn_v1200", "outlier"])
def test_parity_with_the_float64_reference(ctx, oracle, name, kname):
    kind, delta = KINDS[kname]
    g, p = fixture(name)
    a = _a(g)
    V = len(p)
    q = _query(g, V)
    # marginals: rho1 at the poses given
    cov, e2, w = ctx.marginals_robust(p, g["fixed"], *a, q, kname, delta)
    ref, err, wref = RM.marginals(p, g["fixed"], *a, kind, delta, q)
    assert err.max() <= 1e-10
    check_weights(p, g, kind, delta, e2, w)
    e_m = np.abs(cov - ref).max() / np.abs(ref).max()
    assert e_m <= COV_RTOL
    # marginals_all: the same H, every vertex
    cov_all, e2a, wa = ctx.marginals_all_robust(p, g["fixed"], *a, False, kname, delta)
    assert np.array_equal(wa, w) and np.array_equal(e2a, e2)
    e_a = np.abs(cov_all[q] - ref).max() / np.abs(ref).max()
    assert e_a <= COV_RTOL
    # covariance_estimate / condense: rho1 at the spanning-tree guess from the gauge
    gauge = int(q[len(q) // 2])
    ce, e2c, wc = ctx.covariance_estimate_robust(p, *a, gauge, q, kname, delta)
    rc = RM.condense(p, *a, kind, delta, gauge, q, oracle.initial_guess)
    assert rc["cov_err"].max() <= 1e-10 and not rc["not_pd"].any()
    check_weights(rc["guess"], g, kind, delta, e2c, wc)
    for k, v in enumerate(q):
        if v == gauge:
            assert np.all(ce[k] == 0)
            continue
        j = int(np.flatnonzero(rc["to"] == v)[0])
        assert np.abs(ce[k] - rc["cov"][j]).max() <= COV_RTOL * np.abs(rc["cov"]).max(), int(v)
    to, est, iu, cv, e2d, wd = ctx.condense_robust(p, *a, gauge, q, kname, delta)
    assert np.array_equal(to, rc["to"]) and np.array_equal(wd, wc) and np.array_equal(e2d, e2c)
    d = est - rc["est"]
    d[:, 2] = synth.normalize_theta(d[:, 2])
    e_est = float(np.abs(d).max())
    e_iu = float(np.abs(iu - rc["iu"]).max() / np.abs(rc["iu"]).max())
    assert e_est <= EST_ATOL and e_iu <= IU_RTOL
    assert np.abs(cv - rc["cov"]).max() <= COV_RTOL * np.abs(rc["cov"]).max()
    print(f"{name} {kname}: marginals {e_m:.1e}, marginals_all {e_a:.1e}, condensed est {e_est:.1e} m, information {e_iu:.1e}; "
          f"weights at the guess {wc.min():.3g} .. {wc.max():.3g}")


# ------------------------------------------------------------------------------------------------------------------- 3
def test_batched_robust_condensed_graphs_equal_single_calls(ctx):
    """A robot with three peers, own edges only: computeCondensedGraph(-1) builds the three robust condensed graphs in one batch
    (k_linearize<true, true>); each must match condense_robust on the same edges, gauge and query."""
    from cg_mrslam_amd.condensed import RobotGraph
    from ref_condensed import select_gauge_centroid
    nr, V = 4, 1200
    g = synth.make_pose_graph(V, 4000, seed=61, id_base=0)
    ids = g["ids"].astype(np.int64)
    rg = RobotGraph(ctx, 0, nr)
    try:
        rg.add_vertices(ids, g["poses"], g["fixed"])
        rg.add_edges(ids[g["edge_from"]], ids[g["edge_to"]], g["meas"], g["info"])
        rg.set_edge_robust("cauchy", 1.0)
        rc, _ = rg.optimize(6)
        assert rc == 0
        want = {}
        for p in range(1, nr):
            rng = np.random.default_rng(7 + p)
            want[p] = np.sort(rng.choice(V, 10 + 4 * p, replace=False)).astype(np.int32)
            rg.insertOutClosure(p, ids[want[p]])
        assert rg.computeCondensedGraph(-1) == nr - 1
        plain = {p: rg.condensed(p) for p in want}
        rg.set_condensed_robust(True)
        assert rg.computeCondensedGraph(-1) == nr - 1
        poses = rg.poses()
        worst = np.zeros(2)
        for p, idx in want.items():
            gid, to, est, iu = rg.condensed(p)
            gauge = int(idx[select_gauge_centroid(poses[idx, :2])])
            assert gid == ids[gauge]
            to1, est1, iu1, _, _, w1 = ctx.condense_robust(poses, *_a(g), gauge, idx, "cauchy", 1.0)
            assert np.array_equal(to, ids[to1]) and w1.min() < 0.5
            d = est - est1
            d[:, 2] = synth.normalize_theta(d[:, 2])
            worst = np.maximum(worst, [np.abs(d).max(), max(np.linalg.norm(iu[k] - iu1[k]) / np.linalg.norm(iu1[k]) for k in range(len(to)))])
            assert np.abs(d).max() <= EST_ATOL
            for k in range(len(to)):
                assert np.linalg.norm(iu[k] - iu1[k]) <= INFO_RTOL * np.linalg.norm(iu1[k]), (p, int(to[k]))
            assert not np.allclose(iu, plain[p][3], rtol=1e-3)       # (the switch changes the information)
        print(f"batched robust condensed graphs against single calls: est {worst[0]:.1e} m, information {worst[1]:.1e}")
        rg.set_condensed_robust(False)
        assert rg.computeCondensedGraph(-1) == nr - 1
        for p in want:
            assert [np.asarray(v).tobytes() for v in rg.condensed(p)] == [np.asarray(v).tobytes() for v in plain[p]]
    finally:
        rg.close()


# ------------------------------------------------------------------------------------------------------------------- 4
def test_robot_graph_round_with_robust_condensed_graphs(ctx, oracle):
    """The robot-graph scenario of test_robust_gpu.test_robot_graph_robust_round (a corrupted own closure, Cauchy on the own
    closures), the two robots on the session context.  With the switch on the condensed graphs meet the reference on the own
    edges (rho1 at each graph's spanning-tree guess), the synchronous and the asynchronous builds give the same bytes, and
    switching off restores the plain bytes."""
    from cg_mrslam_amd.mrslam import LoopbackExchange
    from robot_sequences import make_robot_rounds
    rounds = make_robot_rounds([ctx, ctx], 1200, 4000, 44, 60, async_condense=True)
    try:
        ex = LoopbackExchange([rr.g for rr in rounds])
        n_rounds, checked = 5, 0
        for t in range(n_rounds):
            for rr in rounds:
                rr.grow()
                g = rr.g
                if t == n_rounds - 1 and g.counts()["received_edges"] > 0:
                    _, oef, oet, _, _ = g.own_system()
                    id_of = {v: k for k, v in g.index.items()}
                    g.add_edges([id_of[int(oef[3])]], [id_of[int(oet[len(oet) // 2])]], np.array([[7.0, -4.0, 2.0]]),
                                np.array([[100.0, 0, 0, 100.0, 0, 1000.0]]))
                    fixed, oef, oet, ometa, oinfo = g.own_system()
                    closure = np.abs(oet.astype(np.int64) - oef.astype(np.int64)) != 1
                    kind = np.where(closure, 3, 0).astype(np.uint8)
                    rc, _ = g.optimize(3)
                    assert rc == 0
                    peers = [p for p in range(g.n_robots) if p != g.robot and len(g.closures(p)) >= 2]
                    assert peers

                    def build_all(async_):
                        out = {}
                        for peer in peers:
                            if async_:
                                assert g.computeCondensedGraph(peer) > 0
                                g.condensed_wait()
                            else:
                                assert g._check(g.lib.cgmr_graph_compute_condensed(g.h, C.c_int(peer))) > 0
                            out[peer] = [np.asarray(v).tobytes() for v in g.condensed(peer)]
                        return out

                    plain = build_all(False)
                    g.set_edge_robust(kind, 1.0)
                    g.set_condensed_robust(True)
                    sync = build_all(False)
                    assert build_all(True) == sync
                    assert sync != plain
                    poses = g.poses()
                    for peer in peers:
                        gid, to, est, iu = g.condensed(peer)
                        gauge = g.index[gid]
                        tov = np.array([g.index[int(i)] for i in to], np.int32)
                        q = np.r_[gauge, tov].astype(np.int32)
                        ref = RM.condense(poses, oef, oet, ometa, oinfo, kind, 1.0, gauge, q, oracle.initial_guess)
                        assert ref["cov_err"].max() <= 1e-10 and not ref["not_pd"].any()
                        assert np.array_equal(ref["to"], tov)
                        d = est - ref["est"]
                        d[:, 2] = synth.normalize_theta(d[:, 2])
                        assert np.abs(d).max() <= EST_ATOL, float(np.abs(d).max())
                        for k in range(len(tov)):
                            assert np.linalg.norm(iu[k] - ref["iu"][k]) <= INFO_RTOL * np.linalg.norm(ref["iu"][k]), (peer, int(tov[k]))
                    g.set_condensed_robust(False)
                    assert build_all(False) == plain
                    g.set_edge_robust(np.zeros(len(kind), np.uint8), 1.0)
                    checked += 1
                else:
                    rc, _ = g.optimize(5)
                    assert rc == 0
            ex.finish_all()
            for rr in rounds:
                rr.condense()
            ex.start_all()
        ex.finish_all()
        assert checked >= 1
    finally:
        for rr in rounds:
            rr.g.close()


# ------------------------------------------------------------------------------------------------------------------- 5
def test_zero_weights_fail_cleanly_and_tree_edges_weigh_one(ctx):
    """Tukey: vertex 2 hangs on one edge far beyond delta, its block of H is singular -- the marginals return
    CGMR_E_CHOLESKY_BASE.  The condensed / covariance-estimate paths cannot meet this: every free vertex has a spanning-tree edge,
    whose residual at the guess is zero to rounding, so its weight is 1 under every kind."""
    poses = np.array([[0.0, 0, 0], [1.0, 0, 0], [50.0, 0, 0]])
    fixed = np.array([1, 0, 0], dtype=np.uint8)
    ef, et = np.array([0, 1], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    meas = np.array([[1.0, 0, 0], [1.0, 0, 0]])
    info = np.tile([1.0, 0, 0, 1.0, 0, 1.0], (2, 1))
    with pytest.raises(CgmrError) as e:
        ctx.marginals_robust(poses, fixed, ef, et, meas, info, np.array([1, 2], np.int32), "tukey", 2.0)
    assert e.value.code == -100
    with pytest.raises(CgmrError) as e:
        ctx.marginals_all_robust(poses, fixed, ef, et, meas, info, False, "tukey", 2.0)
    assert e.value.code == -100
    g, p = fixture("gn_v300")
    V = len(p)
    q = np.arange(0, V, 11, dtype=np.int32)
    gauge = int(q[3])
    fx = np.zeros(V, np.uint8)
    fx[gauge] = 1
    tree = RM.spanning_tree_edges(V, fx, g["edge_from"], g["edge_to"])
    assert len(tree) == V - 1
    for kname in ("tukey", "saturated", "cauchy"):
        _, _, w = ctx.covariance_estimate_robust(p, *_a(g), gauge, q, kname, 0.5)
        to, _, _, _, _, w2 = ctx.condense_robust(p, *_a(g), gauge, q, kname, 0.5)
        assert len(to) == len(q) - 1
        assert np.abs(w[tree] - 1.0).max() <= 1e-12 and np.array_equal(w, w2)
        assert w.min() < 0.5                                     # (other edges are down-weighted)
