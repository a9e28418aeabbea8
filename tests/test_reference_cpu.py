"""The yardsticks of tests/test_reference_gpu.py, proven on the CPU before anyone trusts them on the GPU: the componentwise
backward error of a Gauss-Newton step (ref_numpy.step_backward_error) is calibrated on two independent solvers (the C oracle
and SuperLU) over the whole case matrix, and shown to catch a 1e-9 relative error in one block of H and a dropped duplicate
edge; the refined marginal columns (ref_numpy.marginal_blocks_ref) agree with a dense inverse and a closed form; the numpy
unscented labelling (ref_numpy.label_edges_ut) agrees with the oracle's condensed graph."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import ref_numpy as R
import reference_cases as C
from reference_cases import EST_ATOL, OMEGA_MAX
from cg_mrslam_amd import synth


def _steps(oracle, g):
    """(poses0, oracle's one-iteration step, SuperLU's one-iteration step) from the initial guess, the 3rd and the 8th iterate."""
    a = C.args(g)
    fx = R.active_fixed(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    pts = [g["poses"]]
    for it in (3, 8):
        st, p, _, _ = oracle.gn_optimize(*a, it)
        assert st == 0
        pts.append(p)
    for p0 in pts:
        st, p1, _, _ = oracle.gn_optimize(p0, *a[1:], 1)
        assert st == 0
        q1, _ = R.gn_optimize(p0, fx, *a[2:], 1)
        yield p0, p1, q1


def test_omega_calibration(oracle):
    """OMEGA_MAX is ten times the largest backward error two independent double-precision solvers show on the case matrix
    (measured: 11 u, C2's first step; most steps 0 u)."""
    assert OMEGA_MAX <= 1e-12
    worst = {}
    for name, (make, _) in C.CASES.items():
        g = make()
        for p0, p1, q1 in _steps(oracle, g):
            for w in (R.step_backward_error(p0, p1, *C.args(g)[1:]), R.step_backward_error(p0, q1, *C.args(g)[1:])):
                worst[name] = max(worst.get(name, 0.0), w)
    assert max(worst.values()) * 10 <= OMEGA_MAX, {k: v / R.U for k, v in worst.items()}
    assert max(worst.values()) > 0                   # (the yardstick is not blind: rounding shows)


def _perturbed_step(g, scale_block=None, drop_edge=None):
    """One SuperLU step on a deliberately wrong system: one off-diagonal 3x3 block (and its mirror) scaled, or one edge
    left out of the assembly.  Returns (poses0, poses1)."""
    p0 = g["poses"]
    fx = R.active_fixed(len(p0), g["fixed"], g["edge_from"], g["edge_to"])
    keep = np.ones(len(g["edge_from"]), dtype=bool)
    if drop_edge is not None:
        keep[drop_edge] = False
    H, b, hidx = R.build_system(p0, fx, g["edge_from"][keep], g["edge_to"][keep], g["meas"][keep], g["info"][keep])
    if scale_block is not None:
        i, j, f = scale_block
        H = H.tolil()
        for a in (i, j):
            c = j if a == i else i
            blk = H[3 * a:3 * a + 3, 3 * c:3 * c + 3].toarray()
            H[3 * a:3 * a + 3, 3 * c:3 * c + 3] = blk * f
        H = H.tocsc()
    dx = spla.splu(H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True)).solve(b)
    p1 = p0.copy()
    free = hidx >= 0
    d = dx.reshape(-1, 3)
    p1[free, :2] += d[:, :2]
    p1[free, 2] = R.normalize_theta(p1[free, 2] + d[:, 2])
    return p0, p1


@pytest.mark.parametrize("name", ["pg500", "hub40", "lat40", "fixed_dup_iso"])
def test_omega_catches_a_1e9_error_in_one_block(name):
    g = C.CASES[name][0]()
    a = C.args(g)
    p0, p1 = _perturbed_step(g)
    assert R.step_backward_error(p0, p1, *a[1:]) <= OMEGA_MAX
    # the off-diagonal block that carries the largest share of its row's |H||dx| (a loop closure or odometry edge)
    fx = R.active_fixed(len(p0), g["fixed"], g["edge_from"], g["edge_to"])
    H, _, hidx = R.build_system(p0, fx, *a[2:])
    dx = np.zeros(H.shape[0])
    free = hidx >= 0
    d = p1[free] - p0[free]
    d[:, 2] = R.normalize_theta(d[:, 2])
    dx[:] = d.ravel()
    hi, hj = hidx[g["edge_from"]], hidx[g["edge_to"]]
    both = np.flatnonzero((hi >= 0) & (hj >= 0))
    Ha = abs(H).tocsr()
    row_mag = Ha @ np.abs(dx)
    share = [np.abs(H[3 * hi[k]:3 * hi[k] + 3, 3 * hj[k]:3 * hj[k] + 3].toarray()) @ np.abs(dx[3 * hj[k]:3 * hj[k] + 3])
             / row_mag[3 * hi[k]:3 * hi[k] + 3] for k in both]
    k = both[int(np.argmax([s.max() for s in share]))]
    q0, q1 = _perturbed_step(g, scale_block=(hi[k], hj[k], 1 + 1e-9))
    w = R.step_backward_error(q0, q1, *a[1:])
    assert w >= 100 * OMEGA_MAX, w


def test_omega_catches_a_dropped_duplicate_edge():
    g = C.fixed_dup_isolated_graph()
    a = C.args(g)
    E = len(g["edge_from"])
    p0, p1 = _perturbed_step(g, drop_edge=E - 1)            # one of the 25 duplicates (its twin is edge 24)
    w = R.step_backward_error(p0, p1, *a[1:])
    assert w >= 100 * OMEGA_MAX, w
    p0, p1 = _perturbed_step(g)
    assert R.step_backward_error(p0, p1, *a[1:]) <= OMEGA_MAX


@pytest.mark.parametrize("V,E,seed", [(60, 110, 1), (200, 600, 2)])
def test_marginal_blocks_ref_matches_dense_inverse(V, E, seed):
    g = synth.make_pose_graph(V, E, seed=seed)
    a = C.args(g)
    p, _ = R.gn_optimize(g["poses"], g["fixed"], *a[2:], 6)
    query = np.arange(V)
    want = R.marginals_dense(p, g["fixed"], *a[2:], query)
    H, _, hidx = R.build_system(p, g["fixed"], *a[2:])
    got, err = R.marginal_blocks_ref(H, hidx, query)
    assert err.max() <= 1e-11
    assert np.all(got[0] == 0)                                  # the fixed vertex
    for k in range(1, V):
        assert np.linalg.norm(got[k] - want[k]) <= 1e-10 * np.linalg.norm(want[k])


def test_marginal_blocks_ref_chain_closed_form():
    """A straight chain from a fixed vertex: the x and theta variances add up edge by edge."""
    V = 40
    poses = np.array([[float(k), 0, 0] for k in range(V)])
    fixed = np.zeros(V, np.uint8); fixed[0] = 1
    ef = np.arange(V - 1, dtype=np.int32)
    meas = np.tile([1.0, 0, 0], (V - 1, 1))
    info = np.tile([100.0, 0, 0, 100, 0, 1000], (V - 1, 1))
    H, _, hidx = R.build_system(poses, fixed, ef, ef + 1, meas, info)
    got, err = R.marginal_blocks_ref(H, hidx, np.arange(V))
    assert err.max() <= 1e-11
    for k in range(1, V):
        assert abs(got[k][0, 0] - k / 100.0) <= 1e-13 * k and abs(got[k][2, 2] - k / 1000.0) <= 1e-13 * k


@pytest.mark.parametrize("V,E,seed,gauge", [(60, 110, 3, 59), (300, 900, 4, 120)])
def test_label_edges_ut_matches_oracle_condense(oracle, V, E, seed, gauge):
    g = synth.make_pose_graph(V, E, seed=seed)
    a = C.args(g)
    p, _ = R.gn_optimize(g["poses"], g["fixed"], *a[2:], 6)
    query = np.unique(np.r_[np.linspace(0, V - 1, 9).astype(np.int32), gauge]).astype(np.int32)
    n, to, est, iu, cov = oracle.condense(p, *a[2:], gauge, query)
    ref = R.condense_ref(p, *a[2:], gauge, query, oracle.initial_guess)
    assert n == len(ref["to"]) and np.array_equal(to, ref["to"])
    assert not ref["not_pd"].any()
    # (est is the stepped poses: two correct solvers' steps differ by their forward error -- reference_cases.EST_ATOL)
    np.testing.assert_allclose(est, ref["est"], rtol=0, atol=EST_ATOL)
    for k in range(n):
        assert np.linalg.norm(cov[k] - ref["cov"][k]) <= 1e-9 * np.linalg.norm(ref["cov"][k])
        assert np.linalg.norm(iu[k] - ref["iu"][k]) <= 1e-8 * np.linalg.norm(ref["iu"][k])


def test_label_edges_ut_first_order_limit_and_not_pd(oracle):
    """tests/test_oracle_gn.py's first-order limit (a tiny Sigma: information ~ (J Sigma J^T)^-1), and a Sigma without a
    Cholesky factor: identity information, flagged."""
    xg = np.array([0.3, -0.2, 0.4])
    xv = np.array([2.0, 1.0, -0.7])
    A = np.array([[2.0, 0.3, 0.1], [0.3, 1.5, -0.2], [0.1, -0.2, 0.8]]) * 1e-8
    z, iu, bad = R.label_edges_ut(xg, xv[None], A[None])
    np.testing.assert_allclose(z[0], synth.se2_compose(synth.se2_inverse(xg[None]), xv[None])[0], atol=1e-12)
    _, _, Jj = oracle.edge_terms(xg, xv, z[0])
    want = np.linalg.inv(Jj @ A @ Jj.T)
    got = R.info_full(iu)[0]
    np.testing.assert_allclose(got, want, rtol=1e-4)
    st, m, iu_o = oracle.label_edge(xg, xv, A)
    assert st == 0 and not bad[0]
    np.testing.assert_allclose(m, z[0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(iu_o, iu[0], rtol=1e-9)
    neg = np.diag([1e-4, -1e-6, 1e-4])
    z, iu, bad = R.label_edges_ut(xg, xv[None], neg[None])
    st, _, iu_o = oracle.label_edge(xg, xv, neg)
    assert bad[0] and st == -1
    np.testing.assert_array_equal(iu[0], [1, 0, 0, 1, 0, 1])
    np.testing.assert_array_equal(iu_o, iu[0])
