"""The inter-robot pairwise-consistency entry points (cgmr_closure_consistency_inter[_exact]) as the header, the library and the
Python layers declare them, and the float64 reference (ref_pcm_inter.py) against finite differences, a hand-worked loop, the
single-graph reference on the union of the two graphs, and -- for every candidate set tests/test_pcm_inter_gpu.py holds the device
to -- what that set must show on the reference alone.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_backend as OB
import pcm_inter_cases as K
import ref_clique as RC
import ref_joint_marginals as J
import ref_pcm as P
import ref_pcm_inter as PI
from cg_mrslam_amd import _lib, mr_graph_slam
from cg_mrslam_amd.graph import GraphSLAM
from cg_mrslam_amd.mr_graph_slam import MRGraphSLAMDriver
from ref_condensed import RefRobotGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cgmr_closure_consistency_inter", "cgmr_closure_consistency_inter_exact"]
GAMMA = P.GAMMA_99


def _header():
    return open(os.path.join(ROOT, "include", "cgmr.h")).read()


def test_symbols_declared_listed_and_exported_version_105():
    lib = _lib.load_library()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    assert lib.cgmr_version() == 105


def test_null_context_and_the_new_invalid_arguments_are_invalid():
    """No context can exist without a device, and a missing one is refused before anything else is looked at: with each of
    the arguments the two calls refuse on their own (tests/test_pcm_inter_gpu.py: the same on a context, and the text), the
    answer is CGMR_E_INVALID and nothing is written."""
    lib = _lib.load_library()
    e_invalid = int(re.search(r"#define\s+CGMR_E_INVALID\s+\((-?\d+)\)", _header()).group(1))
    null = ctypes.c_void_p(0)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    poses, fixed = np.zeros((2, 3)), np.array([1, 0], dtype=np.uint8)
    ef, et = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    meas, info = np.array([[1.0, 0, 0]]), np.array([K.IU])
    graph = [null, ctypes.c_int(2), ptr(poses), ptr(fixed), ctypes.c_int(1), ptr(ef), ptr(et), ptr(meas), ptr(info)]
    ca, z, ci = np.array([1, 1], dtype=np.int32), np.zeros((2, 3)), np.tile(K.IU, (2, 1))
    good_pp, good_pc = np.zeros((2, 3)), np.eye(6)
    nan_pp, nan_pc, neg_pc = good_pp.copy(), good_pc.copy(), good_pc.copy()
    nan_pp[1, 2], nan_pc[4, 1], neg_pc[3, 3] = np.nan, np.inf, -1.0
    for pp, pc in ((good_pp, None), (nan_pp, None), (None, None), (good_pp, nan_pc), (good_pp, neg_pc)):
        d2 = np.full((2, 2), 7.0)
        size = np.full(1, 77, dtype=np.int32)
        cands = [ctypes.c_int(2), ptr(ca), null if pp is None else ptr(pp), null if pc is None else ptr(pc), ptr(z), ptr(ci),
                 ctypes.c_double(GAMMA), ptr(d2), null]
        clique = [ptr(np.zeros(2, dtype=np.int32)), ptr(size), ptr(np.zeros(1, dtype=np.int32))]
        assert lib.cgmr_closure_consistency_inter(*graph, *cands, *clique, null) == e_invalid
        assert lib.cgmr_closure_consistency_inter_exact(*graph, *cands, ctypes.c_int64(8), *clique, null) == e_invalid
        assert np.all(d2 == 7.0) and size[0] == 77


def test_python_layers_expose_the_calls_and_reject_a_malformed_check():
    for n in ("closure_consistency_inter", "closure_consistency_inter_exact"):
        assert callable(getattr(_lib.Context, n, None)), n
    assert callable(getattr(GraphSLAM, "interRobotConsistency", None)) and callable(mr_graph_slam.team_peer_covariance)
    octx = OB.OracleContext()
    make = lambda **kw: MRGraphSLAMDriver(octx, None, None, RefRobotGraph(octx, 0, 2), 0, 2, **kw)   # noqa: E731
    for bad in ("nonsense", "pcm", ("pcm",), ("pcm", 0.0), ("pcm", -1.0), ("vote", 9.0), ("pcm", 9.0, 1)):
        with pytest.raises(ValueError):
            make(mr_closure_check=bad)
    with pytest.raises(ValueError):
        make(mr_peer_covariance=np.eye(3))
    d = make()
    assert d.mr_closure_check == "voting" and d.mr_peer_covariance is None and d.closure_check == "voting"
    assert make(mr_closure_check=("pcm", 9.0)).mr_closure_check == ("pcm", 9.0)
    d = make(mr_closure_check=("pcm-exact", GAMMA), mr_peer_covariance=lambda r, v: None, closure_check=("pcm", 9.0))
    assert d.mr_closure_check == ("pcm-exact", GAMMA) and d.closure_check == ("pcm", 9.0)
    with pytest.raises(ValueError):
        _lib.Context._inter_arrays([0, 1], np.zeros((2, 3)), np.eye(3), np.zeros((2, 3)), np.zeros((2, 6)))


# ------------------------------------------------------------------------------------------- the reference's Jacobians
def _central(f, x, h=1e-6):
    """d f / d x by central differences, the angle's difference wrapped."""
    Jn = np.zeros((3, 3))
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        dd = f(x + d) - f(x - d)
        dd[2] = (dd[2] + np.pi) % (2 * np.pi) - np.pi
        Jn[:, k] = dd / (2 * h)
    return Jn


def test_reference_jacobians_match_central_differences():
    """20 random configurations; every fifth has one own vertex (a_k == a_l), every fifth (another) one peer vertex
    (p_k == p_l), every fifth (a third) both: a shared vertex is moved in both of its roles at once and the difference quotient
    is held against the sum of the roles' Jacobians.  The residual differentiated numerically is written out from its
    definition (loop_residual_inter), not the one the Jacobians are accumulated through.  Central difference: error
    h^2 |eps'''| / 6 ~ 1e-12 |x|, rounding u |eps| / h ~ 1e-9 (test_pcm_cpu.py's bar)."""
    rng = np.random.default_rng(12)
    for t in range(20):
        x = {n: rng.uniform(-3, 3, 3) for n in PI.INPUTS}
        shared = []
        if t % 5 in (1, 4):
            x["al"] = x["ak"]
            shared.append(("ak", "al"))
        if t % 5 in (3, 4):
            x["pl"] = x["pk"]
            shared.append(("pk", "pl"))
        moved = {n for pair in shared for n in pair}
        eps, jac = PI.loop_jacobians_inter(*(x[n] for n in PI.INPUTS))
        assert np.abs(eps - PI.loop_residual_inter(*(x[n] for n in PI.INPUTS))).max() <= 1e-14
        for n in PI.INPUTS:
            if n in moved:
                continue
            f = lambda v, n=n: PI.loop_residual_inter(*(v if m == n else x[m] for m in PI.INPUTS))   # noqa: E731
            assert np.abs(_central(f, x[n]) - jac[n]).max() <= 1e-8, (t, n)
        for pair in shared:
            f = lambda v, pair=pair: PI.loop_residual_inter(*(v if m in pair else x[m] for m in PI.INPUTS))   # noqa: E731
            assert np.abs(_central(f, x[pair[0]]) - (jac[pair[0]] + jac[pair[1]])).max() <= 1e-8, (t, pair)


# ------------------------------------------------------------------------------------------- the hand-worked loop
def test_reference_on_the_empty_loop():
    """Two candidates from one own vertex to one peer vertex: p_k^-1 p_l and x_al^-1 x_ak are the identity, and their Jacobians
    cancel vertex by vertex (d(x^-1 x) = 0), so neither covariance enters whatever it is: eps = z_k (+) z_l^-1.  With z_l = 0:
    eps = z_k, d eps / d z_k = I, d eps / d z_l = -R(theta_k), and with Omega_l = diag(a, a, b), which a rotation about z leaves
    alone, S = Omega_k^-1 + Omega_l^-1 and

        d2 = (z_k (-) z_l)^T (Omega_k^-1 + Omega_l^-1)^-1 (z_k (-) z_l)

    By hand: z_k = (0.1, 0, 0), both Omega = diag(500, 500, 5000): S_xx = 0.004, d2 = 0.01 / 0.004 = 2.5."""
    g = J.chain_graph()
    a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
    ca = np.array([3, 3], dtype=np.int32)
    pp = np.tile([4.0, -2.0, 1.1], (2, 1))
    z = np.array([[0.0, 0, 0], [0.1, 0, 0]])                         # l = 0, k = 1
    d2 = PI.consistency_dense_inter(*a, ca, pp, z, np.tile(K.IU, (2, 1)))
    assert abs(d2[1, 0] - 2.5) <= 1e-12 and d2[0, 1] == d2[1, 0] and d2[0, 0] == d2[1, 1] == 0
    # a correlated Omega_k, a rotation in z_k, and a peer covariance: the general formula, the peer covariance without effect
    rng = np.random.default_rng(5)
    M = rng.normal(0, 1, (3, 3))
    Ok = M @ M.T + 3 * np.eye(3)
    iu = np.array([K.IU, [Ok[0, 0], Ok[0, 1], Ok[0, 2], Ok[1, 1], Ok[1, 2], Ok[2, 2]]])
    z = np.array([[0.0, 0, 0], [0.1, -0.2, 0.05]])
    want = float(z[1] @ np.linalg.solve(np.linalg.inv(Ok) + np.diag(1 / K.IU[[0, 3, 5]]), z[1]))
    Cp = rng.normal(0, 1, (3, 3))
    for pc in (None, np.tile(Cp @ Cp.T, (2, 2))):
        d2 = PI.consistency_dense_inter(*a, ca, pp, z, iu, pc)
        assert abs(d2[1, 0] - want) <= 1e-12 * want, (d2, want)
    # equal measurements: eps = z (+) z^-1, zero to rounding (|eps| <= 1e-15, S >= 0.0004); an indefinite information: NaN, and
    # NaN is not adjacent
    assert np.all(PI.consistency_dense_inter(*a, ca, pp, np.tile(z[1], (2, 1)), np.tile(K.IU, (2, 1))) <= 3 * 1e-30 / 0.0004)
    bad = np.array([K.IU, [-1e-6, 0, 0, 1.0, 0, 1.0]])
    d2 = PI.consistency_dense_inter(*a, ca, pp, z, bad)
    assert np.isnan(d2[1, 0]) and not P.adjacency(d2).any()


# ------------------------------------------------------------------------------------------- the candidate sets of the GPU tests
_REF = {}


def _reference(seed, with_cov):
    if (seed, with_cov) not in _REF:
        own, p_own, peer, p_peer = K.graphs()
        ca, pv, z, ci, out = K.candidates(p_own, p_peer, seed)
        _REF[(seed, with_cov)] = PI.consistency_dense_inter(p_own, *K.args(own), ca, p_peer[pv], z, ci,
                                                            K.peer_cov_dense(seed) if with_cov else None)
    return _REF[(seed, with_cov)]


@pytest.mark.parametrize("with_cov", [True, False])
@pytest.mark.parametrize("seed", K.SEEDS)
def test_gpu_candidate_sets_on_the_reference_alone(seed, with_cov):
    """What every end-to-end set must show before a device is asked: the greedy clique is the planted inlier set, ref_clique
    proves it a maximum one, and no d2 lies within 10 % of gamma -- with the peer graph's covariance and without any."""
    own, p_own, peer, p_peer = K.graphs()
    ca, pv, z, ci, out = K.candidates(p_own, p_peer, seed)
    N = len(ca)
    inl = sorted(set(range(N)) - set(out.tolist()))
    d2 = _reference(seed, with_cov)
    A = P.adjacency(d2, GAMMA)
    clique, size, _ = P.greedy_clique(A)
    assert len(inl) == 26 and clique == inl and size == 26
    omega, _ = RC.omega(A)
    assert omega == 26 and RC.is_clique(A, clique)
    off = ~np.eye(N, dtype=bool)
    is_out = np.zeros(N, dtype=bool)
    is_out[out] = True
    with_out = (is_out[:, None] | is_out[None, :]) & off
    near = np.min(np.abs(d2[off] - GAMMA)) / GAMMA
    print(f"generator {seed}, peer_cov {'given' if with_cov else 'None'}: smallest d2 with an outlier {d2[with_out].min():.1f}, "
          f"largest among the inliers {d2[~with_out & off].max():.1f}, nearest to gamma {near:.0%} away")
    assert near > 0.10
    assert len(set(ca.tolist())) < N and len(set(pv.tolist())) < N            # (own and peer vertices repeat)


@pytest.mark.parametrize("seed", K.SEEDS[:1])
def test_reference_equals_the_single_graph_reference_on_the_union(seed):
    """The two graphs as the components of one: its joint covariance is block diagonal, so ref_pcm's single-graph d2 with the
    peer's vertices as b is the two-graph d2 with the peer's own covariance.  Two dense inverses, one of H and one of its
    blocks: 1e-9 of max(d2, 1)."""
    own, p_own, peer, p_peer = K.graphs()
    ca, pv, z, ci, out = K.candidates(p_own, p_peer, seed)
    pu = np.vstack([p_own, p_peer])
    one = P.consistency_dense(pu, *K.union(own, peer), ca, (pv + len(p_own)).astype(np.int32), z, ci)
    two = _reference(seed, True)
    assert np.max(np.abs(one - two) / np.maximum(one, 1)) <= 1e-9
