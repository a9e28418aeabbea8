"""Joint-compatibility data association (cgmr_jcbb_dense, cgmr_joint_compatibility, GraphSLAM.associateObservations) on the
GPU against the float64 reference of tests/ref_jcbb.py on the cases of tests/jcbb_cases.py.  The dense form's d2 is held to
jcbb_cases.D2_BAR; the graph form, whose Sigma is the device's own, to the typed tests' MARG_TAU rule and to AGREE_TAU against
cgmr_observation_covariance."""
import numpy as np
import pytest

import assoc_cases as AC
import jcbb_cases as JC
import ref_jcbb as RJ
from cg_mrslam_amd._lib import JC_DEFAULT_NODE_LIMIT, JC_MAX_LANDMARKS, JC_MAX_OBS, JC_ROUNDS, CgmrError

pytestmark = pytest.mark.gpu
E_INVALID = -1


def _dense(ctx, P, **kw):
    return ctx.jcbb_dense(P["slot"], P["dim"], P["sigma"], P["e"], P["J"], P["R"], P["gamma"], **kw)


def _dense_twice(ctx, P, **kw):
    a, b = _dense(ctx, P, **kw), _dense(ctx, P, **kw)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))
    return a


def _no_worse(a, b):
    """(count, d2) a is no worse than b"""
    return not RJ._better(b, a)


# --------------------------------------------------------------------------------------- 1. the dense form
@pytest.mark.parametrize("name", list(JC.CASES))
def test_dense_against_reference(ctx, name):
    P = JC.case(name)
    want, run = P["answer"], P["run"]
    assign, count, d2, dof, proven, ic, nodes = _dense_twice(ctx, P)
    h = assign.tolist()
    ok, d2_ref, dof_ref = RJ.admissible(P, h)
    ref_ic = RJ.individual(P)
    print(f"{name}: count {count} (reference {want[1]}), d2 {d2:.17g} (reference of the same hypothesis {d2_ref:.17g}, of its own "
          f"{want[2]:.17g}), dof {dof}, nodes {nodes}, proven {proven}; margin {run.margin:.3g}, gap {run.gap:.3g}")
    assert count == want[1] == sum(1 for j in h if j >= 0)
    assert ok and dof == dof_ref == want[3]
    assert abs(d2 - d2_ref) <= JC.D2_BAR * d2_ref
    assert d2_ref <= want[2] * (1 + JC.D2_BAR)                      # the smallest d2 among the hypotheses of that count
    if run.gap >= JC.GAP_MIN:
        assert h == want[0]
    assert proven is True
    assert np.array_equal(np.isnan(ic), np.isnan(ref_ic))
    fin = np.isfinite(ref_ic)
    assert np.all(np.abs(ic[fin] - ref_ic[fin]) <= JC.D2_BAR * ref_ic[fin])
    roots = int(np.sum(ref_ic < P["gamma"][P["dim"]][:, None]))
    assert roots <= nodes <= roots * JC_ROUNDS * JC_DEFAULT_NODE_LIMIT or roots == nodes == 0


def test_crossed_beats_the_greedy_hypothesis(ctx):
    P = JC.case("crossed")
    assign, count, d2, dof, proven, _, _ = _dense(ctx, P)
    assert P["greedy"][0] == [1, -1] and assign.tolist() == [0, 1] and (count, dof, proven) == (2, 4, True)


# --------------------------------------------------------------------------------------- 2. the node limit
def test_node_limit_stops_the_search_and_keeps_an_admissible_hypothesis(ctx):
    """The ambiguous row.  One test per root is the root's own: every root that wants a second one is stopped, at no cost in
    time (the limit ends a search early; it never lets a kernel run on)."""
    P = JC.case("row")
    g = (P["greedy"][1], P["greedy"][2])
    roots = int(np.sum(RJ.individual(P) < P["gamma"][2]))
    prev = None
    for limit in (1, 2, 8, 64, JC_DEFAULT_NODE_LIMIT):
        assign, count, d2, dof, proven, _, nodes = _dense_twice(ctx, P, node_limit=limit)
        ok, d2_ref, _ = RJ.admissible(P, assign.tolist())
        print(f"node_limit {limit}: count {count}, d2 {d2:.12g}, proven {proven}, nodes {nodes} of at most {roots * JC_ROUNDS * limit}")
        assert ok and abs(d2 - d2_ref) <= JC.D2_BAR * d2_ref
        assert _no_worse((count, d2), (g[0], g[1] * (1 + JC.D2_BAR)))
        assert roots <= nodes <= roots * JC_ROUNDS * limit
        if limit == 1:
            assert proven is False
        if prev is not None:
            assert _no_worse((count, d2), prev)                     # raising the limit never worsens the result
        prev = (count, d2)
    assert proven is True and assign.tolist() == P["answer"][0]


# --------------------------------------------------------------------------------------- 3. the graph form
_OPT = {}


def _optimised(ctx, name):
    if name not in _OPT:
        g = AC.case(name)
        rc, p, _ = ctx.gn_optimize_typed(*AC.args(g), 3, vertex_kind=g["vk"], edge_kind=g["ek"])
        assert rc == 0
        _OPT[name] = (g, p, JC.graph_scene(g))
    return _OPT[name]


def _kw(g):
    return dict(vertex_kind=g["vk"], edge_kind=g["ek"])


def _marg_bound(P, h):
    """The typed tests' MARG_TAU rule (tests/test_assoc_gpu.py::test_observation_covariance) for the d2 of a hypothesis:
    MARG_TAU (||J||^2 ||Sigma|| ||C^-1 e||^2 + cond(C) d2), Sigma the covariance of the state entries the hypothesis touches."""
    e, C = RJ.joint(P, h)
    ix = sorted({k for i, j in enumerate(h) if j >= 0 for k in RJ.state_idx(P, i, j)})
    jn2 = sum(float(np.sum(P["J"][i, j, :P["dim"][i]] ** 2)) for i, j in enumerate(h) if j >= 0)
    y2 = float(np.linalg.norm(np.linalg.solve(C, e)) ** 2)
    return AC.MARG_TAU * (jn2 * np.linalg.norm(P["sigma"][np.ix_(ix, ix)]) * y2 + np.linalg.cond(C) * RJ.d2_chol(e, C))


@pytest.mark.parametrize("name", ["mixed5_256", "tree600b"])
def test_graph_form_against_reference(ctx, name):
    g, p, sc = _optimised(ctx, name)
    a = (p,) + AC.args(g)[1:]
    M, lms = len(sc["kinds"]), sc["lms"]
    op = np.full(M, sc["pose"], np.int32)
    pa, pb = np.repeat(op, len(lms)), np.tile(lms, M)
    gate = (pa, pb, np.repeat(sc["kinds"], len(lms)), np.repeat(sc["meas"], len(lms), axis=0), np.repeat(sc["info"], len(lms), axis=0))
    before = ctx.observation_covariance(*a, *gate, **_kw(g))
    got = ctx.joint_compatibility(*a, op, sc["kinds"], sc["meas"], sc["info"], lms, **_kw(g))
    again = ctx.joint_compatibility(*a, op, sc["kinds"], sc["meas"], sc["info"], lms, **_kw(g))
    after = ctx.observation_covariance(*a, *gate, **_kw(g))
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, again))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    assign, count, d2, dof, proven, ic, nodes = got
    # the reference on its own Sigma
    P, err = RJ.graph_problem(g, p, op, sc["kinds"], sc["meas"], sc["info"], lms, JC.GAMMA)
    run = RJ.Run()
    want = RJ.jcbb(P, run)
    assert err <= AC.REF_ERR_MAX and run.margin >= JC.MARGIN_MIN, (err, run.margin)
    pos = {int(v): j for j, v in enumerate(lms)}
    h = [pos[int(v)] if v >= 0 else -1 for v in assign]
    ok, d2_ref, dof_ref = RJ.admissible(P, h)
    print(f"{name}: pose {sc['pose']}, assign {assign.tolist()} (reference {[int(lms[j]) if j >= 0 else -1 for j in want[0]]}), d2 {d2:.15g} "
          f"(reference {d2_ref:.15g}), nodes {nodes}; margin {run.margin:.3g}, gap {run.gap:.3g}, reference Sigma error {err:.2g}")
    assert ok and count == want[1] and dof == dof_ref == want[3] and proven is True
    assert abs(d2 - d2_ref) <= _marg_bound(P, h)
    if run.gap >= JC.GAP_MIN:
        assert h == want[0]
    assert count == 6 and assign[-1] == -1 and sc["kinds"][5] == 2 and assign[5] >= 0      # a bearing paired, the spurious one not
    # ic: the reference's, by the same rule; and cgmr_observation_covariance's own d2 on the same pairs
    ref_ic = RJ.individual(P)
    for i in range(M):
        for j in range(len(lms)):
            one = [-1] * M
            one[i] = j
            assert abs(ic[i, j] - ref_ic[i, j]) <= _marg_bound(P, one), (i, j, ic[i, j], ref_ic[i, j])
    listed = before[2].reshape(M, len(lms))
    assert np.all(np.isfinite(listed)) and np.all(np.abs(ic - listed) <= AC.AGREE_TAU * listed)


# --------------------------------------------------------------------------------------- 4. the wrappers
def test_wrappers(ctx):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g, p, sc = _optimised(ctx, "mixed5_256")
    a = (p,) + AC.args(g)[1:]
    s = GraphSLAM(PoseGraph(np.arange(len(p)), p, g["fixed"], *AC.args(g)[2:], vertex_kind=g["vk"], edge_kind=g["ek"]), ctx)
    M, lms, kinds = len(sc["kinds"]), sc["lms"], sc["kinds"]
    z = sc["meas"][:, :2]
    info = sc["info"][:, [0, 1, 3]]
    gate_before = s.gateObservations(sc["pose"], lms, z[kinds == 1], info[kinds == 1], kind=1)
    want = ctx.joint_compatibility(*a, np.full(M, sc["pose"], np.int32), kinds, sc["meas"], sc["info"], lms, **_kw(g))
    assign, d2, dof, proven = s.associateObservations(sc["pose"], lms, z, info, kind=kinds)
    assert assign.tobytes() == want[0].tobytes() and (d2, dof, proven) == (want[2], want[3], want[4])
    # one kind for all: the xy measurements alone, then the bearing alone
    xy = s.associateObservations(sc["pose"], lms, z[kinds == 1], info[kinds == 1])
    assert xy[0].tolist() == assign[kinds == 1].tolist() and xy[2] == 2 * 5
    b = s.associateObservations(sc["pose"], lms, z[kinds == 2, 0], info[kinds == 2, 0], kind=2)
    assert b[0].tolist() == assign[kinds == 2].tolist() and b[2] == 1
    nE = s.graph.n_edges
    edges = s.addAssociatedObservations(sc["pose"], lms, z, info, kind=kinds)
    paired = np.flatnonzero(assign >= 0)
    assert edges == list(range(nE, nE + len(paired))) and s.graph.n_edges == nE + len(paired)
    vk, ek = s.graph.kinds()
    for e, m in zip(edges, paired):
        assert int(s.graph.edge_from[e]) == sc["pose"] and int(s.graph.edge_to[e]) == int(assign[m]) and int(ek[e]) == int(kinds[m])
        assert s.graph.meas[e, 0] == sc["meas"][m, 0] and s.graph.info[e, 0] == sc["info"][m, 0]
    # gateObservations is what it was: the graph before the new edges gives the same bytes through the context
    n = int(np.sum(kinds == 1)) * len(lms)
    listed = ctx.observation_covariance(*a, np.full(n, sc["pose"], np.int32), np.tile(lms, n // len(lms)), np.full(n, 1, np.uint8),
                                        np.repeat(sc["meas"][kinds == 1], len(lms), axis=0), np.repeat(sc["info"][kinds == 1], len(lms), axis=0),
                                        **_kw(g))[2]
    assert gate_before.tobytes() == listed.reshape(-1, len(lms)).tobytes()


# --------------------------------------------------------------------------------------- 5. refusals
def _launches(ctx):
    return sum(n for _, n in ctx.gn_kernel_times().values())


def test_refusals(ctx):
    P = JC.case("two_poses")
    good = dict(obs_pose_slot=P["slot"], obs_dim=P["dim"], sigma=P["sigma"], e=P["e"], J=P["J"], R_upper=P["R"], gamma_by_dof=P["gamma"])

    def bad_dense(**kw):
        with pytest.raises(CgmrError) as ei:
            ctx.jcbb_dense(**dict(good, **kw))
        assert ei.value.code == E_INVALID and "cgmr_jcbb_dense" in str(ei.value), str(ei.value)
        return str(ei.value)

    bad_dense(node_limit=0)
    bad_dense(node_limit=-3)
    assert "observation 2 " in bad_dense(obs_dim=[2, 2, 3, 2, 2])
    assert "observation 1 " in bad_dense(obs_dim=[2, 0, 1, 2, 2])
    assert "observation 3 " in bad_dense(obs_pose_slot=[0, 1, 0, 2, 1])
    g2 = P["gamma"].copy()
    g2[4] = g2[3]
    assert "gamma_by_dof[4]" in bad_dense(gamma_by_dof=g2)
    g2[4] = np.inf
    assert "gamma_by_dof[4]" in bad_dense(gamma_by_dof=g2)
    s2 = P["sigma"].copy()
    s2[7, 2] = np.nan
    assert "landmark 0" in bad_dense(sigma=s2)
    big = JC_MAX_OBS + 1
    with pytest.raises(CgmrError) as ei:
        ctx.jcbb_dense(np.zeros(big, np.int32), np.full(big, 1, np.int32), np.eye(5), np.zeros((big, 1, 2)), np.zeros((big, 1, 2, 5)),
                       np.ones((big, 3)), np.arange(2 * big + 1.0))
    assert ei.value.code == E_INVALID and "CGMR_JC_MAX_OBS" in str(ei.value)
    big = JC_MAX_LANDMARKS + 1
    with pytest.raises(CgmrError) as ei:
        ctx.jcbb_dense([0], [1], np.eye(3 + 2 * big), np.zeros((1, big, 2)), np.zeros((1, big, 2, 5)), np.ones((1, 3)), [0.0, 1.0, 2.0])
    assert ei.value.code == E_INVALID and "CGMR_JC_MAX_LANDMARKS" in str(ei.value)
    # nothing to pair: CGMR_OK, count 0, proven
    none = ctx.jcbb_dense(P["slot"], P["dim"], P["sigma"][:6, :6], np.zeros((5, 0, 2)), np.zeros((5, 0, 2, 5)), P["R"], P["gamma"])
    assert none[0].tolist() == [-1] * 5 and none[1:5] == (0, 0.0, 0, True)
    none = ctx.jcbb_dense([], [], np.zeros((0, 0)), np.zeros((0, 0, 2)), np.zeros((0, 0, 2, 5)), np.zeros((0, 3)), [0.0])
    assert len(none[0]) == 0 and none[1:5] == (0, 0.0, 0, True)

    g, p, sc = _optimised(ctx, "mixed5_256")
    a = (p,) + AC.args(g)[1:]
    M, lms = len(sc["kinds"]), sc["lms"]
    pose_v, point_v = int(g["P"][3]), int(g["L"][0])
    ok = dict(obs_pose=np.full(M, sc["pose"], np.int32), obs_kind=sc["kinds"], obs_meas=sc["meas"], obs_info=sc["info"], landmarks=lms)

    def bad_graph(kinds=True, **kw):
        with pytest.raises(CgmrError) as ei:
            ctx.joint_compatibility(*a, **dict(ok, **kw), **(_kw(g) if kinds else {}))
        assert ei.value.code == E_INVALID and "cgmr_joint_compatibility" in str(ei.value), str(ei.value)
        return str(ei.value)

    ctx.set_profiling(True)                                         # (counts the launches of every pass from here on)
    try:
        assert _launches(ctx) == 0
        bad_graph(node_limit=0)
        k2 = sc["kinds"].copy()
        k2[4] = 0
        assert "observation 4 " in bad_graph(obs_kind=k2)
        k2[4] = 3
        assert "observation 4 " in bad_graph(obs_kind=k2)
        o2 = ok["obs_pose"].copy()
        o2[2] = point_v
        assert "observation 2 " in bad_graph(obs_pose=o2) and "a point" in bad_graph(obs_pose=o2)
        l2 = lms.copy()
        l2[3] = pose_v
        assert "landmark 3 " in bad_graph(landmarks=l2) and "a pose" in bad_graph(landmarks=l2)
        l2[3] = lms[1]
        assert "landmark 3 " in bad_graph(landmarks=l2) and "repeats" in bad_graph(landmarks=l2)
        l2[3] = len(p)
        assert "landmark 3 " in bad_graph(landmarks=l2)
        assert "landmark 0 " in bad_graph(kinds=False)             # without types every vertex is a pose
        g2 = JC.GAMMA.copy()
        g2[2] = g2[1]
        assert "gamma_by_dof[2]" in bad_graph(gamma_by_dof=g2)
        many = np.tile(lms, 40)[:JC_MAX_LANDMARKS + 1]
        assert "CGMR_JC_MAX_LANDMARKS" in bad_graph(landmarks=many)
        assert "CGMR_JC_MAX_OBS" in bad_graph(obs_pose=np.full(33, sc["pose"], np.int32), obs_kind=np.ones(33, np.uint8),
                                              obs_meas=np.zeros((33, 3)), obs_info=None, gamma_by_dof=np.arange(67.0))
        assert _launches(ctx) == 0                                  # nothing was queued
        none = ctx.joint_compatibility(*a, **dict(ok, landmarks=np.zeros(0, np.int32)), **_kw(g))
        assert none[0].tolist() == [-1] * M and none[1:5] == (0, 0.0, 0, True) and _launches(ctx) == 0
        # the context works afterwards, and now something is queued
        got = ctx.joint_compatibility(*a, **ok, **_kw(g))
        assert got[1] == 6 and _launches(ctx) > 0
    finally:
        ctx.set_profiling(False)
