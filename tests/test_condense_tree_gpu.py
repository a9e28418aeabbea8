"""cgmr_condense_tree on the device against the float64 reference (tests/ref_condense_tree.py) on the cases
tests/test_condense_tree_cpu.py has proved: the chain's known answers, the four loop graphs (the tree exactly -- the
reference's decision margin makes that fair --, the labels and weights at MARG_TAU and, on the device's own blocks, the
arithmetic at 1e-12), KL(tree) < KL(star) for the device's own edges, the gauge's edges against cgmr_condense, the shapes that
straddle the 16-column tiles and the 64x64 macro-tiles, robust kernels, limits and determinism.

Measured on an MI355X (the largest over the four loop cases): est against the reference 3.7e-11 m, weights 5.5e-14 of their
scale and information 4.4e-11 of its norm (bar MARG_TAU); on the device's own blocks weights 3.9e-17 and information 5.3e-13
(bar 1e-12: the 13-point labels of the 200/400 case with 16 requested, 3.5e-14 or less on the other three); the chain's
information against the closed form 2.479e-4 / 5.542e-5 / 1.497e-2, the reference's own figures; KL tree / star 1.31 / 42.56,
5.38 / 70.02, 3.78 / 65.56, 0.097 / 13.47 nats; Cauchy against the scaled information 4.6e-13."""
import numpy as np
import pytest

import condense_tree_cases as CC
import ref_condense_tree as T
import ref_joint_marginals as J
import ref_robust as RR
import ref_robust_marginals as RM
from cg_mrslam_amd import Context, synth
from cg_mrslam_amd._lib import TREE_MAX_NODES, CgmrError
from condense_tree_cases import UT_GAP, UT_MARGIN
from condense_tree_cases import info_full as _full
from reference_cases import EST_ATOL

pytestmark = pytest.mark.gpu

MARG_TAU = 1e-9                 # test_joint_marginals_gpu.py: blocks against the refined reference
AGREE_TAU = 1e-9                # two paths on the same factor
ARITH_TAU = 1e-12               # the device's arithmetic against numpy's on the same blocks (test_relative_covariance_arithmetic)
E_INVALID = -1


def _a(g):
    return g["edge_from"], g["edge_to"], g["meas"], g["info"]


def _parents(fr, to):
    return {int(t): int(f) for f, t in zip(fr, to)}


# --------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("name", [c[0] for c in CC.CHAINS])
def test_chain_known_answers(ctx, name):
    _, mk, gauge, q = next(c for c in CC.CHAINS if c[0] == name)
    g = mk()
    fr, to, est, iu, w, fl = ctx.condense_tree(g["poses"], *_a(g), gauge, q)
    assert _parents(fr, to) == CC.chain_parent_vertices(gauge, q)
    assert np.array_equal(to, T.nodes_of(gauge, q)[1:]) and not fl.any() and np.all(np.isfinite(w))
    assert np.abs(est - np.c_[to - fr, np.zeros((len(to), 2))]).max() <= 1e-9
    gap = max(np.linalg.norm(_full(i) - CC.chain_edge_information(f, t)) / np.linalg.norm(CC.chain_edge_information(f, t))
              for f, t, i in zip(fr, to, iu))
    print(f"{name}: device information against the closed form {gap:.3e} of its norm (bar {UT_MARGIN * UT_GAP[name]:.2e})")
    assert gap <= UT_MARGIN * UT_GAP[name]


# --------------------------------------------------------------------------------------- the loop cases
_DEV = {}


def _device(ctx, name):
    """The device's edges on a loop case, and what its own arithmetic started from: the joint blocks cgmr_marginals_joint
    returns at the guess with the gauge fixed and the poses after the device's own step.  Computed once and shared."""
    if name not in _DEV:
        g, gauge, q = CC.loop_case(name)
        ref = CC.loop_reference(name)
        out = ctx.condense_tree(g["poses"], *_a(g), gauge, q)
        fixed = np.zeros(len(g["poses"]), np.uint8)
        fixed[gauge] = 1
        S = ctx.marginals_joint(ref["guess"], fixed, *_a(g), ref["nodes"][1:])
        rc, p1, _ = ctx.gn_optimize(ref["guess"], fixed, *_a(g), 1)
        assert rc == 0
        _DEV[name] = (out, S, p1)
    return _DEV[name]


@pytest.mark.parametrize("name", [c[0] for c in CC.LOOPS])
def test_loop_case_against_the_reference(ctx, name):
    ref = CC.loop_reference(name)
    (fr, to, est, iu, w, fl), _, _ = _device(ctx, name)
    nodes, tree = ref["nodes"], ref["tree"]
    assert np.array_equal(to, tree["to"]) and np.array_equal(fr, tree["fr"]) and not fl.any()
    d_est = np.abs(est - tree["est"]).max()
    assert d_est <= EST_ATOL
    worst_w = worst_i = 0.0
    p1 = ref["poses1"]
    for k in range(1, len(nodes)):
        p = int(ref["parent"][k])
        a, b = min(p, k), max(p, k)
        Sz = ref["Sz"][a, b]
        scale = J.relative_cov_scale(p1[nodes[a]], p1[nodes[b]], T.node_block(ref["Sigma"], a, a), T.node_block(ref["Sigma"], a, b),
                                     T.node_block(ref["Sigma"], b, b)) * np.linalg.norm(np.linalg.inv(Sz))
        e_w = abs(w[k - 1] - ref["weight"][k - 1]) / scale
        e_i = np.linalg.norm(iu[k - 1] - tree["iu"][k - 1]) / np.linalg.norm(tree["iu"][k - 1])
        worst_w, worst_i = max(worst_w, e_w), max(worst_i, e_i)
    print(f"{name}: est {d_est:.2e} m, weight {worst_w:.2e} of its scale, information {worst_i:.2e} of its norm (bar {MARG_TAU:.0e})")
    assert worst_w <= MARG_TAU and worst_i <= MARG_TAU


@pytest.mark.parametrize("name", [c[0] for c in CC.LOOPS])
def test_loop_case_arithmetic_on_the_devices_own_blocks(ctx, name):
    """The numpy weight and label formulas on the blocks cgmr_marginals_joint returns at the guess with the gauge fixed and at
    the poses of the device's own step: the solvers' forward errors drop out, what is left is the kernels' arithmetic."""
    ref = CC.loop_reference(name)
    (fr, to, est, iu, w, fl), S, p1 = _device(ctx, name)
    nodes = ref["nodes"]
    W, Szs = T.weights(p1, nodes, S)
    parent = np.r_[-1, [int(np.flatnonzero(nodes == f)[0]) for f in fr]]
    own = T.edges_of(ref, parent, Sigma=S, poses=p1)
    assert np.abs(est - own["est"]).max() <= 1e-12
    worst_w = worst_i = 0.0
    for k in range(1, len(nodes)):
        p = int(parent[k])
        a, b = min(p, k), max(p, k)
        scale = J.relative_cov_scale(p1[nodes[a]], p1[nodes[b]], T.node_block(S, a, a), T.node_block(S, a, b), T.node_block(S, b, b)) \
            * np.linalg.norm(np.linalg.inv(Szs[a, b]))
        worst_w = max(worst_w, abs(w[k - 1] - W[a, b]) / scale)
        worst_i = max(worst_i, np.linalg.norm(iu[k - 1] - own["iu"][k - 1]) / np.linalg.norm(own["iu"][k - 1]))
    print(f"{name}: on the device's own blocks, weight {worst_w:.2e} of its scale, information {worst_i:.2e} of its norm (bar {ARITH_TAU:.0e})")
    assert worst_w <= ARITH_TAU and worst_i <= ARITH_TAU
    # the tree the device chose is the tree of its own weights
    assert np.array_equal(T.kruskal(W), parent)


@pytest.mark.parametrize("name", [c[0] for c in CC.LOOPS])
def test_device_tree_is_closer_to_the_joint_marginal_than_the_device_star(ctx, name):
    g, gauge, q = CC.loop_case(name)
    ref = CC.loop_reference(name)
    (fr, to, est, iu, w, fl), _, _ = _device(ctx, name)
    s_to, s_est, s_iu, _ = ctx.condense(g["poses"], *_a(g), gauge, q)
    assert np.array_equal(s_to, to)
    kl_tree = T.kl_of_edges(ref, dict(fr=fr, to=to, est=est, iu=iu))
    kl_star = T.kl_of_edges(ref, dict(fr=np.full(len(s_to), gauge), to=s_to, est=s_est, iu=s_iu))
    print(f"{name}: KL against the reference's joint covariance, device tree {kl_tree:.3f}, device star {kl_star:.3f} nats")
    assert kl_tree < kl_star
    # an edge whose parent is the gauge is the star's edge for that vertex: two Gram layouts over one factor
    at_gauge = np.flatnonzero(fr == gauge)
    assert len(at_gauge) >= 1
    for k in at_gauge:
        assert np.abs(est[k] - s_est[k]).max() <= AGREE_TAU
        assert np.linalg.norm(iu[k] - s_iu[k]) <= AGREE_TAU * np.linalg.norm(s_iu[k])


# --------------------------------------------------------------------------------------- shapes
_G400 = {}


def _g400():
    if not _G400:
        _G400["g"] = synth.make_pose_graph(400, 1000, seed=23)
    return _G400["g"]


def _check_shape(ctx, g, gauge, q):
    """The edge count and the `to` order are cgmr_condense's with duplicates dropped; the edges are a tree on the nodes rooted at
    the gauge; the weights are those numpy gives on the device's own blocks, and the tree is the tree of those weights
    wherever the next-best swap is not within rounding of them."""
    fr, to, est, iu, w, fl = ctx.condense_tree(g["poses"], *_a(g), gauge, q)
    s_to = ctx.condense(g["poses"], *_a(g), gauge, q)[0]
    _, first = np.unique(s_to, return_index=True)
    want_to = s_to[np.sort(first)]
    assert np.array_equal(to, want_to) and len(fr) == len(to) == len(est) == len(iu) == len(w) == len(fl)
    nodes = T.nodes_of(gauge, q)
    assert np.array_equal(nodes[1:], to)
    par = _parents(fr, to)
    for v in to:                                                  # every node reaches the gauge
        seen = 0
        while v != gauge:
            v = par[int(v)]
            seen += 1
            assert seen <= len(to)
    assert not fl.any() and np.all(np.isfinite(w)) and np.all(np.isfinite(iu))
    return fr, to, est, iu, w, fl


def test_no_query_one_query_and_the_gauge_alone(ctx):
    g = _g400()
    for q in ([], [7], [7, 7, 7]):
        out = ctx.condense_tree(g["poses"], *_a(g), 7, q)
        assert all(len(x) == 0 for x in out)
    fr, to, est, iu, w, fl = _check_shape(ctx, g, 7, [200])
    assert list(fr) == [7] and list(to) == [200]
    s_to, s_est, s_iu, _ = ctx.condense(g["poses"], *_a(g), 7, [200])
    assert np.abs(est - s_est).max() <= AGREE_TAU and np.linalg.norm(iu - s_iu) <= AGREE_TAU * np.linalg.norm(s_iu)


@pytest.mark.parametrize("nq", [3, 4, 5, 16, 17, 33, 65, 300])
def test_query_counts_across_tiles_and_macro_tiles(ctx, nq):
    g = _g400()
    rng = np.random.default_rng(nq)
    q = rng.permutation(400)[:nq + 1].astype(np.int32)
    gauge, q = int(q[0]), q[1:]
    fr, to, est, iu, w, fl = _check_shape(ctx, g, gauge, q)       # the gauge outside the list
    assert len(to) == nq
    # the gauge inside the list and duplicated queries: the same nodes, the same bytes
    q2 = np.r_[q[:2], gauge, q[2:], q[::3], gauge].astype(np.int32)
    out2 = _check_shape(ctx, g, gauge, q2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((fr, to, est, iu, w, fl), out2))
    # the weights of the chosen edges on the device's own blocks, and the tree of those weights
    fixed = np.zeros(400, np.uint8)
    fixed[gauge] = 1
    guess = RM.guess_bfs(g["poses"], fixed, g["edge_from"], g["edge_to"], g["meas"])
    S = ctx.marginals_joint(guess, fixed, *_a(g), to)
    rc, p1, _ = ctx.gn_optimize(guess, fixed, *_a(g), 1)
    assert rc == 0
    nodes = T.nodes_of(gauge, q)
    W, Szs = T.weights(p1, nodes, S)
    idx = {int(v): k for k, v in enumerate(nodes)}
    parent = np.r_[-1, [idx[int(f)] for f in fr]]
    worst = 0.0
    for k in range(1, len(nodes)):
        a, b = min(int(parent[k]), k), max(int(parent[k]), k)
        scale = J.relative_cov_scale(p1[nodes[a]], p1[nodes[b]], T.node_block(S, a, a), T.node_block(S, a, b), T.node_block(S, b, b)) \
            * np.linalg.norm(np.linalg.inv(Szs[a, b]))
        worst = max(worst, abs(w[k - 1] - W[a, b]) / scale)
    want = T.kruskal(W)
    # the exact comparison of trees below runs for nq = 3 .. 65 (margins measured: 0.15 down to 1.1e-3 nats, all above
    # MARGIN_MIN); at nq = 300 the margin is not taken (n^2 tree paths) and the tree is held to the minimum total weight alone --
    # the tree rule itself is checked byte for byte, up to n = 1025, in test_min_spanning_tree_gpu.py
    margin = T.decision_margin(W, want) if nq <= 65 else None
    print(f"nq {nq}: weights on the device's own blocks {worst:.2e} of their scale; decision margin of numpy's tree {margin}")
    assert worst <= ARITH_TAU
    if margin is not None and margin >= CC.MARGIN_MIN:
        assert np.array_equal(parent, want)
    total = sum(W[k, parent[k]] for k in range(1, len(nodes)))
    assert abs(total - sum(W[k, want[k]] for k in range(1, len(nodes)))) <= 1e-9 * len(nodes)     # a minimum tree either way


def test_a_requested_vertex_no_edge_touches_hangs_on_the_gauge_unlabelled(ctx):
    g, gauge, q, iso = CC.isolated_case()
    ref = T.condense_tree(g["poses"], *_a(g), gauge, q, refined=True)["tree"]
    fr, to, est, iu, w, fl = ctx.condense_tree(g["poses"], *_a(g), gauge, q)
    assert np.array_equal(fr, ref["fr"]) and np.array_equal(to, ref["to"]) and np.array_equal(fl, ref["flags"])
    k = int(np.flatnonzero(to == iso)[0])
    assert fr[k] == gauge and fl[k] == 2 and np.isinf(w[k]) and list(iu[k]) == [1, 0, 0, 1, 0, 1] and fl.sum() == 2
    assert np.abs(est - ref["est"]).max() <= EST_ATOL
    assert max(np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(iu, ref["iu"])) <= MARG_TAU


# --------------------------------------------------------------------------------------- robust kernels
def test_robust_none_is_the_plain_call_and_cauchy_is_the_scaled_information(ctx):
    g, gauge, q = CC.loop_case("rw200_k16")
    ef, et, meas, info = _a(g)
    plain = ctx.condense_tree(g["poses"], ef, et, meas, info, gauge, q)
    none = ctx.condense_tree(g["poses"], ef, et, meas, info, gauge, q, kind="none")
    assert len(none) == 8 and all(x.tobytes() == y.tobytes() for x, y in zip(plain, none[:6]))
    kinds = np.where(np.abs(ef - et) > 1, RR.KINDS["cauchy"], 0).astype(np.uint8)      # Cauchy on the closures
    fixed = np.zeros(len(g["poses"]), np.uint8)
    fixed[gauge] = 1
    guess = RM.guess_bfs(g["poses"], fixed, ef, et, meas)
    w_ref = RR.weights(guess, ef, et, meas, info, kinds, 1.0)
    assert (w_ref < 0.9).sum() > 10
    rob = ctx.condense_tree(g["poses"], ef, et, meas, info, gauge, q, kind=kinds, delta=1.0)
    sc = ctx.condense_tree(g["poses"], ef, et, meas, info * w_ref[:, None], gauge, q)
    assert np.abs(rob[7] - w_ref).max() <= 1e-12
    assert np.array_equal(rob[0], sc[0]) and np.array_equal(rob[1], sc[1]) and np.array_equal(rob[5], sc[5])
    d_est = np.abs(rob[2] - sc[2]).max()
    d_iu = max(np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(rob[3], sc[3]))
    d_pl = max(np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(plain[3], sc[3]))
    print(f"Cauchy against the scaled information: est {d_est:.2e}, information {d_iu:.2e} (the unweighted call differs by {d_pl:.2e})")
    assert d_est <= AGREE_TAU and d_iu <= AGREE_TAU and d_pl > 1e-3


# --------------------------------------------------------------------------------------- limits, determinism, wrapper
def test_limits_bad_indices_determinism_and_poses_untouched():
    c = Context(0)
    g = synth.make_pose_graph(1100, 2500, seed=29)
    a = (g["poses"], *_a(g))
    over = np.arange(1, TREE_MAX_NODES + 1, dtype=np.int32)       # 1025 unique vertices besides the gauge
    for call in (lambda: c.condense_tree(*a, 0, over),
                 lambda: c.condense_tree(*a, 1100, [3, 4]),
                 lambda: c.condense_tree(*a, -1, [3, 4]),
                 lambda: c.condense_tree(*a, 0, [3, 1100]),
                 lambda: c.condense_tree(*a, 0, [-1])):
        with pytest.raises(CgmrError) as ei:
            call()
        assert ei.value.code == E_INVALID
    p_in = g["poses"].copy()
    q = np.linspace(5, 1090, 40).astype(np.int32)
    one = c.condense_tree(*a, 500, q)                             # the context is still usable
    two = c.condense_tree(*a, 500, q)
    assert len(one[0]) == 40 and all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
    assert np.array_equal(g["poses"], p_in)
    # the limit counts unique vertices besides the gauge
    assert len(c.condense_tree(*a, 0, np.r_[0, np.arange(1, 9), np.arange(1, 9)])[0]) == 8
    c.close()


def test_graph_slam_wrapper_returns_the_context_call_by_id(ctx):
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = synth.make_pose_graph(300, 900, seed=21)
    pg = PoseGraph.from_synth(g)
    gs = GraphSLAM(pg, ctx)
    gs.optimize(3)
    verts, gauge = [250, 10, 40, 41, 120], 40
    fr, to, est, iu, w, fl = gs.condensedTree(verts, gauge)
    c = ctx.condense_tree(pg.poses, *pg.level0(), gauge, verts)
    assert np.array_equal(fr, pg.ids[c[0]]) and np.array_equal(to, pg.ids[c[1]]) and list(c[1]) == [250, 10, 41, 120]
    assert all(np.array_equal(x, y) for x, y in zip((est, iu, w, fl), c[2:]))
