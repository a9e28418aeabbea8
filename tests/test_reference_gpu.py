"""The solver's linear algebra against yardsticks that need no second implementation of it (tests/test_reference_cpu.py proves
they discriminate): every Gauss-Newton step's componentwise backward error against H and b assembled in numpy
(ref_numpy.step_backward_error <= OMEGA_MAX), on graphs that reach each branch of the supernodal factorisation and under the
launch variants; marginal blocks against refined columns of H^-1 (ref_numpy.marginal_blocks_ref), each by its own norm; the
condensed graph against the numpy unscented labelling; and the marginal path's recovery from a bounded wait that ran out."""
import json

import numpy as np
import pytest

import ref_numpy as R
import reference_cases as C
from reference_cases import EST_ATOL, EST_OWN_ATOL_BATCH, INFO_RTOL, OMEGA_MAX, REF_ERR_MAX
from reference_cases import check_labels_on_own_step as _check_labels_on_own_step
from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import gn_symbolic_info
from switch_contexts import assert_launch_shape, context_under
from switch_contexts import launch_counts as _launches

pytestmark = pytest.mark.gpu

MARG_TAU = 1e-9        # ||Sigma_gpu - Sigma_ref||_F <= MARG_TAU ||Sigma_ref||_F, per block (measured: 3.1e-10)
# ... on the pass repeated with one launch per kernel and level after a time-out: 1.15e-9 measured on the 2500/9000 graph
# (cond_1(H) 1.1e10 by onenormest), asserted at ten times that
MARG_TAU_LEVELWISE = 1.2e-8
TOP_MAX_COLS = 128     # kTopMaxCols (gn_symbolic.h): scalar columns of the top block


@pytest.fixture(scope="module")
def ctx_resident_only():
    """A context that merges only the level launches that are certainly resident (CGMR_FWD_MERGE_ANY=0, read at creation)."""
    with context_under({"CGMR_FWD_MERGE_ANY": "0"}) as c:
        yield c


def _branch(name, g, ctx, ctx_resident_only):
    """The case reaches the branch it is there for (reference_cases.CASES)."""
    info = gn_symbolic_info(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    if name in ("pg500", "pg2500", "pg9000", "c2", "illcond"):
        n = _launches(ctx, C.args(g))
        n_res = _launches(ctx_resident_only, C.args(g))
        assert info["launch_levels"] >= 4 and n["front_level"] > 0                 # merged level launches
        assert n["solve_bwd"] < info["launch_levels"]                               # a chained backward solve
        if name in ("pg9000", "c2"):                         # levels merged although not certainly resident at once
            assert n["front_level"] > n_res["front_level"], (n, n_res)
        else:
            assert n["front_level"] == n_res["front_level"], (n, n_res)
    if name == "illcond":
        import scipy.sparse.linalg as spla
        H, _, _ = R.build_system(g["poses"], g["fixed"], *C.args(g)[2:])
        lu = spla.splu(H.tocsc())
        op = spla.LinearOperator(H.shape, matvec=lu.solve, rmatvec=lu.solve, dtype=float)
        assert spla.onenormest(H) * spla.onenormest(op) > 1e12                      # (measured: 1.4e16)
    if name == "lat74":
        assert info["top_block_cols"] > TOP_MAX_COLS - 6                            # within one pose of kTopMaxCols
    if name in ("v2e1", "v5e4"):
        assert info["top_block_fronts"] == info["fronts"]
    elif name == "chain3000":
        assert info["max_border"] <= 2 and info["fronts"] > 100          # dissected chain: borders of 1-2 poses
    elif name == "hub40":
        assert info["max_children"] > 8
    elif name == "hub100":
        assert info["max_children"] > 64
    elif name.startswith("lat"):
        assert info["max_border"] >= int(name[3:])
    elif name == "wrap":
        assert C.straddling_edges(g) >= 20
    elif name == "fixed_dup_iso":
        assert int(g["fixed"].sum()) == 3 and len(g["edge_from"]) > len(set(zip(g["edge_from"], g["edge_to"])))
    return info


@pytest.mark.parametrize("name", list(C.CASES))
def test_gn_step_backward_error(ctx, ctx_resident_only, name):
    """One step from the initial guess, from the GPU's own 3rd iterate and from its 8th."""
    g = C.CASES[name][0]()
    _branch(name, g, ctx, ctx_resident_only)
    a = C.args(g)
    worst = 0.0
    for start in (0, 3, 8):
        p0 = g["poses"]
        if start:
            rc, p0, _ = ctx.gn_optimize(*a, start)
            assert rc == 0
        rc, p1, _ = ctx.gn_optimize(p0, *a[1:], 1)
        assert rc == 0
        w = R.step_backward_error(p0, p1, *a[1:])
        worst = max(worst, w)
        assert w <= OMEGA_MAX, (name, start, w / R.U)
    print(f"{name}: largest omega {worst / R.U:.1f} u")


def test_gn_step_backward_error_device_entry_and_extended_ordering(ctx):
    """gn_optimize_dev's step, and steps on an ordering extended from the cached one (a grown graph)."""
    import torch
    g = synth.make_pose_graph(2000, 7000, seed=13)
    a = C.args(g)
    dev = torch.device("cuda:0")
    d_p = torch.tensor(g["poses"], dtype=torch.float64, device=dev).contiguous()
    d_m = torch.tensor(g["meas"], dtype=torch.float64, device=dev).contiguous()
    d_i = torch.tensor(g["info"], dtype=torch.float64, device=dev).contiguous()
    torch.cuda.synchronize()
    rc, _ = ctx.gn_optimize_dev(d_p.data_ptr(), 2000, g["fixed"], g["edge_from"], g["edge_to"], d_m.data_ptr(), d_i.data_ptr(), 1)
    assert rc == 0
    assert R.step_backward_error(g["poses"], d_p.cpu().numpy(), *a[1:]) <= OMEGA_MAX
    # grow: the first 1900 vertices and their edges, then all of them (the cached ordering is extended)
    last = np.maximum(g["edge_from"], g["edge_to"])
    k = np.argsort(last, kind="stable")
    ef, et, meas, info = (np.ascontiguousarray(g[n][k]) for n in ("edge_from", "edge_to", "meas", "info"))
    ne = int(np.searchsorted(last[k], 1900))
    ctx.set_symbolic_cache(True)
    rc, _, _ = ctx.gn_optimize(g["poses"][:1900], g["fixed"][:1900], ef[:ne], et[:ne], meas[:ne], info[:ne], 2)
    assert rc == 0
    s0 = ctx.symbolic_cache_stats()
    rc, p1, _ = ctx.gn_optimize(g["poses"], g["fixed"], ef, et, meas, info, 1)
    assert rc == 0 and ctx.symbolic_cache_stats()["extended"] == s0["extended"] + 1
    assert R.step_backward_error(g["poses"], p1, g["fixed"], ef, et, meas, info) <= OMEGA_MAX


VARIANTS = (("default", {}), ("separate_launches", {"CGMR_FWD_MERGE": "0"}), ("chain_wgs_2", {"CGMR_BWD_CHAIN_WGS": "2"}),
            ("chain_wgs_4", {"CGMR_BWD_CHAIN_WGS": "4"}), ("merge_resident_only", {"CGMR_FWD_MERGE_ANY": "0"}),
            ("no_top_block", {"CGMR_TOP_BLOCK": "0"}), ("panels_cleared_apart", {"CGMR_CLEAR_IN_TOP": "0"}),
            # (chunk lengths below the defaults 79 / 95 / 31: the panel loads of the factor kernel are sized for the defaults)
            ("short_chunks", {"CGMR_CHUNK": "47", "CGMR_LEAF_CHUNK": "63", "CGMR_TOP_CHUNK": "47"}),
            ("bwd_levelwise", {"CGMR_BWD_CHAIN": "0"}), ("no_amalgamation", {"CGMR_AMALGAMATE": "0"}))
VARIANT_CASES = (("pg2500", 3), ("pg9000", 6), ("lat80", 3), ("hub100", 3))

def test_launch_variants_backward_error():
    """Every switch that changes the factorisation's shape, one context at a time (a context reads them when it is created):
    each step's backward error, on graphs whose tree fits the resident workgroups and on ones that do not, a lattice with
    wide borders and a hub with > 64 children.  Each variant's context holds its switches, and its launches show them.
    (CGMR_GRAPH is left out: it replays a captured graph.)"""
    graphs = {name: C.CASES[name][0]() for name, _ in VARIANT_CASES}
    report = {}
    for vname, env in VARIANTS:
        with context_under(env) as c:
            assert_launch_shape(c, env, C.args(graphs[VARIANT_CASES[0][0]]))
            for name, iters in VARIANT_CASES:
                a = C.args(graphs[name])
                ps = [a[0]]
                for it in range(iters):
                    rc, p, _ = c.gn_optimize(ps[-1], *a[1:], 1)
                    assert rc == 0, (vname, name, it, rc)
                    ps.append(p)
                ws = [R.step_backward_error(ps[i], ps[i + 1], *a[1:]) for i in range(iters)]
                report[(vname, name)] = [round(w / R.U, 1) for w in ws]
                assert max(ws) <= OMEGA_MAX, (vname, name, report[(vname, name)])
            assert c.gn_timeouts() == 0, vname
    print("omega / u per iteration:", json.dumps({f"{v}/{n}": w for (v, n), w in report.items()}))


def _top_vertices(g, k):
    """The k vertices eliminated last: the root front / top block."""
    _, perm = gn_symbolic_info(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"], want_perm=True)
    return np.argsort(perm)[-k:].astype(np.int32)


def _check_marginals(ctx, g, p, query):
    a = C.args(g)
    cov = ctx.marginals(p, g["fixed"], *a[2:], query)
    fx = R.active_fixed(len(p), g["fixed"], g["edge_from"], g["edge_to"])
    H, _, hidx = R.build_system(p, fx, *a[2:])
    want, err = R.marginal_blocks_ref(H, hidx, query)
    assert err.max() <= REF_ERR_MAX, "the reference itself is not accurate enough here"
    worst = 0.0
    for k, v in enumerate(query):
        if hidx[v] < 0:
            assert np.all(cov[k] == 0), v                     # fixed / inactive: exact zeros
            continue
        e = np.linalg.norm(cov[k] - want[k]) / np.linalg.norm(want[k])
        worst = max(worst, e)
        assert e <= MARG_TAU, (int(v), e)
    return worst


@pytest.mark.parametrize("nK", [1, 3, 4, 5, 16, 17, 64, 65])
def test_marginals_query_counts(ctx, nK):
    """The padding of the query columns to 16 and the groups of 4 queries; the fixed vertex, its neighbours, the top block."""
    g = synth.make_pose_graph(1500, 5000, seed=47)
    rc, p, _ = ctx.gn_optimize(*C.args(g), 6)
    assert rc == 0
    near = np.unique(np.r_[g["edge_to"][g["edge_from"] == 0], g["edge_from"][g["edge_to"] == 0]])
    pool = np.unique(np.r_[0, near, _top_vertices(g, 6), np.linspace(1, 1499, 80).astype(np.int32)]).astype(np.int32)
    query = pool[np.random.default_rng(nK).permutation(len(pool))[:nK]]
    if nK >= 3:
        query[:3] = [0, near[0], _top_vertices(g, 1)[0]]
    w = _check_marginals(ctx, g, p, np.ascontiguousarray(query, dtype=np.int32))
    print(f"nK {nK}: largest block error {w:.2e}")


@pytest.mark.parametrize("name", ["hub100", "lat80", "small60"])
def test_marginals_on_hub_lattice_and_every_vertex(ctx, name):
    if name == "small60":
        g = synth.make_pose_graph(60, 110, seed=48)
        query = np.arange(60, dtype=np.int32)                  # every front is live
    else:
        g = C.CASES[name][0]()
        V = len(g["poses"])
        query = np.unique(np.r_[np.arange(min(6, V)), _top_vertices(g, 8), np.linspace(0, V - 1, 40).astype(np.int32)])
        query = query.astype(np.int32)                          # (hub graphs: the hubs are vertices 0..n_hubs-1)
    rc, p, _ = ctx.gn_optimize(*C.args(g), 5)
    assert rc == 0
    w = _check_marginals(ctx, g, p, query)
    print(f"{name}: largest block error {w:.2e}")


def _condense_case(oracle, g, gauge, query, p):
    ref = R.condense_ref(p, *C.args(g)[2:], gauge, query, oracle.initial_guess)
    assert np.all(ref["cov_err"] <= REF_ERR_MAX), "the reference itself is not accurate enough here"
    return ref


@pytest.mark.parametrize("wrap", [False, True])
def test_condense_and_covariance_estimate_against_reference(ctx, oracle, wrap):
    g = C.wrap_graph() if wrap else synth.make_pose_graph(1500, 5000, seed=45)
    a = C.args(g)
    rc, p, _ = ctx.gn_optimize(*a, 8)
    assert rc == 0
    V = len(p)
    gauge = V - 1
    query = np.unique(np.r_[np.linspace(0, V - 1, 24).astype(np.int32), gauge]).astype(np.int32)
    if wrap:                                   # pairs whose relative heading is near +-pi: the sigma points wrap
        rel = np.abs(synth.normalize_theta(p[:, 2] - p[gauge, 2]))
        query = np.unique(np.r_[query, np.argsort(-rel)[:8]]).astype(np.int32)
        assert rel[query].max() > 3.0
    ref = _condense_case(oracle, g, gauge, query, p)
    # covariance_estimate (mode 1): the marginals of H at the spanning-tree guess from the gauge
    cov = ctx.covariance_estimate(p, *a[2:], gauge, query)
    for k, v in enumerate(query):
        if v == gauge:
            assert np.all(cov[k] == 0)
            continue
        j = int(np.flatnonzero(ref["to"] == v)[0])
        assert np.linalg.norm(cov[k] - ref["cov"][j]) <= MARG_TAU * np.linalg.norm(ref["cov"][j]), int(v)
    # condense (mode 2): the same marginals; measurement and information at the poses after the one completed step
    to, est, iu, cov2 = ctx.condense(p, *a[2:], gauge, query)
    assert np.array_equal(to, ref["to"]) and not ref["not_pd"].any()
    np.testing.assert_allclose(est, ref["est"], rtol=0, atol=EST_ATOL)
    for k in range(len(to)):
        assert np.linalg.norm(cov2[k] - ref["cov"][k]) <= MARG_TAU * np.linalg.norm(ref["cov"][k])
        assert np.linalg.norm(iu[k] - ref["iu"][k]) <= INFO_RTOL * np.linalg.norm(ref["iu"][k]), int(to[k])
    d = _check_labels_on_own_step(ctx, *a[2:], gauge, ref, to, est, iu)
    print(f"condense: est against the own step's labels {d:.1e}")


def test_marginal_path_recovers_from_a_bounded_wait_that_ran_out(oracle):
    """CGMR_BWD_SPIN_LIMIT=1 (one poll per wait) makes the merged level launches' hand-offs run out: marginals, the covariance
    estimate and the condensed graph must still return OK with blocks that meet the reference (the pass is repeated with one
    launch per kernel and level), the context counts the event, and its cached structure merges from then on exactly the
    levels a context merges that only ever merged what is certainly resident.  The switch belongs to the context (read when
    it is created): the estimate the blocks are taken at comes from a second, plain context."""
    from cg_mrslam_amd import Context
    g = synth.make_pose_graph(2500, 9000, seed=5)
    a = C.args(g)
    plain = Context(0)
    rc, p, _ = plain.gn_optimize(*a, 8)
    plain.close()
    assert rc == 0
    query = np.linspace(0, 2499, 20).astype(np.int32)
    gauge = 2499
    fx = R.active_fixed(2500, g["fixed"], g["edge_from"], g["edge_to"])
    H, _, hidx = R.build_system(p, fx, *a[2:])
    want, _ = R.marginal_blocks_ref(H, hidx, query)
    ref = _condense_case(oracle, g, gauge, query, p)
    with context_under({"CGMR_BWD_SPIN_LIMIT": "1"}) as c, context_under({"CGMR_FWD_MERGE_ANY": "0"}) as c2:
        t0 = c.gn_timeouts()
        cov = c.marginals(p, g["fixed"], *a[2:], query)
        t1 = c.gn_timeouts()
        cov_e = c.covariance_estimate(p, *a[2:], gauge, query)
        to, est, iu, _ = c.condense(p, *a[2:], gauge, query)
        # the cached structure after the time-out against a context that never asked for merges beyond the resident ones
        # (a pass of the spin-limited context that runs out again is repeated with separate launches: no merged one more)
        n_b, n_c = _launches(c, a), _launches(c2, a)
        assert n_b["front_level"] == n_c["front_level"] > 0, (n_b, n_c)
        assert c2.gn_timeouts() == 0
    assert t1 >= t0 + 1, "the forced time-out did not happen: the test checks nothing"
    assert query[0] == 0 and hidx[0] < 0 and np.all(cov[0] == 0)         # the fixed vertex: exact zeros
    for k in range(1, len(query)):
        assert np.linalg.norm(cov[k] - want[k]) <= MARG_TAU_LEVELWISE * np.linalg.norm(want[k])
    for k, v in enumerate(query[:-1]):
        j = int(np.flatnonzero(ref["to"] == v)[0])
        assert np.linalg.norm(cov_e[k] - ref["cov"][j]) <= MARG_TAU_LEVELWISE * np.linalg.norm(ref["cov"][j])
    np.testing.assert_allclose(est, ref["est"], rtol=0, atol=EST_ATOL)
    for k in range(len(to)):
        assert np.linalg.norm(iu[k] - ref["iu"][k]) <= INFO_RTOL * np.linalg.norm(ref["iu"][k])


def test_batched_condensed_graphs_against_reference(oracle):
    """The batched condensed path (k_solve_fwd_multi and k_label_edges with a job dimension, condensed_host.cpp run_cond_jobs)
    through RobotGraph.computeCondensedGraph: the first round of three robots with their own edges only, so the graph each
    condensed graph is built on is known exactly.  Gauge and query as RefRobotGraph takes them (selectGaugeCentroid over the
    requested vertices); every condensed(peer) meets condense_ref at the bars of the single-graph path."""
    from cg_mrslam_amd import Context
    from cg_mrslam_amd.condensed import RobotGraph
    from ref_condensed import select_gauge_centroid
    c = Context(0)
    nr, V = 3, 1200
    checked = 0
    for r in range(nr):
        g = synth.make_pose_graph(V, 4000, seed=50 + r, id_base=r * 10000)
        ids = g["ids"].astype(np.int64)
        rg = RobotGraph(c, r, nr)
        rg.add_vertices(ids, g["poses"], g["fixed"])
        rg.add_edges(ids[g["edge_from"]], ids[g["edge_to"]], g["meas"], g["info"])
        rc, _ = rg.optimize(6)
        assert rc == 0
        want = {}
        for p in range(nr):
            if p == r:
                continue
            rng = np.random.default_rng(100 * r + p)
            want[p] = np.sort(rng.choice(V, 12 + 5 * p, replace=False)).astype(np.int32)
            rg.insertOutClosure(p, ids[want[p]])
        assert rg.computeCondensedGraph(-1) == nr - 1
        poses = rg.poses()
        ef, et, meas, info = g["edge_from"], g["edge_to"], g["meas"], g["info"]
        for p, idx in want.items():
            gid, to, est, iu = rg.condensed(p)
            gauge = int(idx[select_gauge_centroid(poses[idx, :2])])
            assert gid == ids[gauge]
            ref = _condense_case(oracle, dict(g, poses=poses), gauge, idx, poses)
            k = np.argsort(to)
            to, est, iu = to[k], est[k], iu[k]
            assert np.array_equal(to, np.sort(ids[ref["to"]])) and not ref["not_pd"].any()
            j = np.argsort(ids[ref["to"]])
            rto = ref["to"][j]
            np.testing.assert_allclose(est, ref["est"][j], rtol=0, atol=EST_ATOL)
            for q in range(len(to)):
                assert np.linalg.norm(iu[q] - ref["iu"][j][q]) <= INFO_RTOL * np.linalg.norm(ref["iu"][j][q]), (r, p, int(to[q]))
            ref_sorted = dict(ref, cov=ref["cov"][j])
            d = _check_labels_on_own_step(c, ef, et, meas, info, gauge, ref_sorted, rto, est, iu, atol=EST_OWN_ATOL_BATCH)
            print(f"batched condensed graph {r}->{p}: est against the own step's labels {d:.1e}")
            checked += 1
    assert checked == nr * (nr - 1)
