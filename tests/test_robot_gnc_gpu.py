"""Graduated non-convexity on the resident robot graph (include/cgmr.h: cgmr_graph_optimize_gnc, _keep_gnc_weights,
_set_condensed_gnc) against the float64 contract of tests/ref_gnc.py on ``robot_sequences.solved_system``, on the cases of
tests/robot_gnc_cases.py (whose reach predicates tests/test_robot_gnc_cpu.py proves on the reference alone), and the condensed
graphs without the rejected edges against ``ref_numpy.condense_ref`` on the kept own edges."""
import ctypes as C

import numpy as np
import pytest

import ref_numpy as R
import ref_typed
import robot_gnc_cases as RC
from cg_mrslam_amd import synth
from reference_cases import EST_ATOL, INFO_RTOL
from test_gnc_gpu import ANG_TOL, CHI_RTOL, POS_TOL
from test_robust_gpu import STAT_RTOL, e2_bound

pytestmark = pytest.mark.gpu

_PLAIN = {}


def forget_analysis(c):
    """The context forgets the structure it analysed last.  An edge list that shares its front with the cached one has its
    ordering extended from it (the key-frame pattern) -- another summation order: two runs are compared bit for bit only from
    the same state of that cache."""
    c.set_symbolic_cache(False)
    c.set_symbolic_cache(True)


def plain_bits(c):
    """A plain optimize and a plain computeCondensedGraph on a fresh graph of the clean case: everything they return, as bytes."""
    forget_analysis(c)
    case = RC.build("clean", c)
    g = case.rg
    try:
        rc, chi = g.optimize(3)
        assert rc == 0
        out = [g.poses().tobytes(), chi.tobytes()]
        assert g._check(g.lib.cgmr_graph_compute_condensed(g.h, C.c_int(-1))) == len(case.peers)
        for p in case.peers:
            out += [np.asarray(v).tobytes() for v in g.condensed(p)]
        return out
    finally:
        g.close()


@pytest.fixture(scope="module")
def ctx():
    from cg_mrslam_amd import Context
    from cg_mrslam_amd.condensed import RobotGraph
    c = Context(0)
    # the asynchronous batches of test 7 are announced before the first solve, as a robot that uses them does: from then on the
    # context's two streams share the resident workgroups (cgmr_graph_set_async), for every test of this file alike
    g = RobotGraph(c, 0, 2, async_condense=True)
    g.close()
    _PLAIN["before"] = plain_bits(c)
    yield c
    c.close()


def run_gnc(g, loss, **kw):
    return g.optimize_gnc(loss=loss, **kw)


def check_poses(p, ref):
    d = p - ref
    assert float(np.abs(d[:, :2]).max()) <= POS_TOL, float(np.abs(d[:, :2]).max())
    assert float(np.abs(R.normalize_theta(d[:, 2])).max()) <= ANG_TOL


def check_edge_chi2(case, p, e2):
    s = case.sys
    ref = ref_typed.edge_chi2(p, s["ef"], s["et"], s["meas"], s["info"], np.zeros(len(s["ef"]), np.uint8))
    bound = e2_bound(p, s["info"], ref)
    assert np.all(np.abs(e2 - ref) <= bound), float(np.max(np.abs(e2 - ref) / np.maximum(bound, 1e-300)))


def check_star(est, iu, ref):
    d = est - ref["est"]
    d[:, 2] = synth.normalize_theta(d[:, 2])
    assert np.abs(d).max() <= EST_ATOL, float(np.abs(d).max())
    for k in range(len(iu)):
        assert np.linalg.norm(iu[k] - ref["iu"][k]) <= INFO_RTOL * np.linalg.norm(ref["iu"][k]), k


def kept_reference(case, poses, w_own, gauge, tov, oracle):
    """condense_ref on the kept own edges with info * w, the gauge the device reports, the guess over the kept edges only."""
    _, ef, et, meas, info = case.rg.own_system()
    keep = w_own > 0.0
    ref = R.condense_ref(poses, ef[keep], et[keep], meas[keep], info[keep] * w_own[keep, None], gauge,
                         np.r_[gauge, tov].astype(np.int32), oracle.initial_guess)
    assert ref["cov_err"].max() <= 1e-10 and not ref["not_pd"].any()
    assert np.array_equal(ref["to"], tov)
    return ref


def stars(case):
    """{peer: (gauge index, to indices, est, iu)} of the condensed graphs the case's graph holds."""
    g, out = case.rg, {}
    for p in case.peers:
        gid, to, est, iu = g.condensed(p)
        assert gid is not None and len(to) == len(case.want[p]) - 1
        out[p] = (g.index[gid], np.array([g.index[int(i)] for i in to], np.int32), est, iu)
    return out


# ------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("loss", ["tls", "gm"])
@pytest.mark.parametrize("name", ["pair", "trio"])
def test_contract(ctx, name, loss):
    case = RC.build(name, ctx)
    g = case.rg
    try:
        ref = RC.reference(name, loss)
        out = run_gnc(g, loss)
        n = ref["outer_done"]
        print(f"{name} {loss}: {n} outer iterations, mu {np.abs(out['mu'][:n] / ref['mu'][:n] - 1).max():.1e}, "
              f"cost {np.abs(out['cost'] / ref['cost'] - 1).max():.1e}, poses {np.abs(g.poses() - ref['poses']).max():.1e}, "
              f"weights {np.abs(out['weights'] - ref['weights']).max():.1e}")
        assert out["status"] == 0 and out["outer_done"] == n
        assert np.array_equal(out["partial"], ref["partial"])
        np.testing.assert_allclose(out["mu"], ref["mu"], rtol=STAT_RTOL, atol=0)
        np.testing.assert_allclose(out["cost"], ref["cost"], rtol=CHI_RTOL, atol=0)
        p = g.poses()
        check_poses(p, ref["poses"])
        still = case.sys["fixed"] != 0
        assert np.array_equal(p[still], case.poses0[still])
        assert len(out["weights"]) == len(case.sys["ef"])
        if loss == "tls":
            assert np.array_equal(out["weights"], ref["weights"])
            assert np.array_equal(np.flatnonzero(out["weights"] == 0.0), case.bad)       # the received one included
        else:
            assert float(np.abs(out["weights"] - ref["weights"]).max()) <= 2 * CHI_RTOL
        check_edge_chi2(case, p, out["edge_chi2"])
        e2, w = g.edge_stats()
        assert np.array_equal(e2, out["edge_chi2"]) and np.array_equal(w, out["weights"])
        assert np.array_equal(g.gnc_weights(), out["weights"][:case.n_own])
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("loss", ["tls", "gm"])
def test_nothing_to_reject_is_the_plain_solve_bit_for_bit(ctx, loss):
    a, b = RC.build("clean", ctx), RC.build("clean", ctx)
    try:
        out = run_gnc(a.rg, loss, inner_iters=2)
        rc, chi = b.rg.optimize(2)
        assert out["status"] == rc == 0 and out["outer_done"] == 1 and out["mu"][0] == 0.0 and out["partial"][0] == 0
        assert np.all(out["weights"] == 1.0) and out["cost"][0] == chi[0]
        assert np.array_equal(a.rg.poses(), b.rg.poses())
        assert not np.array_equal(a.rg.poses(), a.poses0)
    finally:
        a.rg.close()
        b.rg.close()


# ------------------------------------------------------------------------------------------------------------------- 3
def test_sticky_weights(ctx):
    from cg_mrslam_amd._lib import CgmrError
    case = RC.build("pair", ctx)
    g = case.rg
    try:
        out = run_gnc(g, "tls")
        w_own = out["weights"][:case.n_own]
        assert np.array_equal(np.flatnonzero(w_own == 0.0), case.bad_own)
        i0, i1 = int(case.ids[17]), int(case.ids[30])                            # (neighbours across two rows of the grid)
        z = RC._rel(case.truth[17], case.truth[30])[None]
        g.add_edges([i0], [i1], z, RC.INFO[None])
        assert np.array_equal(g.gnc_weights(), np.r_[w_own, 1.0])                # appended: weight 1, the others as they were
        s = RC.solved_system(g)
        w = np.r_[w_own, 1.0, np.ones(len(s["ef"]) - case.n_own - 1)]            # received edges: weight 1
        # from a perturbed estimate, so that three iterations have something to do
        p0 = g.poses()
        p0[1:, :2] += 0.05 * np.sin(np.arange(1, len(p0)))[:, None]
        g.set_poses(0, p0)
        g.keep_gnc_weights(True)
        rc, chi = g.optimize(3)
        assert rc == 0
        want, chi_ref, _ = ref_typed.gn_optimize(p0, s["fixed"], s["ef"], s["et"], s["meas"], s["info"] * w[:, None], 3)
        print(f"sticky weights: poses {np.abs(g.poses() - want).max():.1e}, chi2 {np.abs(chi / chi_ref - 1).max():.1e}")
        check_poses(g.poses(), want)
        np.testing.assert_allclose(chi, chi_ref, rtol=CHI_RTOL, atol=0)
        assert g.edge_stats() is None
        # the corrupted own closures stay out: the plain solve from the same estimate ends elsewhere
        g.keep_gnc_weights(False)
        g.set_poses(0, p0)
        rc, _ = g.optimize(3)
        assert rc == 0 and np.abs(g.poses() - want)[:, :2].max() > 100 * POS_TOL
        # Levenberg and dogleg take no stored weights
        g.keep_gnc_weights(True)
        for alg in ("levenberg", "dl"):
            g.set_algorithm(alg)
            with pytest.raises(CgmrError) as e:
                g.optimize(2)
            assert e.value.code == -1
        g.set_algorithm("gn")
        assert g.optimize(1)[0] == 0
    finally:
        g.close()


def test_kept_weights_of_one_are_the_plain_solve_bit_for_bit(ctx):
    a, b = RC.build("clean", ctx), RC.build("clean", ctx)
    try:
        a.rg.keep_gnc_weights(True)
        assert np.all(a.rg.gnc_weights() == 1.0)
        (rca, chia), (rcb, chib) = a.rg.optimize(3), b.rg.optimize(3)
        assert rca == rcb == 0 and np.array_equal(chia, chib) and np.array_equal(a.rg.poses(), b.rg.poses())
        assert not np.array_equal(a.rg.poses(), a.poses0)
    finally:
        a.rg.close()
        b.rg.close()


# ------------------------------------------------------------------------------------------------------------------- 4
def test_failure_handling(ctx):
    from cg_mrslam_amd._lib import CGMR_E_CHOLESKY_BASE, CgmrError, GncParams
    case = RC.build("starved", ctx)
    g = case.rg
    try:
        # stored weights worth keeping: Geman-McClure ends well on this graph
        gm = run_gnc(g, "gm")
        stored = g.gnc_weights()
        assert gm["status"] == 0 and np.array_equal(stored, gm["weights"][:case.n_own]) and stored.min() < 1e-3
        g.set_poses(0, case.poses0)
        ref = RC.reference("starved", "tls")
        out = run_gnc(g, "tls", raise_on_cholesky=False)
        assert out["status"] == CGMR_E_CHOLESKY_BASE - ref["failed"]
        assert out["outer_done"] == ref["outer_done"] and np.array_equal(out["partial"], ref["partial"])
        assert out["weights"][case.bad].tolist() == [0.0, 0.0]
        p = g.poses()
        assert np.all(np.isfinite(p))
        check_poses(p, ref["poses"])                                             # the last good update
        assert np.array_equal(g.gnc_weights(), stored)                           # ... and the stored weights as they were
        with pytest.raises(CgmrError):
            g.set_poses(0, case.poses0)
            run_gnc(g, "tls")
        # a plain solve on the same graph and context is healthy
        g.set_poses(0, case.poses0)
        rc, chi = g.optimize(2)
        s = case.sys
        want, _, _ = ref_typed.gn_optimize(case.poses0, s["fixed"], s["ef"], s["et"], s["meas"], s["info"], 2)
        assert rc == 0
        check_poses(g.poses(), want)
        # robust kernels present: refused
        g.set_edge_robust("cauchy", 1.0, first=2, n=1)
        with pytest.raises(CgmrError) as e:
            run_gnc(g, "gm")
        assert e.value.code == -1
        g.set_edge_robust("none", 1.0, first=2, n=1)
        g.set_received_robust("huber", 1.0)
        with pytest.raises(CgmrError) as e:
            run_gnc(g, "gm")
        assert e.value.code == -1
        g.set_received_robust("none")
        # non-null per-edge pointers in the parameters: refused
        buf = np.ones(len(s["ef"]))
        flags = np.zeros(len(s["ef"]), np.uint8)
        for field, arr in (("barc_sq", buf), ("known_inlier", flags), ("weight_out", buf), ("edge_chi2_out", buf)):
            prm = GncParams(1, 1.4, 100, 1, 8, None, 0.0, None, None, None)
            setattr(prm, field, arr.ctypes.data)
            null = C.c_void_p(0)
            assert g.lib.cgmr_graph_optimize_gnc(g.h, C.byref(prm), null, null, null, null) == -1, field
        for bad in (dict(loss=2), dict(mu_factor=1.0), dict(max_outer=0), dict(inner_iters=0), dict(outer_per_wait=0)):
            with pytest.raises(CgmrError) as e:
                run_gnc(g, bad.pop("loss", "gm"), **bad)
            assert e.value.code == -1
        g.set_poses(0, case.poses0)
        assert run_gnc(g, "gm")["status"] == 0                                   # ... and the call still works
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------- 5, 6
def twin_without(case, ctx, poses, drop):
    """A graph with the case's vertices and its own edges except ``drop``, at ``poses``, asked for the same vertices."""
    from cg_mrslam_amd.condensed import RobotGraph
    fixed, ef, et, meas, info = case.rg.own_system()
    keep = np.ones(len(ef), bool)
    keep[drop] = False
    t = RobotGraph(ctx, 0, 1 + len(case.peers))
    t.add_vertices(case.ids, poses, fixed)
    t.add_edges(case.ids[ef[keep]], case.ids[et[keep]], meas[keep], info[keep])
    for p in case.peers:
        t.insertOutClosure(p, case.want[p])
    return t


@pytest.mark.parametrize("name", ["pair", "trio"])
def test_condensed_graphs_leave_the_rejected_edges_out(ctx, oracle, name):
    case = RC.build(name, ctx)
    g = case.rg
    twin = None
    try:
        out = run_gnc(g, "tls")
        assert out["status"] == 0
        w_own = g.gnc_weights()
        assert np.array_equal(np.flatnonzero(w_own == 0.0), case.bad_own)
        g.set_condensed_gnc(True)
        assert g.computeCondensedGraph(-1) == len(case.peers)                    # trio: one batch of two jobs
        poses = g.poses()
        on = stars(case)
        worst = np.zeros(2)
        for p, (gauge, tov, est, iu) in on.items():
            ref = kept_reference(case, poses, w_own, gauge, tov, oracle)
            d = est - ref["est"]
            worst = np.maximum(worst, [np.abs(d[:, :2]).max(), max(np.linalg.norm(iu[k] - ref["iu"][k]) / np.linalg.norm(ref["iu"][k])
                                                                      for k in range(len(tov)))])
            check_star(est, iu, ref)
        print(f"{name}: condensed graphs on the kept edges against condense_ref: est {worst[0]:.1e} m, information {worst[1]:.1e}")
        # switched off, the same call builds something else: the rejected closures are back in
        g.set_condensed_gnc(False)
        assert g.computeCondensedGraph(-1) == len(case.peers)
        for p, (gauge, tov, est, iu) in stars(case).items():
            assert gauge == on[p][0] and np.array_equal(tov, on[p][1])
            assert not np.allclose(iu, kept_reference(case, poses, w_own, gauge, tov, oracle)["iu"], rtol=1e-3, atol=0), p
        # 6: a graph that never had the corrupted edges, at the same poses, on the plain path
        twin = twin_without(case, ctx, poses, case.bad_own)
        assert twin.computeCondensedGraph(-1) == len(case.peers)
        for p, (gauge, tov, est, iu) in on.items():
            gid, to, est_t, iu_t = twin.condensed(p)
            assert g.index[gid] == gauge and np.array_equal([g.index[int(i)] for i in to], tov)
            check_star(est, iu, dict(est=est_t, iu=iu_t))
    finally:
        g.close()
        if twin is not None:
            twin.close()


def test_drop_below_removes_the_outliers_of_geman_mcclure(ctx, oracle):
    case = RC.build("pair", ctx)
    g = case.rg
    try:
        assert run_gnc(g, "gm")["status"] == 0
        w_own = g.gnc_weights()
        assert np.array_equal(np.flatnonzero(w_own < 1e-3), case.bad_own) and np.all(w_own > 0.0)    # GM: never an exact zero
        g.set_condensed_gnc(True, 1e-3)
        assert g.computeCondensedGraph(-1) == len(case.peers)
        poses = g.poses()
        kept = np.where(w_own < 1e-3, 0.0, w_own)
        for p, (gauge, tov, est, iu) in stars(case).items():
            check_star(est, iu, kept_reference(case, poses, kept, gauge, tov, oracle))
        # drop_below = 0 removes nothing here: the corrupted closures stay in the spanning tree's reach, at their small weight
        g.set_condensed_gnc(True, 0.0)
        assert g.computeCondensedGraph(-1) == len(case.peers)
        for p, (gauge, tov, est, iu) in stars(case).items():
            check_star(est, iu, kept_reference(case, poses, w_own, gauge, tov, oracle))
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------- 7
def test_async_batch_works_from_the_weights_as_they_were_queued(ctx):
    """compute_condensed_async, then at once one more corrupted closure and another GNC solve (which rewrites the stored
    weights), then the wait: the packed message is that of the same sequence with the batch built synchronously."""
    def sequence(go_async):
        forget_analysis(ctx)
        case = RC.build("trio", ctx)
        g = case.rg
        try:
            g._check(g.lib.cgmr_graph_set_async(g.h, C.c_int(1)))
            assert run_gnc(g, "tls")["status"] == 0
            g.set_condensed_gnc(True)
            entry = g.lib.cgmr_graph_compute_condensed_async if go_async else g.lib.cgmr_graph_compute_condensed
            assert g._check(entry(g.h, C.c_int(-1))) == len(case.peers)
            z = RC._rel(case.truth[10], case.truth[100]) + [3.5, 2.0, -1.0]
            g.add_edges([int(case.ids[10])], [int(case.ids[100])], z[None], RC.INFO[None])
            out = run_gnc(g, "tls")
            assert out["status"] == 0 and out["weights"][case.n_own] == 0.0          # the new closure is rejected as well
            g.condensed_wait()
            assert g.failed_batches() == 0
            return g.pack_host().tobytes(), [np.asarray(v).tobytes() for p in case.peers for v in g.condensed(p)]
        finally:
            g.close()
    sync, asyn = sequence(False), sequence(True)
    assert asyn[1] == sync[1]
    assert asyn[0] == sync[0]


# ------------------------------------------------------------------------------------------------------------------- 8
def test_no_state_leaks_into_the_plain_calls(ctx):
    """Last in the file: the plain optimize and computeCondensedGraph of a fresh graph, before anything above ran on this
    context (the ctx fixture) and now."""
    case = RC.build("pair", ctx)                                                  # (also when this test runs alone)
    try:
        run_gnc(case.rg, "tls")
        case.rg.set_condensed_gnc(True)
        case.rg.computeCondensedGraph(-1)
    finally:
        case.rg.close()
    assert plain_bits(ctx) == _PLAIN["before"]
