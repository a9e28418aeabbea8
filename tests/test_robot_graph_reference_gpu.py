"""The device-resident robot graph (cgmr_graph_*) against float64 references, round after round of the C5 protocol with a context
per robot -- so that every robot's analysis cache extends its own ordering with the received stars' gauge vertices forced into
the root separator.  Each checked Gauss-Newton step is checked against H and b assembled in numpy from the system the solve
saw (robot_sequences.solved_system: own edges as added, received edges with the float32-rounded values of the staging), by
ref_numpy.step_backward_error <= OMEGA_MAX; a check that resolves one received edge dropped or its information scaled by
1 + 1e-9.  Condensed graphs of later rounds, built with the received edges switched off, are checked against
ref_numpy.condense_ref on the own edges, and the optimal gauge against the reference's uncertainties.  Also checked: the
asynchronous batch with the device exchange, and the launch variants that change the factorisation's shape."""
import contextlib
import os

import numpy as np
import pytest

import ref_numpy as R
from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import CgmrError
from reference_cases import EST_ATOL, EST_OWN_ATOL_BATCH, INFO_RTOL, OMEGA_MAX, REF_ERR_MAX, check_labels_on_own_step
from ref_condensed import select_gauge_centroid
from switch_contexts import assert_launch_shape, context_under
from robot_sequences import checked_rounds, make_robot_rounds, run_steps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (robots, vertices per robot, edges per robot, seed, chunk, rounds).  Seeds whose robots meet in round 4: received
# edges are in most rounds' solves, and the stars grow from 1 to ~50 edges (below and above the analysis' hub degree of 32)
CASES = {"2robots": (2, 1200, 4000, 44, 60, 20), "3robots": (3, 900, 3000, 48, 50, 18)}
SYSTEM_KEYS = ("fixed", "ef", "et", "meas", "info")


def _close(rounds, ctxs):
    for rr in rounds:
        rr.g.close()
    for c in ctxs:
        c.close()


@pytest.fixture(scope="module")
def runs():
    """The rounds of a case, driven once for the tests below: steps, analysis sequences, condensed graphs, per-context counts."""
    from cg_mrslam_amd import Context
    done = {}

    def get(name):
        if name not in done:
            nr, nv, ne, seed, chunk, n_rounds = CASES[name]
            ctxs = [Context(0) for _ in range(nr)]
            rounds = make_robot_rounds(ctxs, nv, ne, seed, chunk)
            ext0 = [c.symbolic_cache_stats()["extended"] for c in ctxs]
            r = dict(error=None)
            try:
                checked_rounds(rounds, n_rounds, optimal=(n_rounds // 2, 0), record_condensed=True, out=r)
            except (AssertionError, CgmrError) as e:    # (a failed round: the tests check what was recorded before it, then report it)
                r["error"] = repr(e)
            finally:
                r.update(own=[rr.g.own_system() for rr in rounds], timeouts=[c.gn_timeouts() for c in ctxs],
                         extended=[c.symbolic_cache_stats()["extended"] - e for c, e in zip(ctxs, ext0)])
                _close(rounds, ctxs)
            done[name] = r
        return done[name]
    return get


def _omegas(steps):
    return [R.step_backward_error(s["p0"], s["p1"], *(s[k] for k in SYSTEM_KEYS)) for s in steps]


def _check_steps(label, steps):
    """Every step's backward error; returns (omegas, steps with received edges)."""
    ws = _omegas(steps)
    n_recv = sum(1 for s in steps if len(s["ef"]) > s["n_own"])
    worst = int(np.argmax(ws))
    print(f"{label}: {len(steps)} steps, {n_recv} with received edges, largest omega {ws[worst] / R.U:.1f} u "
          f"(round {steps[worst]['t']}, robot {steps[worst]['robot']}, from iterate {steps[worst]['start']})")
    bad = [(s["t"], s["robot"], s["start"], round(w / R.U, 1)) for s, w in zip(steps, ws) if not w <= OMEGA_MAX]
    assert not bad, (label, "steps above OMEGA_MAX (round, robot, iterate, omega / u)", bad)
    return ws, n_recv


def _root_separator_start(fronts):
    """First column of the root's separator: the root front and the chain of fronts below it that have one child each (a
    front's only child is the front just before it in the table)."""
    f = len(fronts) - 1
    assert fronts[f, 3] == -1
    while fronts[f, 5] == 1:
        assert fronts[f - 1, 3] == f
        f -= 1
    return int(fronts[f, 0])


def _hubs_in_root_separator(seq):
    """Replays a robot's analyses (robot_sequences.run_steps) and returns, per round with received stars, whether every
    gauge vertex sits in the root separator, and the number of analyses the replay extended."""
    out = []
    for k in range(len(seq)):
        hubs = seq[k][4]
        if len(hubs) == 0:
            continue
        _, perm, _, fronts, _ = run_steps(seq[:k + 1])
        out.append(bool(perm[hubs].min() >= _root_separator_start(fronts)))
    return out, run_steps(seq)[2]


@pytest.mark.parametrize("name", list(CASES))
def test_every_rounds_steps_against_float64(runs, name):
    """A: every robot's first step of every round and, every third round, its step from the 3rd iterate.  The case must reach
    the branches it is there for: received edges in most steps, an extended ordering on every context, the gauge vertices of
    the received stars in the root separator in every round that has them."""
    r = runs(name)
    steps = r["steps"]
    ws, n_recv = _check_steps(name, steps)
    assert r["error"] is None, r["error"]
    first = [s for s in steps if s["start"] == 0]
    n_recv_first = sum(1 for s in first if len(s["ef"]) > s["n_own"])
    assert any(s["start"] == 3 and len(s["ef"]) > s["n_own"] for s in steps)
    assert r["timeouts"] == [0] * len(r["timeouts"]), r["timeouts"]
    placed = [_hubs_in_root_separator(seq) for seq in r["seqs"]]
    print(f"{name}: extended orderings per context {r['extended']}, replayed {[p[1] for p in placed]}; "
          f"rounds with stars {[len(p[0]) for p in placed]}, gauges in the root separator {[sum(p[0]) for p in placed]}")
    assert n_recv_first > len(first) // 2, (n_recv_first, len(first))
    assert all(e > 0 for e in r["extended"]), r["extended"]
    for rob, (ok, _) in enumerate(placed):
        assert len(ok) > 0 and all(ok), (rob, ok)


@pytest.mark.parametrize("name", list(CASES))
def test_the_step_check_resolves_one_received_edge(runs, name):
    """B: in the round in which a robot's first star arrives, its first step against the system without one received edge,
    and with one received edge's information scaled by 1 + 1e-9: both must be above OMEGA_MAX (the reference sees the
    second edge segment, whose values the device gathers from the staging slots).  Measured on these graphs: 3.5e3 .. 9.0e5 u
    for the scaled information, above 1e15 u for a dropped edge; the device's own steps show 0-0.6 u."""
    steps = runs(name)["steps"]
    for rob in range(CASES[name][0]):
        s = next(s for s in steps if s["robot"] == rob and s["start"] == 0 and len(s["ef"]) > s["n_own"])
        a = [s[k] for k in SYSTEM_KEYS]
        n_own, n = s["n_own"], len(s["ef"])
        w_ok = R.step_backward_error(s["p0"], s["p1"], *a)
        w_drop, w_scale = [], []
        for j in range(n_own, n):
            keep = np.arange(n) != j
            w_drop.append(R.step_backward_error(s["p0"], s["p1"], a[0], *(x[keep] for x in a[1:])))
            info = a[4].copy()
            info[j] *= 1 + 1e-9
            w_scale.append(R.step_backward_error(s["p0"], s["p1"], *a[:4], info))
        print(f"{name} robot {rob}, round {s['t']} ({n - n_own} received edges): omega {w_ok / R.U:.1f} u; one edge dropped "
              f"{min(w_drop) / R.U:.3g} .. {max(w_drop) / R.U:.3g} u; information x (1 + 1e-9) "
              f"{min(w_scale) / R.U:.3g} .. {max(w_scale) / R.U:.3g} u")
        assert w_ok <= OMEGA_MAX
        assert w_drop[0] > OMEGA_MAX and w_scale[0] > OMEGA_MAX, (w_drop[0] / R.U, w_scale[0] / R.U)
    assert runs(name)["error"] is None, runs(name)["error"]


def _condensed_against_reference(c, oracle, rec, own, gauge):
    """One recorded condensed graph against condense_ref on the own edges at the gauge given; returns (est error, info error,
    est against the labels of the GPU's own step) or raises."""
    fixed, ef, et, meas, info = own
    n_own = rec["n_own"]
    ef, et, meas, info = ef[:n_own], et[:n_own], meas[:n_own], info[:n_own]
    poses, idx = rec["poses"], rec["want"]
    ref = R.condense_ref(poses, ef, et, meas, info, gauge, idx, oracle.initial_guess)
    assert np.all(ref["cov_err"] <= REF_ERR_MAX), "the reference itself is not accurate enough here"
    assert not ref["not_pd"].any()
    k, j = np.argsort(rec["to"]), np.argsort(ref["to"])
    to, est, iu = rec["to"][k], rec["est"][k], rec["iu"][k]
    assert np.array_equal(to, ref["to"][j])
    d = est - ref["est"][j]
    d[:, 2] = synth.normalize_theta(d[:, 2])
    e_est = float(np.abs(d).max())
    e_info = max(float(np.linalg.norm(iu[q] - ref["iu"][j][q]) / np.linalg.norm(ref["iu"][j][q])) for q in range(len(to)))
    assert e_est <= EST_ATOL, e_est
    assert e_info <= INFO_RTOL, e_info
    d_own = check_labels_on_own_step(c, ef, et, meas, info, gauge, dict(ref, cov=ref["cov"][j]), to, est, iu, atol=EST_OWN_ATOL_BATCH)
    return e_est, e_info, d_own


@pytest.mark.parametrize("name", list(CASES))
def test_later_round_condensed_graphs_against_reference(runs, ctx, oracle, name):
    """C: every condensed graph of round 2 on that a robot built while it held received edges (switched off in the pass:
    the foreign vertices stay in it through the robot's own closure edges) against condense_ref on the own edges, the gauge
    chosen by select_gauge_centroid over the requested vertices.  The flat-array calls of the check run on a context of their
    own (ctx).  In one round robot 0 picks the optimal gauge: that star must meet the reference for its gauge, and the gauge
    must minimise the reference's sum of det(information^-1) over the candidates (unless the two best are within 1e-6)."""
    r = runs(name)
    recs = [c for c in r["conds"] if c["t"] >= 1]
    worst, fails, n_opt = np.zeros(3), [], 0
    for rec in recs:
        poses, idx = rec["poses"], rec["want"]
        gauge = int(idx[select_gauge_centroid(poses[idx, :2])])
        try:
            if rec["optimal"]:
                ef, et, meas, info = (x[:rec["n_own"]] for x in r["own"][rec["robot"]][1:])
                unc = {}
                for cand in idx.tolist():
                    ref = R.condense_ref(poses, ef, et, meas, info, cand, idx, oracle.initial_guess)
                    unc[cand] = float(np.sum(1.0 / np.linalg.det(R.info_full(ref["iu"]))))
                order = sorted(unc, key=unc.get)
                n_opt = len(order)
                print(f"{name}: optimal gauge of robot {rec['robot']} for {rec['peer']} in round {rec['t']}: {rec['gauge']}, "
                      f"reference {order[0]} ({unc[order[0]]:.6g}; runner-up {unc[order[1]]:.6g}, {len(order)} candidates)")
                if unc[order[1]] > unc[order[0]] * (1 + 1e-6):
                    assert rec["gauge"] == order[0], (rec["gauge"], order[:3])
                gauge = rec["gauge"]
            assert rec["gauge"] == gauge, (rec["gauge"], gauge)
            worst = np.maximum(worst, _condensed_against_reference(ctx, oracle, rec, r["own"][rec["robot"]], gauge))
        except AssertionError as e:
            fails.append((rec["t"], rec["robot"], rec["peer"], str(e)[:200]))
    print(f"{name}: {len(recs)} condensed graphs (optimal gauge: {n_opt} candidates); largest est error {worst[0]:.2e}, "
          f"information {worst[1]:.2e} relative, est against the own step's labels {worst[2]:.2e}")
    assert not fails, fails
    assert r["error"] is None, r["error"]
    assert len(recs) >= 10 and any(c["optimal"] for c in recs)


def test_async_batch_and_device_exchange_steps_against_float64():
    """D: A's step check with the condensed graphs queued on the side stream and not waited for (the next solve overlaps the
    batch; the chained backward solves of both streams share the resident workgroups) and the received edges delivered and
    ingested on the device (k_wire_read, k_accept_gather_edges)."""
    from cg_mrslam_amd import Context
    nr, nv, ne, seed = 3, 900, 3000, 48
    ctxs = [Context(0) for _ in range(nr)]
    rounds = make_robot_rounds(ctxs, nv, ne, seed, chunk=90, async_condense=True)
    try:
        steps, _, _ = checked_rounds(rounds, 10, device=True)
        for rr in rounds:
            rr.g.condensed_wait()
        timeouts = [c.gn_timeouts() for c in ctxs]
    finally:
        _close(rounds, ctxs)
    _, n_recv = _check_steps("async, device exchange", steps)
    assert n_recv > len(steps) // 2 and timeouts == [0] * nr, (n_recv, timeouts)


VARIANTS = (("default", {}), ("no_top_block", {"CGMR_TOP_BLOCK": "0"}), ("separate_launches", {"CGMR_FWD_MERGE": "0"}),
            ("merge_resident_only", {"CGMR_FWD_MERGE_ANY": "0"}), ("bwd_levelwise", {"CGMR_BWD_CHAIN": "0"}),
            ("no_amalgamation", {"CGMR_AMALGAMATE": "0"}))
VARIANT_CASE = (2, 1200, 4000, 44, 120, 10)


def test_launch_variants_robot_graph_steps():
    """E: A's step check under the switches that change the factorisation's shape -- CGMR_TOP_BLOCK=0 makes the hubs'
    separator ordinary fronts -- one set of contexts at a time (a context reads them when it is created)."""
    nr, nv, ne, seed, chunk, n_rounds = VARIANT_CASE
    report = {}
    for vname, env in VARIANTS:
        with contextlib.ExitStack() as stack:
            ctxs = [stack.enter_context(context_under(env)) for _ in range(nr)]
            rounds = make_robot_rounds(ctxs, nv, ne, seed, chunk)
            try:
                steps, _, _ = checked_rounds(rounds, n_rounds)
                timeouts = [c.gn_timeouts() for c in ctxs]
            finally:
                for rr in rounds:
                    rr.g.close()
            s = steps[-1]
            assert_launch_shape(ctxs[0], env, (s["p0"],) + tuple(s[k] for k in SYSTEM_KEYS))
        assert timeouts == [0] * nr, (vname, timeouts)
        ws, n_recv = _check_steps(vname, steps)
        assert n_recv > len(steps) // 2, (vname, n_recv, len(steps))
        report[vname] = round(max(ws) / R.U, 1)
    print("largest omega / u per variant:", report)
