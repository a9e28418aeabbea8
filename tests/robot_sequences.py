"""Host-only C5 rounds (test infrastructure): the edge lists a robot's solver sees round after round -- own edges, appended to,
followed by the condensed stars received from the peers, replaced every round -- produced by the real ``RobotGraph`` books
(no device context) and ``RobotRounds`` with fake numerics, and the analysis of such a sequence the way a context with the
analysis cache on performs it (``cgmr_debug_symbolic_steps``).  Also the whole system a robot graph's solve sees, rebuilt
from its books and what was added to it (``RecordedGraph``, ``solved_system``), and rounds whose solves are split so that
single Gauss-Newton steps of them can be checked (``checked_rounds``)."""
import ctypes as C

import numpy as np

from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import load_library
from cg_mrslam_amd.condensed import RobotGraph
from cg_mrslam_amd.mrslam import LoopbackExchange, RobotRounds, RobotWorld

SYM_KEYS = ["free_poses", "offdiag_blocks", "fronts", "levels", "L_doubles", "U_doubles", "max_border", "factor_flops",
            "order_us", "structure_us"]


def robot_sequences(n_robots, n_vertices, n_edges, seed, n_rounds=None, chunk=50):
    """Per robot: [(nV, ef, et, n_own, hub vertices)] after every round's grow (what the round's optimize analyses)."""
    R = synth.make_multi_robot(n_robots, n_vertices, n_edges, seed=seed)
    rounds = [RobotRounds(RobotGraph(None, r, n_robots, cap_edges=128), RobotWorld(R, r, chunk=chunk)) for r in range(n_robots)]

    def fake_condense(g):
        for p in range(n_robots):
            want = g.closures(p, "out") if p != g.robot else []
            if len(want) >= 2:
                k = len(want) // 2                      # the gauge moves as the set grows (the centroid does)
                rest = np.concatenate([want[:k], want[k + 1:]])
                n = len(rest)
                g.set_condensed(p, want[k], rest, np.zeros((n, 3), np.float32),
                                np.tile(np.array([100, 0, 0, 100, 0, 1000], np.float32), (n, 1)))
    ex = LoopbackExchange([r.g for r in rounds])
    seq = [[] for _ in range(n_robots)]
    cap = 8 * n_edges + 4096
    for _ in range(rounds[0].w.n_rounds if n_rounds is None else n_rounds):
        for rr in rounds:
            rr.grow()
            g = rr.g
            ef, et = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            nown = C.c_int32(0)
            n = g.lib.cgmr_graph_debug_edges(g.h, C.c_int(cap), C.c_void_p(ef.ctypes.data), C.c_void_p(et.ctypes.data), C.byref(nown))
            assert 0 <= n <= cap
            seq[g.robot].append((g.counts()["vertices"], ef[:n].copy(), et[:n].copy(), nown.value,
                                 np.unique(ef[nown.value:n]).astype(np.int32)))
        ex.finish_all()
        for rr in rounds:
            fake_condense(rr.g)
        ex.start_all()
    return seq


def run_steps(steps, use_hubs=True):
    """(info of the last analysis, its permutation, steps that extended the ordering, front table, per-step
    [levels, extended, ordering us, structure us, flops])."""
    lib = load_library()
    nV = np.array([s[0] for s in steps], np.int32)
    e_ptr, h_ptr = np.zeros(len(steps) + 1, np.int32), np.zeros(len(steps) + 1, np.int32)
    for k, s in enumerate(steps):
        e_ptr[k + 1] = e_ptr[k] + len(s[1])
        h_ptr[k + 1] = h_ptr[k] + (len(s[4]) if use_hubs else 0)
    ef = np.concatenate([s[1] for s in steps]).astype(np.int32)
    et = np.concatenate([s[2] for s in steps]).astype(np.int32)
    hubs = np.concatenate([s[4] for s in steps] + [np.zeros(1, np.int32)]).astype(np.int32)
    out, perm, next_ = np.zeros(16, np.int64), np.zeros(int(nV[-1]), np.int32), C.c_int32(0)
    fr, per = np.zeros(6 * 60000, np.int32), np.zeros(5 * len(steps), np.int64)
    P = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    n = lib.cgmr_debug_symbolic_steps(C.c_int(len(steps)), P(nV), P(e_ptr), P(ef), P(et), P(h_ptr), P(hubs), P(out), P(perm),
                                      C.byref(next_), C.c_int(60000), P(fr), P(per))
    assert 0 <= n <= 60000
    return dict(zip(SYM_KEYS, out.tolist())), perm, int(next_.value), fr[:6 * n].reshape(n, 6), per.reshape(-1, 5)


class RecordedGraph:
    """A ``RobotGraph`` (or any object with its interface) that records its own vertices and edges in call order: ids, fixed
    flags, end points as vertex indices, measurements and information as given.  Everything else goes to the graph."""

    def __init__(self, graph):
        self.g = graph
        self.index = {}                     # vertex id -> vertex index (the order of add_vertices)
        self.fixed = []
        self.own_ef, self.own_et, self.own_meas, self.own_info = [], [], [], []

    def __getattr__(self, name):
        return getattr(self.g, name)

    def add_vertices(self, ids, poses, fixed=None):
        self.g.add_vertices(ids, poses, fixed)
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        for i in ids.tolist():
            self.index[i] = len(self.index)
        self.fixed.extend([0] * len(ids) if fixed is None else np.asarray(fixed, dtype=np.uint8).reshape(-1).tolist())

    def add_edges(self, from_ids, to_ids, meas, info):
        self.g.add_edges(from_ids, to_ids, meas, info)
        self.own_ef.extend(self.index[int(i)] for i in np.asarray(from_ids).reshape(-1))
        self.own_et.extend(self.index[int(i)] for i in np.asarray(to_ids).reshape(-1))
        self.own_meas.append(np.array(meas, dtype=np.float64).reshape(-1, 3))
        self.own_info.append(np.array(info, dtype=np.float64).reshape(-1, 6))

    def own_system(self):
        """(fixed, ef, et, meas, info) of the recorded vertices and own edges."""
        return (np.array(self.fixed, np.uint8), np.array(self.own_ef, np.int32), np.array(self.own_et, np.int32),
                np.concatenate(self.own_meas + [np.zeros((0, 3))]), np.concatenate(self.own_info + [np.zeros((0, 6))]))


def debug_edges(g):
    """(ef, et, n_own) of ``cgmr_graph_debug_edges``: the edge list the solver sees, own edges first."""
    n = g.lib.cgmr_graph_debug_edges(g.h, C.c_int(0), None, None, None)
    assert n >= 0
    ef, et = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    nown = C.c_int32(0)
    m = g.lib.cgmr_graph_debug_edges(g.h, C.c_int(n), C.c_void_p(ef.ctypes.data), C.c_void_p(et.ctypes.data), C.byref(nown))
    assert m == n
    return ef[:n].copy(), et[:n].copy(), int(nown.value)


def solved_system(rg):
    """The system ``cgmr_graph_optimize`` of the RecordedGraph ``rg`` solves now: dict(fixed, ef, et, meas, info, n_own, hubs).
    ef / et are the books' (``debug_edges``: own edges, then received ones); the own part must be the recorded adds index for
    index, with their measurements and information; the received part takes its values from ``received_edges(peer)`` (the
    float32-rounded doubles of the device's staging), matched by (from, to) one to one.  hubs: the received stars' gauge
    vertices in the order the solve names them to the analysis (first appearance in the received part)."""
    g = rg.g
    fixed, own_ef, own_et, own_meas, own_info = rg.own_system()
    assert g.counts()["vertices"] == len(fixed)
    ef, et, n_own = debug_edges(g)
    assert n_own == len(own_ef)
    assert np.array_equal(ef[:n_own], own_ef) and np.array_equal(et[:n_own], own_et)
    held = {}
    for p in range(g.n_robots):
        f, t, m, i = g.received_edges(p)
        for k in range(len(f)):
            key = (rg.index[int(f[k])], rg.index[int(t[k])])
            assert key not in held, ("two received edges join", key)
            held[key] = (m[k], i[k])
    recv = list(zip(ef[n_own:].tolist(), et[n_own:].tolist()))
    assert len(recv) == len(held) and set(recv) == set(held), "received edges of the books and of received_edges() differ"
    meas = np.concatenate([own_meas] + [held[k][0][None] for k in recv])
    info = np.concatenate([own_info] + [held[k][1][None] for k in recv])
    hubs = list(dict.fromkeys(ef[n_own:].tolist()))
    return dict(fixed=fixed, ef=ef, et=et, meas=meas, info=info, n_own=n_own, hubs=np.array(hubs, np.int32))


def checked_rounds(rounds, n_rounds, device=False, iters=5, third_every=3, optimal=None, record_condensed=False, out=None):
    """``rounds``: RobotRounds over RecordedGraphs.  The lock-step order of ``mrslam.run_rounds_loopback``, with each robot's
    ``optimize(iters)`` split: one step from the grown graph, and in every ``third_every``-th round one step from the 3rd
    iterate, each recorded with its system.  optimal = (round, robot): that robot builds that round's condensed graphs with
    the optimal gauge.  Returns (steps, sequences, condensed):
      steps       dicts: t, robot, start (iterate the step starts from), p0, p1 and ``solved_system``'s entries
      sequences   per robot, per round: (nV, ef, et, n_own, hubs) as the solve analysed them (``run_steps`` replays them)
      condensed   (record_condensed) dicts: t, robot, peer, poses, n_own (own edges then), want (the requested vertices),
                  optimal, and the result: gauge, to (vertex indices), est, iu -- for every condensed graph built in a round in
                  which the robot held received edges
    out (a dict, optional) gets the three lists as they fill up: what was recorded before a round failed."""
    ex = LoopbackExchange([rr.g for rr in rounds], device=device)
    steps, seqs, conds = [], [[] for _ in rounds], []
    if out is not None:
        out.update(steps=steps, seqs=seqs, conds=conds)
    for t in range(n_rounds):
        for rr in rounds:
            rr.grow()
            g = rr.g
            sysm = solved_system(g)
            seqs[g.robot].append((len(sysm["fixed"]), sysm["ef"], sysm["et"], sysm["n_own"], sysm["hubs"]))
            plan = [(0, 1)] + ([(1, 2), (3, 1)] if third_every and t % third_every == third_every - 1 else [])
            done = 0
            for start, n in plan:
                p0 = g.poses()
                rc, _ = g.optimize(n)
                assert rc == 0, (t, g.robot, rc)
                if n == 1:
                    steps.append(dict(t=t, robot=g.robot, start=start, p0=p0, p1=g.poses(), **sysm))
                done += n
            rc, rr.last_chi2 = g.optimize(iters - done)
            assert rc == 0, (t, g.robot, rc)
        ex.finish_all()
        for rr in rounds:
            g = rr.g
            opt = optimal == (t, g.robot)
            if opt:
                g.set_optimal_gauge(True)
            rr.condense()
            if opt:
                g.set_optimal_gauge(False)
            if record_condensed and g.counts()["received_edges"] > 0:
                poses = g.poses()
                for p in range(g.n_robots):
                    want = g.closures(p, "out") if p != g.robot else []
                    if len(want) >= 2:
                        gid, to, est, iu = g.condensed(p)
                        conds.append(dict(t=t, robot=g.robot, peer=p, poses=poses, n_own=len(g.own_ef), optimal=opt,
                                          want=np.array([g.index[int(i)] for i in want], np.int32),
                                          gauge=None if gid is None else g.index[gid],
                                          to=np.array([g.index[int(i)] for i in to], np.int32), est=est, iu=iu))
        ex.start_all()
    ex.finish_all()
    return steps, seqs, conds


def make_robot_rounds(ctxs, n_vertices, n_edges, seed, chunk, async_condense=False):
    """One RobotRounds over a RecordedGraph per context (one context per robot: each robot's analysis cache sees its own
    sequence only, as with one rank per robot) on ``synth.make_multi_robot(len(ctxs), n_vertices, n_edges, seed)``."""
    nr = len(ctxs)
    R = synth.make_multi_robot(nr, n_vertices, n_edges, seed=seed)
    return [RobotRounds(RecordedGraph(RobotGraph(ctxs[r], r, nr, cap_edges=128, async_condense=async_condense)),
                        RobotWorld(R, r, chunk=chunk)) for r in range(nr)]
