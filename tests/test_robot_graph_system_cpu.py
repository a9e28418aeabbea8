"""The rebuilt system of a robot graph (robot_sequences.solved_system), on host-only rounds (no device context): the received part
is exactly the stars the peers sent -- in the books' order, with the float32 values of the wire -- filtered to the edges whose end
points the receiver knows, the newest non-empty set per peer; the hubs are the stars' gauge vertices; a received edge the getter
does not report is an error, not a smaller system."""
import numpy as np
import pytest

from cg_mrslam_amd import synth
from cg_mrslam_amd.condensed import RobotGraph
from cg_mrslam_amd.mrslam import LoopbackExchange, RobotRounds, RobotWorld
from robot_sequences import RecordedGraph, solved_system


def _fake_star(rng, n):
    """Distinct per-edge values (a mixed-up slot or information entry changes the system), float32 as on the wire."""
    est = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    d = rng.uniform(10, 1000, (n, 3))
    off = rng.uniform(-1, 1, (n, 3))
    info = np.stack([d[:, 0], off[:, 0], off[:, 1], d[:, 1], off[:, 2], d[:, 2]], axis=1).astype(np.float32)
    return est, info


def test_solved_system_is_the_books_edge_lists_with_the_sent_values():
    nr, chunk, n_rounds = 3, 50, 12
    R = synth.make_multi_robot(nr, 900, 3000, seed=48)
    rounds = [RobotRounds(RecordedGraph(RobotGraph(None, r, nr, cap_edges=128)), RobotWorld(R, r, chunk=chunk)) for r in range(nr)]
    graphs = [rr.g for rr in rounds]
    ex = LoopbackExchange(graphs)
    rng = np.random.default_rng(5)
    sent = {}          # (sender, receiver) -> (gauge id, to ids, est, info) of the sender's last message
    held = {}          # (receiver, sender) -> [(from id, to id, est, info)] the receiver should hold
    checked = recv_rounds = 0
    for t in range(n_rounds):
        for rr in rounds:
            rr.grow()
            g = rr.g
            s = solved_system(g)
            n_own = s["n_own"]
            f0, t0, m0, i0 = g.own_system()[1:]
            assert np.array_equal(s["ef"][:n_own], f0) and np.array_equal(s["meas"][:n_own], m0)
            assert np.array_equal(s["et"][:n_own], t0) and np.array_equal(s["info"][:n_own], i0)
            want = [e for q in range(nr) for e in held.get((g.robot, q), [])]        # peer order, star order
            assert len(s["ef"]) == n_own + len(want)
            for k, (fid, tid, est, info) in enumerate(want):
                assert (s["ef"][n_own + k], s["et"][n_own + k]) == (g.index[fid], g.index[tid])
                assert np.array_equal(s["meas"][n_own + k], est.astype(np.float64))
                assert np.array_equal(s["info"][n_own + k], info.astype(np.float64))
            gauges = [g.index[held[(g.robot, q)][0][0]] for q in range(nr) if held.get((g.robot, q))]
            assert s["hubs"].tolist() == gauges
            assert np.array_equal(np.sort(s["hubs"]), np.unique(s["ef"][n_own:]))     # robot_sequences' hub set
            assert s["fixed"][0] == 1 and s["fixed"].sum() == 1                           # the robot's first vertex, as added
            checked += 1
            recv_rounds += len(want) > 0
        # ingest: what every peer sent last round, edges whose end points the receiver knows; an empty set changes nothing
        ex.finish_all()
        for (q, r), (gid, to, est, info) in sent.items():
            known = graphs[r].index
            keep = [(gid, int(v), est[k], info[k]) for k, v in enumerate(to) if gid in known and int(v) in known]
            if keep:
                held[(r, q)] = keep
        sent = {}
        for g in graphs:
            for p in range(nr):
                want = g.closures(p, "out") if p != g.robot else []
                if len(want) >= 2:
                    k = len(want) // 2
                    rest = np.concatenate([want[:k], want[k + 1:]])
                    est, info = _fake_star(rng, len(rest))
                    g.set_condensed(p, want[k], rest, est, info)
                    sent[(g.robot, p)] = (int(want[k]), rest, est, info)
        ex.start_all()
    assert checked == nr * n_rounds and recv_rounds >= nr * n_rounds // 2
    assert sum(len(v) for v in held.values()) > 50

    class Dropping:                      # a getter that misses one received edge: the rebuilt system must not shrink with it
        def __init__(self, g):
            self.g = g

        def __getattr__(self, name):
            return getattr(self.g, name)

        def received_edges(self, peer):
            f, t, m, i = self.g.received_edges(peer)
            return (f[1:], t[1:], m[1:], i[1:]) if len(f) else (f, t, m, i)

    rg = graphs[0]
    rg.g = Dropping(rg.g)
    with pytest.raises(AssertionError):
        solved_system(rg)
