"""Robot graphs with corrupted closures for graduated non-convexity on the resident graph (include/cgmr.h:
cgmr_graph_optimize_gnc) -- TEST INFRASTRUCTURE ONLY.

Every case is a deterministic recipe built through ``RecordedGraph`` over ``RobotGraph``, with or without a device context:
robot 0's own vertices walk a boustrophedon over a 1 m grid (odometry chain: known inliers; closures between neighbouring
rows: free), the peers' vertices it has met lie beside the path, each the end of a true inter-robot closure.  Every peer's
condensed star comes from a host-only sender graph of that peer -- ``set_condensed`` from ground truth narrowed to float32
with a fixed information, as ``robot_sequences.fake_condense`` does, then ``message_for`` / ``message_from`` -- so the books
and the numbers are the same with and without a device.  ``robot_sequences.solved_system`` then gives the reference its
system.

  pair     two robots: 120 own vertices, 6 peer vertices, 261 own edges (the linearisation's second workgroup holds 5 + the
           received 5), three own closures and one inter-robot closure grossly corrupted, one received star edge corrupted
  trio     three robots (two peers, two stars, a condensed batch of two jobs), corrupted as pair, one star edge per peer
  clean    pair without a corrupted edge: nothing to reject
  starved  a chain of eight poses and a lone vertex whose only two edges, from the same pose and with the same information,
           place it 15 m ahead and 15 m behind: TLS ends with both at weight 0
"""
import numpy as np

from cg_mrslam_amd import synth
from cg_mrslam_amd.condensed import RobotGraph
from robot_sequences import RecordedGraph, solved_system

import ref_gnc

INFO = np.array([100.0, 0.0, 0.0, 100.0, 0.0, 1000.0])      # sigma 0.1 m, 0.0316 rad
NOISE = 0.2                                                 # measurement noise, in sigmas of INFO
START = np.array([0.02, 0.02, 0.005])                       # the initial estimates: truth + N(0, START)
PEER_BASE = 20000                                           # ids of peer p's vertices: p * PEER_BASE + k


def _rel(a, b):
    return synth.se2_compose(synth.se2_inverse(np.asarray(a, dtype=np.float64)), np.asarray(b, dtype=np.float64))


def _truth(n, cols=12):
    """n poses along a boustrophedon of `cols` columns, 1 m apart, heading along the path."""
    p = np.zeros((n, 3))
    for k in range(n):
        r, c = divmod(k, cols)
        p[k, 0] = c if r % 2 == 0 else cols - 1 - c
        p[k, 1] = r
    d = np.diff(p[:, :2], axis=0)
    p[:-1, 2] = np.arctan2(d[:, 1], d[:, 0])
    p[-1, 2] = p[-2, 2]
    return p


class _Case:
    """What a built case holds: rg (the RecordedGraph), poses0, truth, n_own, the system of solved_system() (sys), bad (indices
    of the corrupted edges in the system's order, the received ones included), bad_own (those among the own edges), known / barc_sq
    [nE] as the graph was told, peers (ids of the peers with a star) and want (peer -> my vertex ids that peer asks for)."""


def _build(ctx, n_robots, n_own, n_peer, n_closures, seed, corrupt):
    rng = np.random.default_rng(seed)
    sig = 1.0 / np.sqrt(INFO[[0, 3, 5]])
    truth_own = _truth(n_own)
    ids_own = 100 + np.arange(n_own)
    peers = list(range(1, n_robots))
    # the peers' vertices: beside own vertices spread along the path, 0.4 m off the grid
    truth_peer, ids_peer, anchor = {}, {}, {}
    for p in peers:
        anchor[p] = np.linspace(5 + 3 * p, n_own - 7 - 2 * p, n_peer).astype(int)
        t = truth_own[anchor[p]].copy()
        t[:, 0] += 0.4
        t[:, 1] += 0.3 * (1 if p % 2 else -1)
        t[:, 2] = synth.normalize_theta(t[:, 2] + 0.5 * p)
        truth_peer[p] = t
        ids_peer[p] = p * PEER_BASE + np.arange(n_peer)
    truth = np.concatenate([truth_own] + [truth_peer[p] for p in peers])
    ids = np.concatenate([ids_own] + [ids_peer[p] for p in peers])
    index = {int(i): k for k, i in enumerate(ids)}
    poses0 = truth + rng.normal(size=truth.shape) * START
    poses0[:, 2] = synth.normalize_theta(poses0[:, 2])
    poses0[0] = truth[0]
    fixed = np.zeros(len(ids), np.uint8)
    fixed[0] = 1

    ef, et, known = [], [], []
    for k in range(n_own - 1):                                   # the odometry chain: known inliers
        ef.append(k); et.append(k + 1); known.append(1)
    # true closures between neighbouring rows (at most 1.5 m apart, not chain neighbours), drawn without repetition
    cand = [(i, j) for i in range(n_own) for j in range(i + 2, n_own)
            if np.hypot(*(truth_own[i, :2] - truth_own[j, :2])) <= 1.5]
    for q in rng.permutation(len(cand))[:n_closures]:
        ef.append(cand[q][0]); et.append(cand[q][1]); known.append(0)
    for p in peers:                                              # every peer vertex ends a true inter-robot closure
        for k in range(n_peer):
            ef.append(int(anchor[p][k])); et.append(index[int(ids_peer[p][k])]); known.append(0)
    ef, et = np.array(ef), np.array(et)
    meas = _rel(truth[ef], truth[et]) + rng.normal(size=(len(ef), 3)) * sig * NOISE
    bad_own = []
    if corrupt:
        # gross errors: three own closures across the map and one inter-robot closure onto a vertex of peer 1's star
        extra = [(7, n_own - 9), (n_own // 2 + 3, 4), (n_own - 20, 30), (int(anchor[1][2]) + 5, index[int(ids_peer[1][4])])]
        wrong = np.array([[3.0, -2.0, 1.2], [-4.0, 1.5, -2.0], [2.5, 3.5, 0.8], [-3.0, -2.5, 2.4]])
        bad_own = list(range(len(ef), len(ef) + len(extra)))
        ef = np.r_[ef, [a for a, _ in extra]]
        et = np.r_[et, [b for _, b in extra]]
        meas = np.concatenate([meas, _rel(truth[ef[bad_own]], truth[et[bad_own]]) + wrong])
        known += [0] * len(extra)
    meas[:, 2] = synth.normalize_theta(meas[:, 2])
    info = np.tile(INFO, (len(ef), 1))
    known = np.array(known, np.uint8)

    rg = RecordedGraph(RobotGraph(ctx, 0, n_robots))
    rg.add_vertices(ids, poses0, fixed)
    rg.add_edges(ids[ef], ids[et], meas, info)
    rg.set_edge_gnc(None, known)
    # the received stars: gauge = the peer's first vertex, true relative poses narrowed to float32, one corrupted per peer
    bad_recv = []
    for p in peers:
        sender = RobotGraph(None, p, n_robots)
        try:
            sender.add_vertices(ids_peer[p], truth_peer[p])
            est = _rel(truth_peer[p][0], truth_peer[p][1:])
            if corrupt:
                est[1 + p % 2] += [2.0, -3.0, 1.5]
                bad_recv.append((index[int(ids_peer[p][0])], index[int(ids_peer[p][2 + p % 2])]))
            sender.set_condensed(0, ids_peer[p][0], ids_peer[p][1:], est.astype(np.float32), np.tile(INFO, (n_peer - 1, 1)).astype(np.float32))
            msg = sender.message_for(0)
            assert msg is not None and rg.message_from(msg) == n_peer - 1
        finally:
            sender.close()
    c = _Case()
    c.rg, c.poses0, c.truth, c.ids, c.n_own, c.peers = rg, poses0, truth, ids, len(ef), peers
    c.want = {}
    for p in peers:                                              # peer p asks for my ends of its closures (and one more vertex)
        c.want[p] = np.unique(np.r_[ids_own[anchor[p]], ids_own[3 + p]])
        rg.insertOutClosure(p, c.want[p])
    c.sys = solved_system(rg)
    nE = len(c.sys["ef"])
    recv = list(zip(c.sys["ef"][c.n_own:].tolist(), c.sys["et"][c.n_own:].tolist()))
    c.bad_own = np.array(bad_own, np.int64)
    c.bad = np.sort(np.r_[c.bad_own, [c.n_own + recv.index(k) for k in bad_recv]]).astype(np.int64)
    c.known = np.r_[known, np.zeros(nE - c.n_own, np.uint8)]
    c.barc_sq = np.full(nE, ref_gnc.QUANTILE[3])
    return c


def pair(ctx=None):
    return _build(ctx, 2, 120, 6, 132, 51, True)


def trio(ctx=None):
    return _build(ctx, 3, 120, 5, 128, 12, True)


def clean(ctx=None):
    return _build(ctx, 2, 120, 6, 132, 51, False)


def starved(ctx=None):
    """Eight poses in a row with three closures, two peer vertices, and a lone vertex hung on pose 3 by two edges that contradict
    each other symmetrically; it starts on pose 3, in the middle: both edges keep the same r = 100 * 15^2 at every outer
    iteration, the largest of the graph, and TLS gives both weight 0 in the same one."""
    n_own = 8
    truth = np.zeros((n_own + 3, 3))
    truth[:n_own, 0] = np.arange(n_own)
    truth[n_own] = [3.0, 0.0, 0.0]                               # the lone vertex: on pose 3
    truth[n_own + 1] = [2.0, 0.6, 0.3]                           # the peer's two vertices
    truth[n_own + 2] = [5.0, -0.6, -0.2]
    ids = np.r_[100 + np.arange(n_own + 1), PEER_BASE, PEER_BASE + 1]
    rng = np.random.default_rng(13)
    sig = 1.0 / np.sqrt(INFO[[0, 3, 5]])
    poses0 = truth + rng.normal(size=truth.shape) * START
    poses0[0] = truth[0]
    lone = n_own
    fixed = np.zeros(len(ids), np.uint8)
    fixed[0] = 1
    ef = np.r_[np.arange(n_own - 1), [0, 2, 4], [2, 5]]
    et = np.r_[np.arange(1, n_own), [2, 4, 7], [n_own + 1, n_own + 2]]
    known = np.r_[np.ones(n_own - 1, np.uint8), np.zeros(5, np.uint8)]
    meas = _rel(truth[ef], truth[et]) + rng.normal(size=(len(ef), 3)) * sig * NOISE
    ef, et = np.r_[ef, [3, 3]], np.r_[et, [lone, lone]]
    meas = np.concatenate([meas, [[15.0, 0.0, 0.0], [-15.0, 0.0, 0.0]]])
    known = np.r_[known, [0, 0]].astype(np.uint8)
    poses0[lone] = poses0[3]                                     # (the middle, exactly)
    rg = RecordedGraph(RobotGraph(ctx, 0, 2))
    rg.add_vertices(ids, poses0, fixed)
    rg.add_edges(ids[ef], ids[et], meas, np.tile(INFO, (len(ef), 1)))
    rg.set_edge_gnc(None, known)
    sender = RobotGraph(None, 1, 2)
    try:
        sender.add_vertices(ids[-2:], truth[-2:])
        sender.set_condensed(0, ids[-2], ids[-1:], _rel(truth[-2], truth[-1:]).astype(np.float32), INFO[None].astype(np.float32))
        assert rg.message_from(sender.message_for(0)) == 1
    finally:
        sender.close()
    c = _Case()
    c.rg, c.poses0, c.truth, c.ids, c.n_own, c.peers, c.want, c.lone = rg, poses0, truth, ids, len(ef), [1], {}, lone
    c.sys = solved_system(rg)
    nE = len(c.sys["ef"])
    c.bad_own = np.array([len(ef) - 2, len(ef) - 1], np.int64)
    c.bad = c.bad_own
    c.known = np.r_[known, np.zeros(nE - c.n_own, np.uint8)]
    c.barc_sq = np.full(nE, ref_gnc.QUANTILE[3])
    return c


BUILD = {"pair": pair, "trio": trio, "clean": clean, "starved": starved}
_HOST, _REF = {}, {}


def build(name, ctx=None):
    """The case on a graph of its own (close ``case.rg`` when done): host-only without a context."""
    return BUILD[name](ctx)


def host_case(name):
    """The case on a host-only graph, built once (not to be modified)."""
    if name not in _HOST:
        _HOST[name] = build(name)
    return _HOST[name]


def args(c):
    s = c.sys
    return c.poses0, s["fixed"], s["ef"], s["et"], s["meas"], s["info"]


def reference(name, loss, **params):
    """ref_gnc.gnc_optimize on the host-only case's solved system, computed once per (case, loss, parameters)."""
    key = (name, loss, tuple(sorted(params.items())))
    if key not in _REF:
        c = host_case(name)
        _REF[key] = ref_gnc.gnc_optimize(*args(c), loss=loss, barc_sq=c.barc_sq, known=c.known, **params)
    return _REF[key]
