"""The graphs and candidate sets that tests/test_pcm_inter_cpu.py and tests/test_pcm_inter_gpu.py share: an own graph of 120
poses, a peer graph of 60, their union as two components, and inter-robot candidates with planted inliers and gross outliers.

Everything is at fixed linearisation points -- the generators' true poses moved by seeded noise --, so that the float64
reference's answers on a candidate set (test_pcm_inter_cpu.py checks what they must show) are those of the very inputs the
device gets, with no solver in between."""
import numpy as np

import ref_joint_marginals as J
from cg_mrslam_amd import synth

IU = np.array([500.0, 0, 0, 500.0, 0, 5000.0])
SEEDS = (3, 5, 6)                       # the end-to-end generators (margins: test_pcm_inter_cpu.py)
FRAME = np.array([2.0, -1.0, 0.7])        # the peer's frame in the own one; no call is told


def se2_mul(a, b):
    """a (+) b, arrays [..., 3]; theta left as the sum."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c, s = np.cos(a[..., 2]), np.sin(a[..., 2])
    return np.stack([a[..., 0] + c * b[..., 0] - s * b[..., 1], a[..., 1] + s * b[..., 0] + c * b[..., 1], a[..., 2] + b[..., 2]], axis=-1)


def _at(g, seed):
    p = g["truth"] + np.random.default_rng(seed).normal(0, 1, g["truth"].shape) * [0.05, 0.05, 0.02]
    p.setflags(write=False)
    return p


_CACHE = {}


def graphs():
    """(own graph, its poses, peer graph, its poses): computed once, never modified."""
    if "g" not in _CACHE:
        own, peer = synth.make_pose_graph(120, 300, seed=48), synth.make_pose_graph(60, 150, seed=49)
        _CACHE["g"] = (own, _at(own, 480), peer, _at(peer, 490))
    return _CACHE["g"]


def args(g):
    return g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"]


def union(own, peer, peer_all_fixed=False):
    """The two graphs as the components of one, the peer's vertices behind the own ones: (fixed, ef, et, meas, info)."""
    n = len(own["fixed"])
    fixed = np.concatenate([own["fixed"], np.ones_like(peer["fixed"]) if peer_all_fixed else peer["fixed"]])
    return (fixed, np.concatenate([own["edge_from"], peer["edge_from"] + n]).astype(np.int32),
            np.concatenate([own["edge_to"], peer["edge_to"] + n]).astype(np.int32), np.vstack([own["meas"], peer["meas"]]),
            np.vstack([own["info"], peer["info"]]))


def candidates(p_own, p_peer, seed, N=40, n_out=14):
    """N candidates from random own vertices to random peer vertices (some of either repeat): the relative pose through FRAME
    plus noise of the information IU; n_out of them, picked by a permutation, moved per coordinate by
    +-([1, 1, 0.3] + U(0, 1) [4, 4, 1.5]).  Returns (ca, pv, z, info, outliers): pv the peer vertex of every candidate."""
    rng = np.random.default_rng(seed)
    ca = rng.integers(0, len(p_own), N).astype(np.int32)
    pv = rng.integers(0, len(p_peer), N).astype(np.int32)
    z = J.relative_pose(p_own[ca], se2_mul(FRAME, p_peer[pv])) + rng.normal(0, 1, (N, 3)) / np.sqrt(IU[[0, 3, 5]])
    out = np.sort(rng.permutation(N)[:n_out])
    sign = rng.choice([-1.0, 1.0], (n_out, 3))
    z[out] += sign * (np.array([1, 1, 0.3]) + rng.random((n_out, 3)) * np.array([4, 4, 1.5]))
    return ca, pv, z, np.tile(IU, (N, 1)), out


def expand(cov, where):
    """A joint covariance of unique vertices, per candidate: candidate k takes the rows and columns of position where[k]."""
    rows = np.concatenate([np.arange(3 * int(w), 3 * int(w) + 3) for w in where])
    return np.ascontiguousarray(cov[np.ix_(rows, rows)])


def peer_cov_dense(seed):
    """The peer graph's float64 joint covariance (dense inverse of its H) of the candidates' peer vertices, per candidate."""
    key = ("pc", seed)
    if key not in _CACHE:
        own, p_own, peer, p_peer = graphs()
        pv = candidates(p_own, p_peer, seed)[1]
        uq = np.unique(pv)
        _CACHE[key] = expand(J.joint_dense(p_peer, *args(peer), uq.astype(np.int32)), np.searchsorted(uq, pv))
        _CACHE[key].setflags(write=False)
    return _CACHE[key]
