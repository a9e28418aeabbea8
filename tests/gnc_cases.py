"""The graphs the graduated non-convexity checks run on (tests/test_gnc_cpu.py, tests/test_gnc_gpu.py): deterministic builders,
each with the set of edges it corrupted, and the reference's result on each, computed once per process.  TEST INFRASTRUCTURE ONLY.

A case is a dict: poses, fixed, edge_from, edge_to, meas, info, vk / ek (None for a pure pose graph), known (uint8 [nE]), barc_sq
(scalar, or None for the dimension default), bad (sorted indices of the corrupted edges), inner_iters."""
import numpy as np

import ref_gnc
import ref_robust
import ref_typed
import typed_cases

KEYS = ("poses", "fixed", "edge_from", "edge_to", "meas", "info")
MARGIN = 1e-6          # every free edge's r stays this far (in units of c) from lo and up at every outer iteration


def args(g):
    return tuple(g[k] for k in KEYS)


def hand():
    """Pose 0 fixed at the origin, pose 1 started at (1, 0, 0); three edges 0 -> 1 with unit information: the odometry (a
    known inlier) and a closure measuring (1, 0, 0), and a gross outlier measuring (4, 0, 0).  c = 1.  At the start r = (0, 0, 9):
        mu0 = c / (2 r - c) = 1 / 17
        up = (mu0 + 1) / mu0 = 18, lo = 1 / 18:  w = (1, 1, sqrt((1/17)(18/17) / 9) - 1/17) = (1, 1, (sqrt 2 - 1) / 17)
    and since up falls towards c = 1 while the outlier's r stays near 9, it ends with weight 0: the final weights are (1, 1, 0)
    and pose 1 is back at (1, 0, 0)."""
    I = [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    return dict(poses=np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), fixed=np.array([1, 0], np.uint8),
                edge_from=np.zeros(3, np.int32), edge_to=np.ones(3, np.int32),
                meas=np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [4.0, 0.0, 0.0]]), info=np.array([I, I, I]), vk=None, ek=None,
                known=np.array([1, 0, 0], np.uint8), barc_sq=1.0, bad=np.array([2]), inner_iters=1,
                mu0=1.0 / 17.0, w_first=np.array([1.0, 1.0, 0.024365503669005598]), w_final=np.array([1.0, 1.0, 0.0]))


def og(nV, nE, frac):
    """ref_robust.outlier_graph's recipe (seed 7, rng seed 1), the odometry chain as known inliers, barc^2 = 21.1."""
    g, bad, closure = ref_robust.outlier_graph(nV=nV, nE=nE, seed=7, frac=frac, rng_seed=1)
    return dict({k: g[k] for k in KEYS}, vk=None, ek=None, known=(~closure).astype(np.uint8), barc_sq=21.1, bad=np.sort(bad),
                inner_iters=1)


def _obs_r(g, k, p):
    """r of the landmark observation k were it attached to point p, at the case's initial estimates."""
    xi, l, z, u = g["poses"][g["edge_from"][k]], g["poses"][p], g["meas"][k], g["info"][k]
    c, s = np.cos(xi[2]), np.sin(xi[2])
    dx, dy = l[0] - xi[0], l[1] - xi[1]
    e0, e1 = c * dx + s * dy - z[0], -s * dx + c * dy - z[1]
    return u[0] * e0 * e0 + 2 * u[1] * e0 * e1 + u[3] * e1 * e1


GROSS = 1e3            # a re-attached observation starts with r above this (the 0.99 quantile of two dimensions is 9.2)


def _reattach(g, frac, seed, last, barc_sq, spread=False, gross=GROSS, free_every=1):
    """A ``frac``-th of the landmark observations of a typed case re-attached to a wrong landmark (the edge's ``to`` changes, its
    measurement stays), one that makes it a gross outlier at the initial estimates (r >= ``gross``); with ``last`` the last edge is
    one of them, attached to the landmark that gives it the largest r, and the others stay below 0.9 of that.  Priors and
    pose-pose edges are known inliers.  ``spread``: no landmark loses more than one observation.  ``free_every``: of the
    untouched observations every ``free_every``-th stays free, the others are known inliers too."""
    rng = np.random.default_rng(seed)
    ek, vk = g["ek"], g["vk"]
    et = g["edge_to"].copy()
    nE = len(ek)
    obs = np.flatnonzero(ek == 1)
    points = np.flatnonzero(vk == 1)
    cap = np.inf
    pool = rng.permutation(obs[obs != nE - 1] if last else obs)
    if spread:                                              # at most one observation taken from any landmark
        pool = pool[np.unique(et[pool], return_index=True)[1]]
        pool = rng.permutation(pool)
    bad = pool[:len(obs) // frac - (1 if last else 0)]
    if last:
        assert ek[nE - 1] == 1
        wrong = points[points != et[nE - 1]]
        rs = np.array([_obs_r(g, nE - 1, p) for p in wrong])
        et[nE - 1] = wrong[int(np.argmax(rs))]
        cap = 0.9 * float(rs.max())
    for k in bad:
        wrong = points[points != et[k]]
        if len(wrong) > 64:                                 # (a large case: a sample of the landmarks is enough)
            wrong = rng.choice(wrong, 64, replace=False)
        rs = np.array([_obs_r(g, k, p) for p in wrong])
        ok = wrong[(rs >= gross) & (rs < cap)]
        assert len(ok) > 0
        et[k] = rng.choice(ok)
    if last:
        bad = np.append(bad, nE - 1)
    known = np.ones(nE, np.uint8)
    known[obs[::free_every]] = 0
    known[bad] = 0
    return dict({k: g[k] for k in KEYS}, edge_to=et, vk=vk, ek=ek, known=known, barc_sq=barc_sq, inner_iters=1, bad=np.sort(bad))


MIXED_SEED = {255: 32, 256: 33, 257: 33}       # the first seeds from 31 on that meet test_gnc_cpu.py's predicates
TREE_SEED = 34                                   # the first seed from 32 on that meets them, for TLS and GM


def mixed_x(n_edges):
    return _reattach(typed_cases.mixed(n_edges, 1), 10, MIXED_SEED[n_edges], True, MIXED_BARC)


def tree600x():
    return _reattach(typed_cases.tree600(), 10, TREE_SEED, False, TREE_BARC, spread=True, gross=1e4, free_every=5)


def clean(typed):
    """Nothing to reject: the uncorrupted graph with a barc^2 no residual comes near."""
    if typed:
        g = typed_cases.mixed(255, 0)
        return dict({k: g[k] for k in KEYS}, vk=g["vk"], ek=g["ek"], known=(g["ek"] >= 3).astype(np.uint8), barc_sq=1e9,
                    bad=np.zeros(0, np.int64), inner_iters=2)
    g, _, closure = ref_robust.outlier_graph(nV=60, nE=257, seed=7, frac=10 ** 6, rng_seed=1)
    return dict({k: g[k] for k in KEYS}, vk=None, ek=None, known=(~closure).astype(np.uint8), barc_sq=1e9,
                bad=np.zeros(0, np.int64), inner_iters=2)


def starved():
    """A chain of eight poses (odometry: known inliers), three landmarks seen consistently and one whose only two observations,
    both from pose 2 and with the same information, place it at (15, 0) and at (-15, 0) of that pose's frame.  The landmark sits
    in the middle, both edges keep the same r = 300 * 15^2 = 67500 -- the largest of the graph, so mu0 = c / (2 r - c) and
    up = 2 r, 1.43 r, 1.02 r, 0.73 r at t = 0 .. 3 -- and at t = 3 TLS gives both weight 0: the landmark's block is zero."""
    b = typed_cases._Builder(41)
    P = b.trajectory(8)
    b.fixed[P[0]] = 1
    for k in range(7):
        b.odom(P[k], P[k + 1])
    for k in (1, 3, 5):
        l = b.point(*(np.array(b.truth[P[k]][:2]) + b.rng.uniform(-2, 2, 2)))
        for q in (k - 1, k, k + 1):
            b.observe(P[q], l)
    lone = b.point(2.0, 3.0)
    for z0 in (15.0, -15.0):
        b._edge(P[2], lone, [z0, 0.0, 5.0], [300.0, 0.0, 7.0, 300.0, -3.0, 11.0], 1)
    g = b.build()
    g["poses"][lone, :2] = g["poses"][P[2], :2]              # (the middle, exactly: both start with the same r)
    nE = len(g["ek"])
    return dict({k: g[k] for k in KEYS}, vk=g["vk"], ek=g["ek"], known=(g["ek"] != 1).astype(np.uint8), barc_sq=None,
                bad=np.array([nE - 2, nE - 1]), inner_iters=1, lone=lone)


MIXED_BARC = None      # the dimension default: the predicates of test_gnc_cpu.py hold with it on these cases
TREE_BARC = 21.1       # (og's value: with the default and one step per mu the reference rejects true inliers here)

CASES = {
    "hand": hand,
    "og60": lambda: og(60, 257, 4),
    "og300": lambda: og(300, 1200, 5),
    "mixed255": lambda: mixed_x(255),
    "mixed256": lambda: mixed_x(256),
    "mixed257": lambda: mixed_x(257),
    "tree600x": tree600x,
    "clean": lambda: clean(False),
    "clean_typed": lambda: clean(True),
    "starved": starved,
}
REJECTING = ("hand", "og60", "og300", "mixed255", "mixed256", "mixed257", "tree600x")     # cases that end with the corrupted set rejected
GM_CASES = ("og60", "og300", "mixed255", "mixed256", "mixed257", "tree600x")             # every corrupted edge ends below 1e-3
BOUNDARY = ("mixed255", "mixed256", "mixed257")                                            # the extreme of mu0 on the last edge

_BUILT, _REF = {}, {}


def case(name):
    """The case's graph, built once (callers must not modify it)."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def reference(name, loss, **params):
    """ref_gnc.gnc_optimize's result on the case, computed once per (case, loss, parameters); not to be modified."""
    key = (name, loss, tuple(sorted(params.items())))
    if key not in _REF:
        g = case(name)
        _REF[key] = ref_gnc.gnc_optimize(*args(g), vk=g["vk"], ek=g["ek"], loss=loss, barc_sq=g["barc_sq"], known=g["known"],
                                         **dict(dict(inner_iters=g["inner_iters"]), **params))
    return _REF[key]
