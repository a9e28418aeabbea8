"""The graphs the max-mixture checks run on (tests/test_mixture_cpu.py, tests/test_mixture_gpu.py): deterministic builders and
the reference's result on each, computed once per process.  TEST INFRASTRUCTURE ONLY.

A case is a dict: poses, fixed, edge_from, edge_to, meas, info (every edge's component 0), vk / ek (None for a pure pose
graph), mix = (comp_ptr, comp_meas, comp_info, comp_weight), iters, exempt (edges whose components are identical: left out of
the margin), and where it applies clean (the graph of the true components alone) and multi (the multi-component edges).

The reach predicate every case carries: at every point the reference visits -- every linearisation, every trial point of
Levenberg-Marquardt and dogleg -- every multi-component edge's best and second-best costs differ by more than MARGIN,
relative to the second best.  MARGIN is the project's per-iteration chi2 bar (typed_cases.CHI_RTOL): an edge's cost on the
device differs from the reference's by far less, so rounding cannot flip a selection.  It is a condition on the inputs,
asserted by tests/test_mixture_cpu.py from the reference alone."""
import numpy as np

import ref_mixture as RM
import ref_robust
import ref_typed
import typed_cases
from cg_mrslam_amd import synth

KEYS = ("poses", "fixed", "edge_from", "edge_to", "meas", "info")
MARGIN = 1e-6
ANCHOR_R = 6 * np.log(10.0) / 0.99          # the null component of the anchor wins exactly when r_1 exceeds this
I3 = [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]


def args(g):
    return tuple(g[k] for k in KEYS)


def mix_from_lists(comps):
    """comps[k] = [(w, z [3], u [6]), ...] per edge -> (comp_ptr, comp_meas, comp_info, comp_weight)."""
    ptr = np.cumsum([0] + [len(c) for c in comps]).astype(np.int32)
    flat = [q for c in comps for q in c]
    return (ptr, np.array([q[1] for q in flat], dtype=np.float64).reshape(-1, 3),
            np.array([q[2] for q in flat], dtype=np.float64).reshape(-1, 6), np.array([q[0] for q in flat], dtype=np.float64))


def _case(g, comps, iters, vk=None, ek=None, exempt=(), **extra):
    mix = mix_from_lists(comps)
    first = mix[0][:-1]
    out = dict({k: g[k] for k in KEYS}, meas=mix[1][first].copy(), info=mix[2][first].copy(), vk=vk, ek=ek, mix=mix, iters=iters,
               exempt=np.asarray(list(exempt), dtype=np.int64), multi=np.flatnonzero(np.diff(mix[0]) > 1))
    out.update(extra)
    return out


def anchor(d):
    """Pose 0 fixed at the origin, pose 1 free at (1, 0, 0).  Edge 0: the odometry (1, 0, 0) with information 1000 I.  Edge 1: a
    mixture measuring (1 + d, 0, 0) with Omega_1 = I, Omega_2 = 0.01 I, w = (1/2, 1/2): a = (2 ln 1/2, 2 ln 1/2 - 6 ln 10), so
    c = (0, 6 ln 10) and the costs at the start are (d^2, 0.01 d^2 + 6 ln 10): the null component wins exactly when
    d^2 > 6 ln 10 / 0.99 = 13.95506...: d = 3.7 (13.69) stays on component 0, d = 3.8 (14.44) takes the null one."""
    g = dict(poses=np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), fixed=np.array([1, 0], np.uint8),
             edge_from=np.zeros(2, np.int32), edge_to=np.ones(2, np.int32), meas=None, info=None)
    z = [1.0 + d, 0.0, 0.0]
    comps = [[(1.0, [1.0, 0.0, 0.0], [1000.0 * v for v in I3])], [(0.5, z, I3), (0.5, z, [0.01 * v for v in I3])]]
    return _case(g, comps, 3, d=d)


def _alternatives(g, edges, K, where, rng, lo, hi, dth):
    """Per edge of ``edges`` K components of equal weight and the edge's information: the true measurement at index ``where``
    ("first", "last" or "random"), the others moved by +-U(lo, hi) m on x and y and, dth None, a heading drawn from U(-pi, pi),
    else +-dth rad."""
    comps = [[(1.0, g["meas"][k], g["info"][k])] for k in range(len(g["edge_from"]))]
    true_at = {}
    for k in edges:
        t = 0 if where == "first" else K - 1 if where == "last" else int(rng.integers(K))
        c = []
        for q in range(K):
            z = g["meas"][k].copy()
            if q != t:
                z[:2] += rng.choice([-1.0, 1.0], 2) * rng.uniform(lo, hi, 2)
                z[2] = rng.uniform(-np.pi, np.pi) if dth is None else ref_typed.R.normalize_theta(z[2] + rng.choice([-1.0, 1.0]) * dth)
            c.append((1.0, z, g["info"][k]))
        comps[int(k)] = c
        true_at[int(k)] = t
    return comps, true_at


def gross(nV, nE, K, where, extra_edges=(), tie_edge=None):
    """synth.make_pose_graph(nV, nE, seed 7); every 5th closure (and ``extra_edges``) is one of K alternatives, all but one gross
    (ref_robust.outlier_graph's corruption: +-U(3, 10) m, heading uniform).  ``tie_edge``: that edge gets its own measurement
    twice."""
    g = synth.make_pose_graph(nV, nE, seed=7)
    assert len(g["edge_from"]) == nE
    rng = np.random.default_rng(1)
    lc = np.arange(nV - 1, nE)[::5]
    edges = np.unique(np.concatenate([lc, np.asarray(list(extra_edges), dtype=np.int64)]))
    comps, true_at = _alternatives(g, edges, K, where, rng, 3.0, 10.0, None)
    exempt = ()
    if tie_edge is not None:
        assert tie_edge not in true_at
        comps[tie_edge] = [(1.0, g["meas"][tie_edge], g["info"][tie_edge])] * 2
        exempt = (tie_edge,)
    return _case(g, comps, 10, exempt=exempt, clean=g, true_at=true_at)


def switching():
    """300 / 1000; every 5th closure has the wrong alternative FIRST, close to the true one (+-U(0.2, 0.6) m, +-0.2 rad, rng
    seed 1; drawn array by array: the signs on x and y, the heading's signs, the magnitudes): 22 edges start on the wrong
    component, 19 change over after iteration 1, 3 after iteration 2, none later (asserted by tests/test_mixture_cpu.py).  The
    outcome depends on the draw: other orders of the same draws leave one to three edges on the wrong component for good."""
    g = synth.make_pose_graph(300, 1000, seed=7)
    rng = np.random.default_rng(1)
    edges = np.arange(299, 1000)[::5]
    sgn = rng.choice([-1.0, 1.0], size=(len(edges), 2))
    sth = rng.choice([-1.0, 1.0], size=len(edges))
    mag = rng.uniform(0.2, 0.6, size=(len(edges), 2))
    comps = [[(1.0, g["meas"][k], g["info"][k])] for k in range(len(g["edge_from"]))]
    for q, k in enumerate(edges):
        z = g["meas"][k].copy()
        z[:2] += sgn[q] * mag[q]
        z[2] = ref_typed.R.normalize_theta(z[2] + 0.2 * sth[q])
        comps[int(k)] = [(1.0, z, g["info"][k]), (1.0, g["meas"][k], g["info"][k])]
    return _case(g, comps, 10, clean=g, true_at={int(k): 1 for k in edges})


NULL_SCALE = 1e-2


def null_hypothesis():
    """ref_robust.outlier_graph's recipe on 300 / 1000 (every 10th closure corrupted); every closure gets a null hypothesis --
    the same measurement with NULL_SCALE times the information, weight 1 -- behind its own component.  Max-mixture has no
    schedule: from the odometry guess most true closures start beyond 6 ln 10 / 0.99 and take the null component too.  The case
    starts where the method is meant to start, near the optimum: the clean optimum moved by N(0, 0.02) per coordinate."""
    g, bad, closure = ref_robust.outlier_graph(nV=300, nE=1000, seed=7, frac=10, rng_seed=1)
    start = ref_robust.clean_optimum(g, bad) + 0.02 * np.random.default_rng(2).standard_normal(g["poses"].shape)
    start[g["fixed"] != 0] = g["poses"][g["fixed"] != 0]
    g = dict(g, poses=start)
    comps = [[(1.0, g["meas"][k], g["info"][k])] + ([(1.0, g["meas"][k], NULL_SCALE * g["info"][k])] if closure[k] else [])
             for k in range(len(closure))]
    return _case(g, comps, 10, bad=bad, closure=np.flatnonzero(closure))


def typed():
    """typed_cases.mixed(257, 1).  Every 4th landmark observation is one of two: its own measurement, or one 2 to 5 m away with
    half the information (the 2x2 determinants differ by 4; a 3x3 determinant would read the junk the case keeps in the unused
    entries).  The pose prior is one of two with the same measurement and unequal information: a null hypothesis FIRST
    (0.01 Omega), the real one second -- by r alone the null one would win (its r is a hundredth), c = 6 ln 10 on it decides
    for the real one."""
    g = typed_cases.mixed(257, 1)
    rng = np.random.default_rng(3)
    ek = g["ek"]
    comps = [[(1.0, g["meas"][k], g["info"][k])] for k in range(len(ek))]
    for k in np.flatnonzero(ek == 1)[::4]:
        z = g["meas"][k].copy()
        z[:2] += rng.choice([-1.0, 1.0], 2) * rng.uniform(2.0, 5.0, 2)
        comps[int(k)] = [(1.0, g["meas"][k], g["info"][k]), (1.0, z, 0.5 * g["info"][k])]
    prior = int(np.flatnonzero(ek == 3)[0])
    comps[prior] = [(1.0, g["meas"][prior], 0.01 * g["info"][prior]), (1.0, g["meas"][prior], g["info"][prior])]
    return _case(g, comps, 6, vk=g["vk"], ek=ek, prior=prior)


def boundary(nE):
    """120 poses and nE = 255, 256 or 257 edges: multi-component edges at 0, 255, 256 and nE - 1 where they exist -- the workgroup
    boundary of the chi2 partial sums and of the record staging -- beside every 5th closure; the true one last."""
    return gross(120, nE, 2, "last", extra_edges=[k for k in (0, 255, 256, nE - 1) if k < nE])


CASES = {
    "anchor_lo": lambda: anchor(3.7),
    "anchor_hi": lambda: anchor(3.8),
    "g60_k2_first": lambda: gross(60, 150, 2, "first"),
    "g60_k2_last": lambda: gross(60, 150, 2, "last"),
    "g60_k5_random": lambda: gross(60, 150, 5, "random"),
    "g300_k2_last": lambda: gross(300, 1000, 2, "last"),
    "g300_k5_random": lambda: gross(300, 1000, 5, "random"),
    "switching": switching,
    "null": null_hypothesis,
    "typed": typed,
    "b255": lambda: boundary(255),
    "b256": lambda: boundary(256),
    "b257": lambda: boundary(257),
    "tie": lambda: gross(60, 150, 2, "last", tie_edge=3),
}
TRUST_REGION = ("g60_k2_last", "switching")       # the cases Levenberg-Marquardt and dogleg run on
TR_ITERS = 6
_BUILT, _REF = {}, {}


def case(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def reference(name, algorithm="gn"):
    """The reference's run of a case, once per process: dict(poses, chi2, selected, visits, and for "gn" sels (the selection of
    every linearisation), for "lm" / "dl" the policy's own result under out)."""
    key = (name, algorithm)
    if key not in _REF:
        g = case(name)
        a = (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["mix"])
        v = RM.Visits(g["exempt"])
        if algorithm == "gn":
            p, chi, sel, sels = RM.gn_optimize(*a, g["iters"], g["vk"], g["ek"], visits=v)
            _REF[key] = dict(poses=p, chi2=chi, selected=sel, sels=sels, visits=v)
        else:
            run = RM.lm_optimize if algorithm == "lm" else RM.dl_optimize
            out = run(*a, TR_ITERS, g["vk"], g["ek"], visits=v)
            _REF[key] = dict(poses=out["poses"], chi2=out["chi2"], selected=out["selected"], visits=v, out=out)
    return _REF[key]


def clean_optimum(name):
    """Plain Gauss-Newton (15 iterations) on the case's graph of true components."""
    key = (name, "clean")
    if key not in _REF:
        c = case(name)["clean"]
        _REF[key] = ref_typed.R.gn_optimize(c["poses"], c["fixed"], c["edge_from"], c["edge_to"], c["meas"], c["info"], 15)[0]
    return _REF[key]


def plain_on_component0(name):
    """Plain Gauss-Newton on every edge's component 0: what the solver did with such a graph before."""
    key = (name, "plain0")
    if key not in _REF:
        g = case(name)
        _REF[key] = ref_typed.R.gn_optimize(*args(g), g["iters"])[0]
    return _REF[key]
