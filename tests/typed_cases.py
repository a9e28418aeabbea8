"""The graphs the typed-factor checks run on (tests/test_typed_cpu.py, tests/test_typed_gpu.py): deterministic builders, one
per gap of the typed path, each with a predicate (``reach``) proving that the case gets there, and the bars of the checks.
TEST INFRASTRUCTURE ONLY.

A case is a dict: poses [nV, 3], fixed [nV], edge_from / edge_to [nE], meas [nE, 3], info [nE, 6], vk [nV] (0 pose, 1 point),
ek [nE] (0 EDGE_SE2, 1 EDGE_SE2_XY, 3 EDGE_PRIOR_SE2, 4 EDGE_PRIOR_SE2_XY)."""
import numpy as np

import ref_numpy as R
import reference_cases
from cg_mrslam_amd import synth

KEYS = ("poses", "fixed", "edge_from", "edge_to", "meas", "info")
U = R.U

# Componentwise backward error (ref_typed.step_backward_error) a typed Gauss-Newton step may show: reference_cases.OMEGA_MAX
# (120 u), unless ten times the largest value the two float64 reference solves (SuperLU, dense LAPACK) show on these cases is
# larger.  Measured by tests/test_typed_cpu.py::test_reference_backward_error on every case, from the initial guess and from
# the reference's 3rd iterate: 9.78 u (the dense solve of tree600's first step; every other step shows 0 u, that is, a
# residual below the pose update's own rounding allowance).  Ten times that, 97.8 u, is below 120 u: reference_cases.OMEGA_MAX holds.
REF_OMEGA_MEASURED = 9.78
OMEGA_MAX = max(reference_cases.OMEGA_MAX, 10 * REF_OMEGA_MEASURED * U)
CHI_RTOL = 1e-6        # chi2 before every iteration against the reference: tests/test_gn_gpu.py's bar
MARG_TAU = 1e-9        # marginal blocks, per block by its own Frobenius norm: tests/test_reference_gpu.py's bar
REF_ERR_MAX = reference_cases.REF_ERR_MAX


def args(g):
    return tuple(g[k] for k in KEYS)


def kinds(g):
    return g["vk"], g["ek"]


def _rot(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, s], [-s, c]])          # R(t)^T


class _Builder:
    """Truth first (a trajectory and points), then edges measured on the truth with a little noise, then a perturbed guess."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.truth, self.vk, self.fixed = [], [], []
        self.ef, self.et, self.meas, self.info, self.ek = [], [], [], [], []

    def pose(self, x, y, t, fixed=False):
        self.truth.append([x, y, float(R.normalize_theta(t))])
        self.vk.append(0)
        self.fixed.append(1 if fixed else 0)
        return len(self.truth) - 1

    def point(self, x, y, fixed=False):
        self.truth.append([x, y, 0.0])
        self.vk.append(1)
        self.fixed.append(1 if fixed else 0)
        return len(self.truth) - 1

    def trajectory(self, n, step=1.0, turn=0.25):
        """n poses on a wandering path; returns their indices."""
        idx, x, y, t = [], 0.0, 0.0, 0.3
        for _ in range(n):
            idx.append(self.pose(x, y, t))
            t += turn * self.rng.standard_normal()
            x += step * np.cos(t)
            y += step * np.sin(t)
        return idx

    def _edge(self, i, j, z, u, kind):
        self.ef.append(i); self.et.append(j); self.meas.append(z); self.info.append(u); self.ek.append(kind)

    def _info3(self, scale):
        Q, _ = np.linalg.qr(self.rng.standard_normal((3, 3)))
        O = Q @ np.diag(scale * self.rng.uniform(0.5, 2.0, 3)) @ Q.T
        return [O[0, 0], O[0, 1], O[0, 2], O[1, 1], O[1, 2], O[2, 2]]

    def _info2(self, scale):
        Q, _ = np.linalg.qr(self.rng.standard_normal((2, 2)))
        O = Q @ np.diag(scale * self.rng.uniform(0.5, 2.0, 2)) @ Q.T
        # (the entries a 2-dimensional factor must ignore are filled with junk on purpose)
        return [O[0, 0], O[0, 1], 7.0, O[1, 1], -3.0, 11.0]

    def odom(self, i, j, sigma=0.01):
        a, b = np.array(self.truth[i]), np.array(self.truth[j])
        d = _rot(a[2]) @ (b[:2] - a[:2])
        z = np.array([d[0], d[1], float(R.normalize_theta(b[2] - a[2]))]) + sigma * self.rng.standard_normal(3)
        self._edge(i, j, z.tolist(), self._info3(500.0), 0)

    def observe(self, i, l, sigma=0.01, z=None):
        a, p = np.array(self.truth[i]), np.array(self.truth[l])
        d = _rot(a[2]) @ (p[:2] - a[:2]) + sigma * self.rng.standard_normal(2) if z is None else np.asarray(z, float)
        self._edge(i, l, [d[0], d[1], 5.0], self._info2(300.0), 1)     # (meas[2] of a 2-dimensional factor: junk, ignored)

    def prior_se2(self, i, sigma=0.01, z=None):
        z = np.array(self.truth[i]) + sigma * self.rng.standard_normal(3) if z is None else np.asarray(z, float)
        self._edge(i, i, [z[0], z[1], float(z[2])], self._info3(200.0), 3)

    def prior_xy(self, i, sigma=0.02):
        z = np.array(self.truth[i][:2]) + sigma * self.rng.standard_normal(2)
        self._edge(i, i, [z[0], z[1], -2.0], self._info2(100.0), 4)

    def shuffle_edges(self, last_kind=None):
        """Interleave the kinds; ``last_kind``: the kind of the last edge."""
        n = len(self.ef)
        perm = self.rng.permutation(n)
        if last_kind is not None:
            k = int(np.flatnonzero(np.array(self.ek)[perm] == last_kind)[-1])
            perm[[k, n - 1]] = perm[[n - 1, k]]
        for name in ("ef", "et", "meas", "info", "ek"):
            setattr(self, name, [getattr(self, name)[q] for q in perm])

    def build(self, noise=0.05):
        truth = np.array(self.truth, dtype=np.float64).reshape(-1, 3)
        vk = np.array(self.vk, dtype=np.uint8)
        fixed = np.array(self.fixed, dtype=np.uint8)
        poses = truth + noise * self.rng.standard_normal(truth.shape)
        poses[:, 2] = R.normalize_theta(poses[:, 2])
        poses[vk == 1, 2] = 0.0
        poses[fixed == 1] = truth[fixed == 1]
        return dict(truth=truth, poses=poses, fixed=fixed, vk=vk, edge_from=np.array(self.ef, dtype=np.int32),
                    edge_to=np.array(self.et, dtype=np.int32), meas=np.array(self.meas, dtype=np.float64).reshape(-1, 3),
                    info=np.array(self.info, dtype=np.float64).reshape(-1, 6), ek=np.array(self.ek, dtype=np.uint8))


def mixed(n_edges, last_kind, seed=21):
    """48 poses, 24 points, no fixed vertex, one pose prior and five position priors, kinds interleaved; exactly ``n_edges``
    edges, the last of kind ``last_kind``."""
    b = _Builder(seed)
    P = b.trajectory(48)
    L = [b.point(*(np.array(b.truth[P[2 * k]][:2]) + b.rng.uniform(-3, 3, 2))) for k in range(24)]
    for k in range(47):
        b.odom(P[k], P[k + 1])
    for k in range(0, 40, 4):
        b.odom(P[k], P[k + 7], sigma=0.02)
    b.prior_se2(P[0])
    for k in (5, 15, 25, 35, 45):
        b.prior_xy(P[k])
    for l in L:                                   # every point from two poses at least
        near = np.argsort([np.hypot(*(np.array(b.truth[p][:2]) - np.array(b.truth[l][:2]))) for p in P])
        b.observe(P[near[0]], l)
        b.observe(P[near[1]], l)
    while len(b.ef) < n_edges:                    # ... then more observations up to the edge count
        l = L[int(b.rng.integers(len(L)))]
        b.observe(P[int(b.rng.integers(len(P)))], l)
    assert len(b.ef) == n_edges
    b.shuffle_edges(last_kind)
    return b.build()


def prior_gauge(with_prior=True):
    """30 poses, a chain with closures, no fixed vertex: one EDGE_PRIOR_SE2 holds the gauge (without it H is singular)."""
    b = _Builder(22)
    P = b.trajectory(30)
    for k in range(29):
        b.odom(P[k], P[k + 1])
    for k in range(0, 24, 5):
        b.odom(P[k], P[k + 6], sigma=0.02)
    if with_prior:
        b.prior_se2(P[3])
    return b.build()


def gps_chain():
    """A 200-pose chain, no fixed vertex, a position prior on every tenth pose; pose 50 carries three priors."""
    b = _Builder(23)
    P = b.trajectory(200, turn=0.1)
    for k in range(199):
        b.odom(P[k], P[k + 1])
        if k % 10 == 0:
            b.prior_xy(P[k])
    b.prior_xy(P[50])
    b.prior_se2(P[50], sigma=0.02)
    return b.build(noise=0.03)


def leaf_and_hub():
    """45 poses (the first fixed); ten points seen once, one point seen from 40 poses, one point no edge touches, one fixed
    point seen from five poses."""
    b = _Builder(24)
    P = b.trajectory(45)
    b.fixed[P[0]] = 1
    for k in range(44):
        b.odom(P[k], P[k + 1])
    leaves = [b.point(*(np.array(b.truth[P[4 * k + 1]][:2]) + b.rng.uniform(-2, 2, 2))) for k in range(10)]
    for k, l in enumerate(leaves):
        b.observe(P[4 * k + 1], l)
    hub = b.point(3.0, 2.0)
    for k in range(40):
        b.observe(P[k + 2], hub)
    lone = b.point(-7.0, 9.0)
    fixed_pt = b.point(1.0, -4.0, fixed=True)
    for k in (3, 9, 20, 31, 40):
        b.observe(P[k], fixed_pt)
    b.shuffle_edges()
    g = b.build()
    g.update(hub=hub, lone=lone, fixed_point=fixed_pt, leaves=np.array(leaves))
    return g


def prior_only_vertex():
    """A small landmark graph plus one pose whose only factors are priors (a pose prior and a position prior)."""
    b = _Builder(25)
    P = b.trajectory(12)
    b.fixed[P[0]] = 1
    for k in range(11):
        b.odom(P[k], P[k + 1])
    l = b.point(2.0, 1.0)
    for k in (1, 4, 8):
        b.observe(P[k], l)
    alone = b.pose(20.0, -5.0, 1.0)
    b.prior_se2(alone)
    b.prior_xy(alone)
    g = b.build()
    g["alone"] = alone
    return g


def tree600():
    """600 poses of the C2 recipe with 1600 pose-pose edges, 300 points seen three times each: 2500 edges, deep enough for
    merged level launches and the chained backward solve (reference_cases' pg500 branch)."""
    pg = synth.make_pose_graph(600, 1600, seed=4)
    b = _Builder(26)
    for v in range(600):
        b.pose(*pg["truth"][v], fixed=bool(pg["fixed"][v]))
    for k in range(len(pg["edge_from"])):
        b._edge(int(pg["edge_from"][k]), int(pg["edge_to"][k]), pg["meas"][k].tolist(), pg["info"][k].tolist(), 0)
    for k in range(300):
        p = 2 * k
        l = b.point(*(pg["truth"][p, :2] + b.rng.uniform(-2, 2, 2)))
        for q in (p, min(p + 1, 599), min(p + 3, 599)):
            b.observe(q, l)
    g = b.build(noise=0.0)
    g["poses"][:600] = pg["poses"]                       # the recipe's own odometry guess
    pts = g["vk"] == 1
    g["poses"][pts, :2] = g["truth"][pts, :2] + 0.05 * b.rng.standard_normal((int(pts.sum()), 2))
    return g


def wrap_prior():
    """A pose just across -pi with a prior whose z_theta lies within 1e-3 of +pi (and a second pose, to have an edge)."""
    b = _Builder(27)
    a = b.pose(1.0, 2.0, -np.pi + 2e-4)
    c = b.pose(2.0, 2.5, -3.0)
    b.odom(a, c)
    b.prior_se2(a, z=[1.1, 1.9, np.pi - 5e-4])
    g = b.build(noise=0.0)
    g["poses"] = g["truth"].copy()
    return g


def landmark_answer():
    """One pose fixed at (1, 2, pi/2), one point started at (7, -4), seen once at z = (3, 0): the point is at (1, 5) after one step."""
    return dict(poses=np.array([[1.0, 2.0, np.pi / 2], [7.0, -4.0, 0.0]]), fixed=np.array([1, 0], np.uint8),
                vk=np.array([0, 1], np.uint8), edge_from=np.array([0], np.int32), edge_to=np.array([1], np.int32),
                meas=np.array([[3.0, 0.0, 0.0]]), info=np.array([[4.0, 1.5, 9.0, 3.0, -2.0, 5.0]]), ek=np.array([1], np.uint8),
                answer=np.array([1.0, 5.0]))


def prior_answer(wrap=False):
    """A lone free pose with one EDGE_PRIOR_SE2: at z after one step (wrap: z_theta near pi, the pose just across -pi)."""
    z = [0.7, -1.2, np.pi - 5e-4] if wrap else [0.7, -1.2, 0.9]
    x = [0.2, 0.4, -np.pi + 3e-4] if wrap else [0.2, 0.4, 0.1]
    return dict(poses=np.array([x]), fixed=np.array([0], np.uint8), vk=np.array([0], np.uint8), edge_from=np.array([0], np.int32),
                edge_to=np.array([0], np.int32), meas=np.array([z]), info=np.array([[5.0, 1.0, 0.5, 4.0, 0.2, 3.0]]),
                ek=np.array([3], np.uint8), answer=np.array(z))


# ------------------------------------------------------------------------------------------------ reach predicates

def _count(g, kind):
    return int(np.sum(g["ek"] == kind))


def _interleaved(g):
    return int(np.sum(np.diff(g["ek"].astype(int)) != 0)) >= len(g["ek"]) // 4


def _reach_mixed(n_edges, last_kind):
    def reach(g):
        nE = len(g["ek"])
        return (nE == n_edges and int(g["ek"][-1]) == last_kind and all(_count(g, k) > 0 for k in (0, 1, 3, 4)) and _interleaved(g)
                and int(g["fixed"].sum()) == 0 and int((g["vk"] == 1).sum()) == 24 and int((g["vk"] == 0).sum()) == 48
                and (nE != 257 or (nE - 1) // 256 == 1 and (nE - 1) % 256 == 0))     # 257: the second workgroup's one live lane
    return reach


def _reach_gps(g):
    per_vertex = np.bincount(g["edge_from"][g["ek"] >= 3], minlength=len(g["poses"]))
    return (int(g["fixed"].sum()) == 0 and int((g["vk"] == 0).sum()) == 200 and _count(g, 4) >= 20 and per_vertex.max() == 3
            and int((per_vertex > 0).sum()) == 20)


def _reach_leaf_hub(g):
    deg = np.bincount(g["edge_to"][g["ek"] == 1], minlength=len(g["poses"]))
    touched = np.zeros(len(g["poses"]), bool)
    touched[g["edge_from"]] = touched[g["edge_to"]] = True
    return (deg[g["hub"]] == 40 and np.all(deg[g["leaves"]] == 1) and not touched[g["lone"]] and g["vk"][g["lone"]] == 1
            and g["fixed"][g["fixed_point"]] == 1 and g["vk"][g["fixed_point"]] == 1 and deg[g["fixed_point"]] == 5)


def _reach_prior_only(g):
    v = g["alone"]
    mine = (g["edge_from"] == v) | (g["edge_to"] == v)
    return bool(mine.sum() == 2 and np.all(g["ek"][mine] >= 3) and g["fixed"][v] == 0)


def _reach_tree(g):
    from cg_mrslam_amd._lib import gn_symbolic_info
    info = gn_symbolic_info(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    return (int((g["vk"] == 0).sum()) == 600 and int((g["vk"] == 1).sum()) == 300 and len(g["ek"]) == 2500
            and info["launch_levels"] >= 4)       # (the GPU test counts the merged launches and the chained solve themselves)


def _reach_wrap(g):
    k = int(np.flatnonzero(g["ek"] == 3)[0])
    v = int(g["edge_from"][k])
    return bool(abs(abs(g["meas"][k, 2]) - np.pi) < 1e-3 and g["meas"][k, 2] > 0 and g["poses"][v, 2] < -3.0
                and abs(g["poses"][v, 2] - g["meas"][k, 2]) > 6.0)


# name -> (builder, the gap it is there for, reach)
CASES = {
    "mixed257": (lambda: mixed(257, 3), "second workgroup of the linearisation: one live lane, a prior; idle lanes shadow it",
                 _reach_mixed(257, 3)),
    "mixed257_xy": (lambda: mixed(257, 1), "the same with a landmark observation last", _reach_mixed(257, 1)),
    "mixed256": (lambda: mixed(256, 4), "exactly one full workgroup", _reach_mixed(256, 4)),
    "mixed255": (lambda: mixed(255, 0), "one idle lane in the only workgroup", _reach_mixed(255, 0)),
    "prior_gauge": (prior_gauge, "no fixed vertex: the prior is the gauge",
                    lambda g: int(g["fixed"].sum()) == 0 and _count(g, 3) == 1 and _count(g, 4) == 0 and _count(g, 1) == 0),
    "gps_chain": (gps_chain, "position priors alone fix the frame; three priors on one vertex (order of the unary sum)", _reach_gps),
    "leaf_and_hub": (leaf_and_hub, "points seen once, a point seen 40 times, an untouched point, a fixed point", _reach_leaf_hub),
    "prior_only_vertex": (prior_only_vertex, "a vertex whose only factors are priors is a live column", _reach_prior_only),
    "tree600": (tree600, "merged level launches and the chained backward solve with typed terms", _reach_tree),
    "wrap_prior": (wrap_prior, "a prior's heading error across +-pi", _reach_wrap),
}

_BUILT = {}


def case(name):
    """The case's graph, built once (callers must not modify it)."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name][0]()
    return _BUILT[name]
