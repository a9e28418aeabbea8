"""The graphs the bearing / data-association checks run on (tests/test_assoc_cpu.py, tests/test_assoc_gpu.py): deterministic
builders, one per gap, each with a predicate (``reach``) proving that the case gets there, and the bars of the checks.
typed_cases' builder with bearings added.  TEST INFRASTRUCTURE ONLY.

A case is typed_cases' dict; ek may hold 2 (EDGE_BEARING_SE2_XY: meas[0] the angle, info[0] its information, the rest junk on
purpose).  On every bearing edge the point lies at least 0.5 m from the pose, at the truth and at the starting guess."""
import numpy as np

import ref_numpy as R
import reference_cases
import typed_cases as TC

U = R.U
KEYS = TC.KEYS
args, kinds = TC.args, TC.kinds

# Componentwise backward error (ref_assoc.step_backward_error) a Gauss-Newton step may show: typed_cases' rule, the larger of
# reference_cases.OMEGA_MAX (120 u) and ten times what the two float64 reference solves (SuperLU, dense LAPACK) show on these
# cases.  Measured by tests/test_assoc_cpu.py::test_reference_backward_error on every case Gauss-Newton can step, from the
# initial guess and from the reference's 3rd iterate: 0 u everywhere, that is, every residual lies below the pose update's own
# rounding allowance (tree600b starts 0.02 from the truth; tree600's 9.78 u came from the first step off the odometry guess).
REF_OMEGA_MEASURED = 0.0
OMEGA_MAX = max(reference_cases.OMEGA_MAX, 10 * REF_OMEGA_MEASURED * U)
CHI_RTOL = TC.CHI_RTOL
MARG_TAU = TC.MARG_TAU
AGREE_TAU = 1e-9       # two device calls on the same H, per block by the Frobenius scale: tests/test_joint_marginals_gpu.py's bar
REF_ERR_MAX = TC.REF_ERR_MAX
R_MIN = 0.5


class _Builder(TC._Builder):
    def bearing(self, i, l, sigma=0.01, z=None, w=None):
        a, p = np.array(self.truth[i]), np.array(self.truth[l])
        d = TC._rot(a[2]) @ (p[:2] - a[:2])
        zz = float(R.normalize_theta(np.arctan2(d[1], d[0]) + sigma * self.rng.standard_normal())) if z is None else float(z)
        w = 2000.0 * self.rng.uniform(0.5, 2.0) if w is None else float(w)
        self._edge(i, l, [zz, 5.0, -6.0], [w, 9.0, 7.0, -4.0, -3.0, 11.0], 2)     # (all but meas[0] / info[0]: junk, ignored)

    def dist(self, i, l):
        return float(np.hypot(*(np.array(self.truth[i][:2]) - np.array(self.truth[l][:2]))))


def _anchor(b, l):
    """A fixed pose that sees point l with an EDGE_SE2_XY: makes the tiny cases regular."""
    p = np.array(b.truth[l][:2])
    f = b.pose(p[0] + 2.0, p[1], np.pi, fixed=True)
    b.observe(f, l, z=[2.01, -0.02])
    return f


def bearing_answer():
    """Pose (0, 0, 0) sees point (1, 1) under z = pi / 4 + 0.1 with Omega = 4 (edge 0): e = -0.1, J_i = (1/2, -1/2, -1),
    J_l = (-1/2, 1/2), chi2 = 0.04.  A pose prior and an anchored observation make the system regular."""
    b = _Builder(41)
    a = b.pose(0.0, 0.0, 0.0)
    l = b.point(1.0, 1.0)
    b.bearing(a, l, z=np.pi / 4 + 0.1, w=4.0)
    b.prior_se2(a, z=[0.0, 0.0, 0.0])
    _anchor(b, l)
    g = b.build(noise=0.0)
    g["poses"] = g["truth"].copy()
    return g


def bearing_wrap():
    """A point behind the robot: the predicted bearing is -pi + 0.01, the measured one pi - 0.01; e = 0.02, not 2 pi - 0.02."""
    b = _Builder(42)
    a = b.pose(0.0, 0.0, 0.0)
    l = b.point(-2.0 * np.cos(0.01), -2.0 * np.sin(0.01))
    b.bearing(a, l, z=np.pi - 0.01, w=50.0)
    b.prior_se2(a, z=[0.0, 0.0, 0.0])
    _anchor(b, l)
    g = b.build(noise=0.0)
    g["poses"] = g["truth"].copy()
    return g


def bearing_axis():
    """Three fixed poses and one free point, bearings only, small information: the pose at the origin with theta = 0 sees the
    point at (2, 0) along the world's x axis -- that edge's H_jj(0,0) is exactly 0 --, the other two see it obliquely (three
    bearings for two unknowns: chi2 does not converge to 0, where comparing it would compare rounding).  Every diagonal entry
    of the true system is below 1: a dummy pivot of 1.0 would be Levenberg's max |H_jj|."""
    b = _Builder(43)
    a = b.pose(0.0, 0.0, 0.0, fixed=True)
    c = b.pose(1.0, -2.0, 1.0, fixed=True)
    l = b.point(2.0, 0.0)
    b.bearing(a, l, z=0.04, w=0.5)
    b.bearing(c, l, sigma=0.0, w=0.75)
    b.meas[-1][0] += 0.03
    d = b.pose(3.0, 2.5, -2.0, fixed=True)
    b.bearing(d, l, sigma=0.0, w=0.6)
    b.meas[-1][0] -= 0.05
    g = b.build(noise=0.0)
    g["poses"] = g["truth"].copy()
    g.update(point=l, axis_edge=0)
    return g


def _chain(b, n=6):
    P = [b.pose(0.9 * k, 0.3 * np.sin(0.8 * k), 0.2 * np.cos(0.7 * k), fixed=(k == 0)) for k in range(n)]
    for k in range(n - 1):
        b.odom(P[k], P[k + 1])
    return P


def bearing_two():
    """Six poses (the first fixed) and a point with exactly two bearings: the fewest that make its block positive definite."""
    b = _Builder(44)
    P = _chain(b)
    b.odom(P[0], P[3], sigma=0.02)
    b.odom(P[2], P[5], sigma=0.02)
    l = b.point(2.0, 2.5)
    b.bearing(P[1], l)
    b.bearing(P[4], l)
    g = b.build(noise=0.03)
    g["point"] = l
    return g


def bearing_one():
    """The same chain with two closures, the point seen once, along the world's x axis from a pose with theta = 0 at the start:
    its block is singular with H_xx exactly 0 (no rounding decides).  Gauss-Newton cannot step; Levenberg can."""
    b = _Builder(45)
    P = _chain(b)
    b.odom(P[0], P[3], sigma=0.02)
    b.odom(P[2], P[5], sigma=0.02)
    a = b.pose(1.5, 3.0, 0.0)
    b.odom(P[2], a)
    b.odom(P[4], a, sigma=0.02)
    l = b.point(3.5, 3.0)
    b.bearing(a, l)
    g = b.build(noise=0.03)
    g["poses"][a] = g["truth"][a]
    g["poses"][l] = g["truth"][l]
    g.update(point=l, pose=a)
    return g


def mixed5(n_edges, last_kind, seed=46):
    """typed_cases.mixed with bearings: 48 poses, 24 points, no fixed vertex, one pose prior, five position priors; every point
    has two EDGE_SE2_XY observations, the further ones alternate between bearings (from poses at least 0.8 m away) and
    EDGE_SE2_XY; exactly ``n_edges`` edges, kinds interleaved, the last of kind ``last_kind``."""
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
    for l in L:
        near = np.argsort([b.dist(p, l) for p in P])
        b.observe(P[near[0]], l)
        b.observe(P[near[1]], l)
    flip = 0
    while len(b.ef) < n_edges:
        l, p = L[int(b.rng.integers(len(L)))], P[int(b.rng.integers(len(P)))]
        flip += 1
        if flip % 3 != 0 and 0.8 <= b.dist(p, l) <= 12.0:
            b.bearing(p, l)
        else:
            b.observe(p, l)
    assert len(b.ef) == n_edges
    b.shuffle_edges(last_kind)
    g = b.build(noise=0.03)
    g.update(P=np.array(P), L=np.array(L))
    return g


def tree600b():
    """typed_cases.tree600 with one observation of every point -- the one from furthest away, 300 of the 900 -- made a
    bearing: several tree levels, points as leaves and inside fronts.  The poses start 0.02 from the truth: from the recipe's
    odometry guess, metres off, Gauss-Newton on bearings diverges (the reference's own chi2 grows)."""
    g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in TC.case("tree600").items()}
    rng = np.random.default_rng(47)
    free = (g["vk"] == 0) & (g["fixed"] == 0)
    g["poses"][free] = g["truth"][free] + 0.02 * rng.standard_normal((int(free.sum()), 3))
    g["poses"][free, 2] = R.normalize_theta(g["poses"][free, 2])
    ek, ef, et, truth, guess = g["ek"], g["edge_from"], g["edge_to"], g["truth"], g["poses"]
    for l in np.flatnonzero(g["vk"] == 1):
        obs = np.flatnonzero((et == l) & (ek == 1))
        r = np.minimum(np.hypot(*(truth[ef[obs], :2] - truth[l, :2]).T), np.hypot(*(guess[ef[obs], :2] - guess[l, :2]).T))
        k = int(obs[np.argmax(r)])
        zx, zy = g["meas"][k, :2]
        ek[k] = 2
        g["meas"][k] = [np.arctan2(zy, zx) + 0.005 * rng.standard_normal(), 5.0, -6.0]
        g["info"][k] = [2000.0 * rng.uniform(0.5, 2.0), 9.0, 7.0, -4.0, -3.0, 11.0]
    return g


# ------------------------------------------------------------------------------------------------ reach predicates

def bearing_ranges(g, poses=None):
    """|l - t_i| of every bearing edge at ``poses`` (default: the starting guess)."""
    p = g["poses"] if poses is None else poses
    m = g["ek"] == 2
    return np.hypot(*(p[g["edge_to"][m], :2] - p[g["edge_from"][m], :2]).T)


def _far(g):
    return bool((g["ek"] == 2).any() and bearing_ranges(g).min() >= R_MIN and bearing_ranges(g, g["truth"]).min() >= R_MIN)


def _reach_answer(g):
    return _far(g) and int(g["ek"][0]) == 2 and g["info"][0, 0] == 4.0 and g["meas"][0, 0] == np.pi / 4 + 0.1


def _reach_wrap(g):
    import ref_assoc as A
    z, _ = A.predict(g["poses"], int(g["edge_from"][0]), int(g["edge_to"][0]), 2)
    return (_far(g) and int(g["ek"][0]) == 2 and abs(z[0] - (-np.pi + 0.01)) < 1e-12 and abs(z[0] - g["meas"][0, 0]) > 6.0
            and abs(A.edge_errors(*args(g)[:1], *args(g)[2:5], g["ek"])[0, 0] - 0.02) < 1e-12)


def _reach_axis(g):
    import ref_assoc as A
    Jj = A.jacobians(g["poses"], g["edge_from"], g["edge_to"], g["meas"], g["ek"])[1]
    H, _, lay = A.build_system(*args(g), *kinds(g))
    return (_far(g) and np.all(g["ek"] == 2) and Jj[g["axis_edge"], 0, 0] == 0.0 and Jj[1, 0, 0] != 0.0 and lay.n == 2
            and 0 < H.diagonal().max() < 1.0)


def _reach_two(g):
    to = g["edge_to"][g["ek"] == 2]
    return _far(g) and len(to) == 2 and np.all(to == g["point"]) and int(np.sum(g["edge_to"] == g["point"])) == 2


def _reach_one(g):
    import ref_assoc as A
    H, _, lay = A.build_system(*args(g), *kinds(g))
    o = lay.off[g["point"]]
    return (_far(g) and int(np.sum(g["edge_to"] == g["point"])) == 1 and H[o, o] == 0.0 and H[o + 1, o + 1] > 0
            and g["poses"][g["pose"], 2] == 0.0)


def _reach_mixed5(n_edges, last_kind):
    def reach(g):
        nE = len(g["ek"])
        return (_far(g) and nE == n_edges and int(g["ek"][-1]) == last_kind and all(TC._count(g, k) > 0 for k in (0, 1, 2, 3, 4))
                and TC._interleaved(g) and int(g["fixed"].sum()) == 0 and TC._count(g, 2) >= 20
                and (nE != 257 or (nE - 1) // 256 == 1 and (nE - 1) % 256 == 0))
    return reach


def _reach_tree(g):
    per_point = np.bincount(g["edge_to"][g["ek"] == 2], minlength=len(g["poses"]))[g["vk"] == 1]
    return _far(g) and TC._reach_tree(g) and TC._count(g, 2) == 300 and TC._count(g, 1) == 600 and np.all(per_point == 1)


# name -> (builder, the gap it is there for, reach).  "gn": False where Gauss-Newton cannot factor H.
CASES = {
    "bearing_answer": (bearing_answer, "the hand-worked bearing", _reach_answer),
    "bearing_wrap": (bearing_wrap, "a bearing error across +-pi", _reach_wrap),
    "bearing_axis": (bearing_axis, "a bearing along the world's x axis: H_jj(0,0) == 0 exactly, every real diagonal below 1", _reach_axis),
    "bearing_two": (bearing_two, "a point with exactly two bearings", _reach_two),
    "bearing_one": (bearing_one, "a point with a single bearing: singular for Gauss-Newton, regular for Levenberg", _reach_one),
    "mixed5_255": (lambda: mixed5(255, 4), "all five kinds, one idle lane in the only workgroup, a position prior last", _reach_mixed5(255, 4)),
    "mixed5_256": (lambda: mixed5(256, 1), "all five kinds, exactly one full workgroup, a landmark observation last", _reach_mixed5(256, 1)),
    "mixed5_257": (lambda: mixed5(257, 2), "all five kinds, the second workgroup's one live lane is a bearing", _reach_mixed5(257, 2)),
    "tree600b": (tree600b, "merged level launches and the chained backward solve with bearings", _reach_tree),
}
GN_CASES = [n for n in CASES if n != "bearing_one"]

_BUILT = {}


def case(name):
    """The case's graph, built once (callers must not modify it)."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name][0]()
    return _BUILT[name]
