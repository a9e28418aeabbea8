"""The problems the joint-compatibility checks run on (tests/test_jcbb_cpu.py, tests/test_jcbb_gpu.py): deterministic builders,
each with a predicate (``reach``) proving that the case gets where it is meant to, the reference's answer (computed once), and
the bar of the d2 comparison.  TEST INFRASTRUCTURE ONLY.

Every case keeps margin >= MARGIN_MIN in the reference: no compatibility test it makes lies within 1e-3 (relative) of its
threshold, so rounding cannot decide one.  Assignments are compared only where gap >= GAP_MIN."""
import numpy as np

import ref_jcbb as RJ
from cg_mrslam_amd._lib import JC_GAMMA_99

MARGIN_MIN = 1e-3
GAP_MIN = 1e-3
# The device's d2 against the reference's d2 of the same hypothesis: the larger of 1e-9 and ten times what the reference's own
# two float64 methods (Cholesky solve, np.linalg.solve) disagree by, relative, over every hypothesis it evaluates on these
# cases.  Measured by tests/test_jcbb_cpu.py::test_reference_d2_disagreement: 1.3e-13 at most (the row, whose C has the pose's
# variance of 4 beside landmark variances of 1e-4; the D = 64 case shows 1.6e-15), so the bar is 1e-9 -- a millionth of the
# cases' margin.
REF_D2_DISAGREEMENT_MEASURED = 1.4e-13
D2_BAR = max(1e-9, 10 * REF_D2_DISAGREEMENT_MEASURED)
GAMMA = np.array(JC_GAMMA_99)


def _sigma(pose_cov, lm_cov, L):
    """block diagonal: the poses' joint covariance [3 nA, 3 nA], then lm_cov * I per landmark"""
    pose_cov = np.atleast_2d(np.array(pose_cov, dtype=np.float64))
    n = pose_cov.shape[0] + 2 * L
    S = np.zeros((n, n))
    S[:pose_cov.shape[0], :pose_cov.shape[0]] = pose_cov
    S[pose_cov.shape[0]:, pose_cov.shape[0]:] = lm_cov * np.eye(2 * L)
    return S


def _measure(pose, lm, kind, noise):
    z = RJ.predict_xy(pose, lm)[0]
    if kind == 1:
        return z + noise[:2]
    return np.array([np.arctan2(z[1], z[0]) + noise[0], 0.0])


def _scene(poses, pose_cov, lms, lm_cov, obs, sig_xy=0.05, sig_b=0.002, seed=0, with_R=True):
    """obs: (pose slot, kind, true landmark or an explicit measurement [2]).  Noise at half the stated sigma."""
    rng = np.random.default_rng(seed)
    poses, lms = np.array(poses, dtype=np.float64).reshape(-1, 3), np.array(lms, dtype=np.float64).reshape(-1, 2)
    slot, kinds, zh, R = [], [], [], []
    for s, kind, what in obs:
        sg = sig_xy if kind == 1 else sig_b
        zh.append(_measure(poses[s], lms[what], kind, 0.5 * sg * rng.standard_normal(2)) if np.isscalar(what) else np.array(what, dtype=np.float64))
        slot.append(s); kinds.append(kind)
        R.append(([sg * sg, 0.0, sg * sg] if kind == 1 else [sg * sg, 0.0, 0.0]) if with_R else [0.0, 0.0, 0.0])
    P = RJ.make_problem(poses, slot, kinds, zh, R, lms, _sigma(pose_cov, lm_cov, len(lms)), GAMMA)
    P["truth"] = [what if np.isscalar(what) else -1 for _, _, what in obs]
    return P


def _ring(L, r0=6.0, phase=0.1):
    """L landmarks around the origin at distinct bearings 2 pi / L apart and radii 6 .. 9 m: apart in xy and in bearing"""
    a = phase + 2 * np.pi * np.arange(L) / L
    r = r0 + 3.0 * ((7 * np.arange(L)) % L) / L
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


POSE_COV = np.diag([0.04, 0.04, 1e-4])


def crossed():
    """Two landmarks 0.6 m apart along the line of sight, the pose uncertain by 1 m along it: both measurements are
    individually closest to the wrong landmark."""
    return _scene([[0, 0, 0]], np.diag([1.0, 0.01, 1e-4]), [[5.0, 0.0], [5.6, 0.0]], 1e-4, [(0, 1, [5.35, 0.0]), (0, 1, [5.95, 0.0])])


def m1l1():
    return _scene([[0, 0, 0.3]], POSE_COV, [[4.0, 1.0]], 1e-3, [(0, 1, 0)], seed=1)


def m1l3():
    return _scene([[0, 0, 0.3]], POSE_COV, [[4.0, 1.0], [-3.0, 2.0], [1.0, -5.0]], 1e-3, [(0, 1, 2)], seed=2)


def spurious():
    """three measurements metres from every landmark: no pairing is individually compatible"""
    return _scene([[0, 0, 0.3]], POSE_COV, [[4.0, 1.0], [-3.0, 2.0], [1.0, -5.0], [6.0, 6.0]], 1e-3,
                  [(0, 1, [10.0, -9.0]), (0, 1, [-8.0, -8.0]), (0, 2, [3.0, 0.0])], seed=3)


def fixed_pose():
    """a fixed observing pose (zero rows of Sigma) with measurement noise"""
    return _scene([[1.0, -1.0, 0.5]], np.zeros((3, 3)), _ring(5), 1e-3, [(0, 1, 3), (0, 2, 1), (0, 1, 0), (0, 1, [1.0, 1.0])], seed=4)


def fixed_noinfo():
    """a fixed pose, fixed landmarks and no measurement noise: C = 0, not positive definite -- NaN, incompatible"""
    return _scene([[1.0, -1.0, 0.5]], np.zeros((3, 3)), _ring(3), 0.0, [(0, 1, 0), (0, 2, 1)], seed=5, with_R=False)


def _width(kinds, seed):
    L = 32
    return _scene([[0, 0, 0.2]], POSE_COV, _ring(L), 1e-3, [(0, k, (5 * i + 3) % L) for i, k in enumerate(kinds)], seed=seed)


def width64():
    return _width([1] * 32, 6)


def width32b():
    return _width([2] * 32, 7)


def width33():
    return _width([2] * 20 + [1] + [2] * 11, 8)


def width63():
    return _width([1] * 9 + [2] + [1] * 22, 9)


def _mask(L, seed):
    """four measurements whose landmarks lie in the last word of the used-landmark mask"""
    # 40 m out the ring's neighbours are 1 m apart, eight sigma of what the pose, the landmark and the measurement allow
    return _scene([[0, 0, 0.2]], np.diag([0.01, 0.01, 1e-6]), _ring(L, r0=40.0), 1e-3, [(0, 1, L - 1 - k) for k in range(4)], seed=seed)


def two_poses():
    """observations from two poses whose cross-covariance is not zero"""
    A = np.array([[0.2, 0, 0, 0, 0, 0], [0, 0.2, 0, 0, 0, 0], [0, 0, 0.01, 0, 0, 0],
                  [0.15, 0.02, 0, 0.1, 0, 0], [-0.02, 0.15, 0, 0, 0.1, 0], [0, 0, 0.008, 0, 0, 0.005]])
    return _scene([[0, 0, 0.2], [1.0, 0.5, 0.4]], A @ A.T, _ring(5), 1e-3, [(0, 1, 0), (1, 1, 2), (0, 2, 4), (1, 1, 1), (1, 1, [0.5, 0.5])], seed=13)


def row(M=8, L=12, seed=14, x_var=4.0):
    """M measurements of L landmarks 0.5 m apart in a row along the line of sight, the pose's variance along it x_var: the
    whole row shifted by one landmark is admissible as well."""
    lms = [[3.0 + 0.5 * k, 0.0] for k in range(L)]
    first = (L - M) // 2
    return _scene([[0, 0, 0]], np.diag([x_var, 0.01, 1e-4]), lms, 1e-4, [(0, 1, first + i) for i in range(M)], seed=seed)


def decoy_row(M=32, L=256, seed=16, x_var=1e4):
    """The row with a trap for the greedy hypothesis (tools/gpu_jcbb_time.py; not a test case): the last landmark is a decoy a
    quarter of the spacing off the row's lattice and measurement 0 lies exactly on it, while the other measurements see the
    row from a pose a quarter of the spacing back.  The greedy hypothesis pairs measurement 0 with the decoy and then nothing
    else (every other pairing implies a shift the decoy's contradicts), so its count is 1 and in the first round no root is
    left at its root node for the count."""
    lms = [[3.0 + 0.5 * k, 0.0] for k in range(L - 1)]
    first = (L - 1 - M) // 2
    decoy = [lms[first][0] + 0.25, 0.0]
    return _scene([[0, 0, 0]], np.diag([x_var, 0.01, 1e-4]), lms + [decoy], 1e-4,
                  [(0, 1, decoy)] + [(0, 1, [lms[first + i][0] + 0.25, 0.0]) for i in range(1, M)], sig_xy=0.02, seed=seed)


def graph_scene(g, seed=15):
    """A scan for the graph form on a case of tests/assoc_cases.py: the first free pose whose nearest landmark is at least
    0.8 m away (at the truth) observes its 6 nearest landmarks -- five as xy, the sixth as a bearing -- and makes one spurious xy
    measurement behind itself; the candidates are those 6 and the next 2 (distractors).  The measurements are the true
    relative positions plus noise at half the standard deviation of the information of the graph's own first edges of each
    kind.  Returns dict(pose, lms [8], kinds [7], meas [7, 3], info [7, 6], truth [7])."""
    rng = np.random.default_rng(seed)
    t, vk, ek = g["truth"], g["vk"], g["ek"]
    points = np.flatnonzero(vk == 1)
    for pose in np.flatnonzero((vk == 0) & (g["fixed"] == 0)):
        d = np.hypot(*(t[points, :2] - t[pose, :2]).T)
        if np.sort(d)[0] >= 0.8:
            break
    near = points[np.argsort(d, kind="stable")[:8]]
    c, s = np.cos(t[pose, 2]), np.sin(t[pose, 2])
    rel = (t[near, :2] - t[pose, :2]) @ np.array([[c, -s], [s, c]])
    i_xy = g["info"][np.flatnonzero(ek == 1)[:6]][:, [0, 1, 3]]
    w_b = float(g["info"][np.flatnonzero(ek == 2)[0], 0])
    kinds = np.array([1, 1, 1, 1, 1, 2, 1], np.uint8)
    meas, info = np.zeros((7, 3)), np.zeros((7, 6))
    for i in range(7):
        if kinds[i] == 1:
            W = np.linalg.inv(np.array([[i_xy[i % 6, 0], i_xy[i % 6, 1]], [i_xy[i % 6, 1], i_xy[i % 6, 2]]]))
            z = rel[i] if i < 6 else -1.5 * rel[0]
            meas[i, :2] = z + 0.5 * np.linalg.cholesky(W) @ rng.standard_normal(2)
            info[i, [0, 1, 3]] = i_xy[i % 6]
        else:
            meas[i, 0] = np.arctan2(rel[i, 1], rel[i, 0]) + 0.5 / np.sqrt(w_b) * rng.standard_normal()
            info[i, 0] = w_b
    return dict(pose=int(pose), lms=near.astype(np.int32), kinds=kinds, meas=meas, info=info,
                truth=[int(v) for v in near[:6]] + [-1])


def _answer(P):
    return P["answer"]


def _reach_crossed(P):
    return P["greedy"][0] == [1, -1] and _answer(P)[0] == [0, 1] and RJ.crossed_nearest_neighbour(P) == [1, 0]


def _reach_paired(P):
    return _answer(P)[0] == P["truth"] and _answer(P)[1] == sum(1 for t in P["truth"] if t >= 0)


def _reach_spurious(P):
    return all(len(c) == 0 for c in RJ.candidates(P, RJ.individual(P))) and np.all(np.isfinite(RJ.individual(P)))


def _reach_fixed(P):
    return _reach_paired(P) and np.all(P["sigma"][:3] == 0) and np.all(P["R"][:, 0] > 0) and -1 in P["truth"]


def _reach_noinfo(P):
    return np.all(P["sigma"] == 0) and np.all(P["R"] == 0) and np.all(np.isnan(RJ.individual(P))) and _answer(P)[1] == 0


def _reach_width(D):
    return lambda P: _reach_paired(P) and _answer(P)[3] == D and P["M"] == 32


def _reach_mask(P):
    L = P["L"]
    return _reach_paired(P) and max(P["truth"]) == L - 1 and (L == 65 or min(P["truth"]) >= 64 * ((L - 1) // 64))


def _reach_two(P):
    return P["nA"] == 2 and np.abs(P["sigma"][3:6, 0:3]).max() > 0.01 and _reach_paired(P) and set(P["slot"].tolist()) == {0, 1}


def _reach_row(P):
    n = [len(c) for c in RJ.candidates(P, RJ.individual(P))]
    return _answer(P)[1] == P["M"] and np.isfinite(P["run"].gap) and min(n) >= 5


# name -> (builder, what it is there for, reach, exhaustive?)
CASES = {
    "crossed": (crossed, "nearest neighbour pairs both measurements with the wrong landmarks, greedy one of them", _reach_crossed),
    "m1l1": (m1l1, "one measurement, one landmark", _reach_paired),
    "m1l3": (m1l3, "one measurement, three landmarks", _reach_paired),
    "spurious": (spurious, "every measurement spurious: no root at all", _reach_spurious),
    "fixed_pose": (fixed_pose, "a fixed observing pose with information; one spurious measurement, one bearing", _reach_fixed),
    "fixed_noinfo": (fixed_noinfo, "fixed pose, fixed landmarks, no information: NaN, incompatible", _reach_noinfo),
    "width64": (width64, "32 xy observations: D = 64, the full wavefront", _reach_width(64)),
    "width32b": (width32b, "32 bearings: D = 32", _reach_width(32)),
    "width33": (width33, "31 bearings and one xy: D = 33", _reach_width(33)),
    "width63": (width63, "31 xy and one bearing: D = 63", _reach_width(63)),
    "mask64": (lambda: _mask(64, 10), "L = 64: one mask word, the matches at its end", _reach_mask),
    "mask65": (lambda: _mask(65, 11), "L = 65: the last landmark alone in the second mask word", _reach_mask),
    "mask256": (lambda: _mask(256, 12), "L = 256: the matches in the fourth mask word", _reach_mask),
    "two_poses": (two_poses, "observations from two correlated poses", _reach_two),
    "row": (row, "8 measurements of 12 landmarks in a row: many admissible maximum-count hypotheses", _reach_row),
}
SMALL = [n for n in ("crossed", "m1l1", "m1l3", "spurious", "fixed_pose", "fixed_noinfo", "two_poses")]

_BUILT = {}


def case(name):
    """The case's problem with the reference's answer, built once (callers must not modify it): P["answer"] = (h, count,
    d2, dof) of the sequential JCBB, P["greedy"] likewise, P["run"] the reference's Run (margin, gap, dis)."""
    if name not in _BUILT:
        P = CASES[name][0]()
        run = RJ.Run()
        P["greedy"] = RJ.greedy(P, run)
        P["answer"] = RJ.jcbb(P, run)
        P["run"] = run
        _BUILT[name] = P
    return _BUILT[name]
