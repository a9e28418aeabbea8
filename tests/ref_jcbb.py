"""Float64 numpy reference of the joint-compatibility data association (include/cgmr.h: cgmr_jcbb_dense,
cgmr_joint_compatibility).  TEST INFRASTRUCTURE ONLY.

A problem is a dict: M, L, nA, slot [M], dim [M] (2 xy, 1 bearing), sigma [n, n] with n = 3 nA + 2 L (poses first), e [M, L, 2],
J [M, L, 2, 5], R [M, 3] = (R00, R01, R11), gamma [2 M + 1].  A hypothesis is a list h [M] of landmark positions or -1.

d2 of a hypothesis is computed twice, by a Cholesky solve and by np.linalg.solve; a Run collects over every test made
  margin   the smallest relative distance |d2 - gamma| / gamma of a compatibility test to its threshold
  dis      the largest relative disagreement of the two d2 methods
and the searches add gap, the relative d2 gap between the best and the second-best hypothesis of maximum count (inf: one only).

The exhaustive enumerator lists every admissible hypothesis (every pairing individually compatible, every prefix jointly
compatible); the sequential JCBB searches the same set with the bounds of the device's search; the greedy hypothesis is the
sequential pass of k_jc_greedy.  For the graph form Sigma comes from ref_assoc's system by marginal_blocks' refined solves
(the columns of the scan's vertices alone) and the predictions from ref_assoc.predict -- no device output."""
import numpy as np


class Run:
    def __init__(self):
        self.margin, self.dis, self.gap, self.tests = np.inf, 0.0, np.inf, 0


def state_idx(P, i, j):
    pb, lb = 3 * int(P["slot"][i]), 3 * P["nA"] + 2 * j
    return [pb, pb + 1, pb + 2, lb, lb + 1]


def _sym(P):
    if "_S" not in P:
        P["_S"] = np.tril(P["sigma"]) + np.tril(P["sigma"], -1).T     # the lower triangle is the matrix
    return P["_S"]


def joint(P, h):
    """(e_H [D], C_H [D, D]) of the hypothesis' pairings in observation order."""
    ix, jj, es, obs = [], [], [], []
    for i, j in enumerate(h):
        if j < 0:
            continue
        for t in range(int(P["dim"][i])):
            ix.append(state_idx(P, i, j))
            jj.append(P["J"][i, j, t])
            es.append(P["e"][i, j, t])
            obs.append((i, t))
    if not ix:
        return np.zeros(0), np.zeros((0, 0))
    IX, JJ = np.array(ix), np.array(jj)
    C = np.einsum("ap,apbq,bq->ab", JJ, _sym(P)[IX[:, :, None, None], IX[None, None, :, :]], JJ)
    C = 0.5 * (C + C.T)
    for a, (i, t) in enumerate(obs):
        for b, (k, u) in enumerate(obs):
            if i == k:
                C[a, b] += P["R"][i, t + u]
    return np.array(es), C


def d2_chol(e, C):
    """|L^-1 e|^2 with C = L L^T; NaN where C is not finite or not positive definite."""
    if len(e) == 0:
        return 0.0
    if not (np.all(np.isfinite(C)) and np.all(np.isfinite(e))):
        return float("nan")
    try:
        L = np.linalg.cholesky(C)
    except np.linalg.LinAlgError:
        return float("nan")
    y = np.linalg.solve(L, e)
    return float(y @ y)


def d2_solve(e, C):
    if len(e) == 0:
        return 0.0
    try:
        return float(e @ np.linalg.solve(C, e))
    except np.linalg.LinAlgError:
        return float("nan")


def d2_of(P, h, run=None):
    """(d2 by Cholesky, dof) of a hypothesis; the disagreement with the second method goes into run."""
    e, C = joint(P, h)
    a = d2_chol(e, C)
    if run is not None and np.isfinite(a) and len(e):
        b = d2_solve(e, C)
        run.dis = max(run.dis, abs(a - b) / max(abs(a), 1e-300))
    return a, len(e)


def passes(P, d2, dof, run=None):
    g = float(P["gamma"][dof])
    if run is not None:
        run.tests += 1
        if np.isfinite(d2):
            run.margin = min(run.margin, abs(d2 - g) / g)
    return bool(np.isfinite(d2) and d2 < g)


def individual(P, run=None):
    """ic [M, L]: d2 of every single pairing (computed once per problem; its d2 disagreement is kept with it)."""
    if "_ic" not in P:
        own = Run()
        ic = np.full((P["M"], P["L"]), np.nan)
        for i in range(P["M"]):
            for j in range(P["L"]):
                h = [-1] * P["M"]
                h[i] = j
                ic[i, j] = d2_of(P, h, own)[0]
        P["_ic"], P["_ic_dis"] = ic, own.dis
    if run is not None:
        run.dis = max(run.dis, P["_ic_dis"])
    return P["_ic"]


def candidates(P, ic, run=None):
    """per observation the individually compatible landmarks, ascending in (ic, j)"""
    out = []
    for i in range(P["M"]):
        ok = [j for j in range(P["L"]) if passes(P, ic[i, j], int(P["dim"][i]), run)]
        out.append(sorted(ok, key=lambda j: (ic[i, j], j)))
    return out


def admissible(P, h, run=None):
    """(admissible?, d2, dof) of a hypothesis under the definitions."""
    pairs = [j for j in h if j >= 0]
    if len(set(pairs)) != len(pairs):
        return False, float("nan"), 0
    ic = individual(P, run)
    d2, dof = 0.0, 0
    for i, j in enumerate(h):
        if j < 0:
            continue
        if not passes(P, ic[i, j], int(P["dim"][i]), run):
            return False, float("nan"), 0
        d2, dof = d2_of(P, list(h[:i + 1]) + [-1] * (P["M"] - i - 1), run)
        if not passes(P, d2, dof, run):
            return False, d2, dof
    return True, d2, dof


def _better(a, b):
    """(count, d2) a strictly better than b"""
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


def _gap(best, second):
    if second is None or second[0] < best[0]:
        return np.inf
    return abs(second[1] - best[1]) / max(best[1], 1e-300)


def enumerate_all(P, run=None):
    """Every admissible hypothesis as (h, count, d2, dof), the empty one included.  M <= 6, L <= 8."""
    assert P["M"] <= 6 and P["L"] <= 8
    run = run or Run()
    cand = candidates(P, individual(P, run), run)
    out = []

    def go(i, h, count, d2, dof):
        if i == P["M"]:
            out.append((list(h), count, d2, dof))
            return
        for j in cand[i]:
            if j in h:
                continue
            h2 = h[:i] + [j] + [-1] * (P["M"] - i - 1)
            d, f = d2_of(P, h2, run)
            if passes(P, d, f, run):
                go(i + 1, h2, count + 1, d, f)
        go(i + 1, h, count, d2, dof)

    go(0, [-1] * P["M"], 0, 0.0, 0)
    return out


def best_of(hyps, run=None):
    """The best (h, count, d2, dof) of a list: most pairings, then the smallest d2; the gap to the runner-up goes into run."""
    order = sorted(hyps, key=lambda x: (-x[1], x[2]))
    if run is not None:
        run.gap = _gap((order[0][1], order[0][2]), (order[1][1], order[1][2]) if len(order) > 1 else None)
    return order[0]


def greedy(P, run=None):
    """Observations in order; each takes its first candidate that is unused and keeps the hypothesis jointly compatible."""
    cand = candidates(P, individual(P, run), run)
    h, d2, dof = [-1] * P["M"], 0.0, 0
    for i in range(P["M"]):
        for j in cand[i]:
            if j in h:
                continue
            h2 = list(h)
            h2[i] = j
            d, f = d2_of(P, h2, run)
            if passes(P, d, f, run):
                h, d2, dof = h2, d, f
                break
    return h, sum(1 for j in h if j >= 0), d2, dof


def jcbb(P, run=None):
    """The sequential branch and bound with the device's rule: (h, count, d2, dof).  Candidates in ascending (ic, j), "none"
    last; a subtree is left when it cannot reach the best count, or only reaches it with a d2 not below the SECOND best's, so
    that the runner-up of maximum count is found too (run.gap)."""
    run = run or Run()
    cand = candidates(P, individual(P, run), run)
    M = P["M"]
    live = [sum(1 for k in range(i, M) if cand[k]) for i in range(M + 1)]
    g = greedy(P, run)
    best = [g]
    second = [None]

    def offer(h, count, d2, dof):
        c = (list(h), count, d2, dof)
        if c[0] == best[0][0]:
            return
        if _better((count, d2), (best[0][1], best[0][2])):
            second[0], best[0] = best[0], c
        elif second[0] is None or _better((count, d2), (second[0][1], second[0][2])):
            if second[0] is None or c[0] != second[0][0]:
                second[0] = c

    def go(i, h, count, d2, dof):
        if count:
            offer(h, count, d2, dof)
        if i == M:
            return
        reach = count + live[i]
        if reach < best[0][1]:
            return
        if reach == best[0][1] and second[0] is not None and second[0][1] == best[0][1] and not d2 < second[0][2]:
            return
        for j in cand[i]:
            if j in h:
                continue
            h2 = list(h)
            h2[i] = j
            d, f = d2_of(P, h2, run)
            if passes(P, d, f, run):
                go(i + 1, h2, count + 1, d, f)
        go(i + 1, h, count, d2, dof)

    go(0, [-1] * M, 0, 0.0, 0)
    run.gap = _gap((best[0][1], best[0][2]), None if second[0] is None else (second[0][1], second[0][2]))
    return best[0]


def crossed_nearest_neighbour(P):
    """What callers do today: measurements in order, each takes the unused individually compatible landmark of smallest ic."""
    ic = individual(P)
    cand = candidates(P, ic)
    h = [-1] * P["M"]
    for i in range(P["M"]):
        for j in cand[i]:
            if j not in h:
                h[i] = j
                break
    return h


# ------------------------------------------------------------------ problems

def predict_xy(pose, lm):
    """(z [2], J [2, 5]) of a point seen from a pose: ref_assoc.predict's kind 1 on bare coordinates."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    dx, dy = lm[0] - pose[0], lm[1] - pose[1]
    rx, ry = c * dx + s * dy, -s * dx + c * dy
    return np.array([rx, ry]), np.array([[-c, -s, ry, c, s], [s, -c, -rx, -s, c]])


def normalize(t):
    return float((t + np.pi) % (2 * np.pi) - np.pi)


def make_problem(poses, slot, kinds, zh, R, lms, sigma, gamma):
    """The dense problem of observations (pose slot, kind 1 xy / 2 bearing, measurement zh [M, 2], R [M, 3]) of the landmarks
    lms [L, 2] from poses [nA, 3] under sigma."""
    M, L, nA = len(slot), len(lms), len(poses)
    e, J = np.zeros((M, L, 2)), np.zeros((M, L, 2, 5))
    for i in range(M):
        for j in range(L):
            z, J1 = predict_xy(poses[slot[i]], lms[j])
            if kinds[i] == 1:
                e[i, j], J[i, j] = z - zh[i], J1
            else:
                q = z @ z
                Jb = (-z[1] / q) * J1[0] + (z[0] / q) * J1[1]
                Jb[2] = -1.0
                e[i, j, 0], J[i, j, 0] = normalize(np.arctan2(z[1], z[0]) - zh[i][0]), Jb
    return dict(M=M, L=L, nA=nA, slot=np.array(slot, np.int32), dim=np.array([2 if k == 1 else 1 for k in kinds], np.int32),
                sigma=np.array(sigma, dtype=np.float64), e=e, J=J, R=np.array(R, dtype=np.float64).reshape(M, 3),
                gamma=np.array(gamma[:2 * M + 1], dtype=np.float64))


def graph_problem(g, poses, obs_pose, kinds, meas, info, lms, gamma):
    """The problem of the graph form on the reference's own Sigma: observations from the vertices obs_pose [M] with meas
    [M, 3] / info [M, 6] (None: R = 0) as cgmr_observation_covariance reads a hypothesis, candidates lms (vertex indices).
    Returns (problem, the largest relative last correction of a Sigma block)."""
    import assoc_cases as AC
    import ref_assoc as A
    ups = []
    for v in obs_pose:
        if int(v) not in ups:
            ups.append(int(v))
    verts = ups + [int(l) for l in lms]
    vk, ek = AC.kinds(g)
    nA, L, M = len(ups), len(lms), len(obs_pose)
    n = 3 * nA + 2 * L
    off = [3 * k for k in range(nA)] + [3 * nA + 2 * j for j in range(L)]
    dim = [3] * nA + [2] * L
    # marginal_blocks' system, factor and refined solves (ref_typed), for the columns of these vertices alone: the joint
    # covariance needs every cross block among them, and marginal_blocks solves every column of H for a pair list
    a = AC.args(g)[1:]
    fx = A.active_fixed(len(poses), a[0], a[1], a[2])
    H, _, lay = A.build_system(poses, fx, *a[1:], vk, ek)
    S, err = np.zeros((n, n)), 0.0
    live = [x for x, v in enumerate(verts) if lay.off[v] >= 0]
    if lay.n and live:
        import scipy.sparse.linalg as spla
        import ref_numpy as R
        cols = [lay.off[verts[x]] + k for x in live for k in range(dim[x])]
        mine = [off[x] + k for x in live for k in range(dim[x])]
        E = np.zeros((lay.n, len(cols)))
        E[cols, np.arange(len(cols))] = 1.0
        lu = spla.splu(H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        X, D = R._refine_solve(H, lu, E)
        S[np.ix_(mine, mine)] = X[cols]
        for x in live:
            o, d = lay.off[verts[x]], dim[x]
            k0 = cols.index(o)
            err = max(err, float(np.linalg.norm(D[o:o + d, k0:k0 + d]) / np.linalg.norm(X[o:o + d, k0:k0 + d])))
        assert all(lay.dim[verts[x]] == dim[x] for x in live)
    S = 0.5 * (S + S.T)
    e, J = np.zeros((M, L, 2)), np.zeros((M, L, 2, 5))
    R = np.zeros((M, 3))
    for i in range(M):
        for j, l in enumerate(lms):
            z, Jk = A.predict(poses, int(obs_pose[i]), int(l), int(kinds[i]))
            d = Jk.shape[0]
            J[i, j, :d] = Jk
            if kinds[i] == 1:
                e[i, j] = z[:2] - meas[i][:2]
            else:
                e[i, j, 0] = normalize(z[0] - meas[i][0])
        if info is not None:
            u = info[i]
            if kinds[i] == 1:
                W = np.linalg.inv(np.array([[u[0], u[1]], [u[1], u[3]]]))
                R[i] = [W[0, 0], W[0, 1], W[1, 1]]
            else:
                R[i, 0] = 1.0 / u[0]
    P = dict(M=M, L=L, nA=nA, slot=np.array([ups.index(int(v)) for v in obs_pose], np.int32),
             dim=np.array([2 if k == 1 else 1 for k in kinds], np.int32), sigma=S, e=e, J=J, R=R,
             gamma=np.array(gamma[:2 * M + 1], dtype=np.float64))
    return P, err
