"""Independent numpy/scipy restatement of the g2o Gauss-Newton step for SE2 pose
graphs.  TEST INFRASTRUCTURE ONLY: it cross-checks the C
oracle (oracle/gn_oracle.c) and generates the golden fixtures under
tests/golden/ (tools/make_golden.py).  It is deliberately written a different
way from the C oracle (vectorised assembly, SuperLU factorisation, dense
inverse for marginals) so that agreement between the two means something.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def normalize_theta(t):
    t = np.asarray(t, dtype=np.float64)
    return np.where((t >= -np.pi) & (t < np.pi), t, t - 2 * np.pi * np.floor((t + np.pi) / (2 * np.pi)))


def info_full(info_upper):
    E = info_upper.shape[0]
    O = np.empty((E, 3, 3))
    O[:, 0, 0] = info_upper[:, 0]
    O[:, 0, 1] = O[:, 1, 0] = info_upper[:, 1]
    O[:, 0, 2] = O[:, 2, 0] = info_upper[:, 2]
    O[:, 1, 1] = info_upper[:, 3]
    O[:, 1, 2] = O[:, 2, 1] = info_upper[:, 4]
    O[:, 2, 2] = info_upper[:, 5]
    return O


def edge_errors(poses, ef, et, meas):
    """e = (z^-1 * (xi^-1 * xj)).toVector()  (EdgeSE2::computeError)."""
    xi, xj = poses[ef], poses[et]
    ci, si = np.cos(xi[:, 2]), np.sin(xi[:, 2])
    dx = xj[:, 0] - xi[:, 0]
    dy = xj[:, 1] - xi[:, 1]
    rx = ci * dx + si * dy
    ry = -si * dx + ci * dy
    rth = normalize_theta(xj[:, 2] - xi[:, 2])
    cz, sz = np.cos(meas[:, 2]), np.sin(meas[:, 2])
    ex = cz * (rx - meas[:, 0]) + sz * (ry - meas[:, 1])
    ey = -sz * (rx - meas[:, 0]) + cz * (ry - meas[:, 1])
    eth = normalize_theta(rth - meas[:, 2])
    return np.stack([ex, ey, eth], axis=1)


def jacobians(poses, ef, et, meas):
    xi, xj = poses[ef], poses[et]
    c, s = np.cos(xi[:, 2]), np.sin(xi[:, 2])
    dx = xj[:, 0] - xi[:, 0]
    dy = xj[:, 1] - xi[:, 1]
    E = len(ef)
    A = np.zeros((E, 3, 3))
    B = np.zeros((E, 3, 3))
    A[:, 0, 0] = -c; A[:, 0, 1] = -s; A[:, 0, 2] = -s * dx + c * dy
    A[:, 1, 0] = s;  A[:, 1, 1] = -c; A[:, 1, 2] = -c * dx - s * dy
    A[:, 2, 2] = -1
    B[:, 0, 0] = c; B[:, 0, 1] = s
    B[:, 1, 0] = -s; B[:, 1, 1] = c
    B[:, 2, 2] = 1
    cz, sz = np.cos(meas[:, 2]), np.sin(meas[:, 2])
    Z = np.zeros((E, 3, 3))
    Z[:, 0, 0] = cz; Z[:, 0, 1] = sz
    Z[:, 1, 0] = -sz; Z[:, 1, 1] = cz
    Z[:, 2, 2] = 1
    Ji, Jj = Z @ A, Z @ B
    # an edge from a vertex to itself is the chain rule's term: e = z^-1 (xi^-1 xi) with the one Jacobian Ji + Jj on the one
    # block, H_ii += (Ji + Jj)^T Omega (Ji + Jj) and b_i likewise.  (e does not depend on xi: the sum is zero, the edge adds
    # to chi2 only.)  Carried by Ji; Jj is cleared so that build_system's four blocks add up to exactly that term
    self_edge = np.asarray(ef) == np.asarray(et)
    Ji[self_edge] += Jj[self_edge]
    Jj[self_edge] = 0
    return Ji, Jj


def chi2(poses, ef, et, meas, info_upper):
    e = edge_errors(poses, ef, et, meas)
    O = info_full(info_upper)
    return float(np.einsum("ei,eij,ej->", e, O, e))


def build_system(poses, fixed, ef, et, meas, info_upper):
    """Returns (H csc over free scalars, b, index map vertex->hessian index)."""
    V = poses.shape[0]
    free = np.flatnonzero(fixed == 0)
    hidx = -np.ones(V, dtype=np.int64)
    hidx[free] = np.arange(len(free))
    e = edge_errors(poses, ef, et, meas)
    Ji, Jj = jacobians(poses, ef, et, meas)
    O = info_full(info_upper)
    JiO = np.transpose(Ji, (0, 2, 1)) @ O
    JjO = np.transpose(Jj, (0, 2, 1)) @ O
    Hii, Hij, Hjj = JiO @ Ji, JiO @ Jj, JjO @ Jj
    bi = -(JiO @ e[:, :, None])[:, :, 0]
    bj = -(JjO @ e[:, :, None])[:, :, 0]
    n = 3 * len(free)
    rows, cols, vals = [], [], []
    b = np.zeros(n)
    hi, hj = hidx[ef], hidx[et]
    rr, cc = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")

    def add(block, r, c, mask):
        rows.append((3 * r[mask, None, None] + rr).ravel())
        cols.append((3 * c[mask, None, None] + cc).ravel())
        vals.append(block[mask].ravel())

    mi, mj = hi >= 0, hj >= 0
    add(Hii, hi, hi, mi)
    add(Hjj, hj, hj, mj)
    both = mi & mj
    add(Hij, hi, hj, both)
    add(np.transpose(Hij, (0, 2, 1)), hj, hi, both)
    np.add.at(b, (3 * hi[mi, None] + np.arange(3)).ravel(), bi[mi].ravel())
    np.add.at(b, (3 * hj[mj, None] + np.arange(3)).ravel(), bj[mj].ravel())
    H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()
    return H, b, hidx


def gn_optimize(poses, fixed, ef, et, meas, info_upper, iters):
    """n Gauss-Newton iterations (no damping, no stopping rule).  Returns the
    new poses and chi2 before each iteration plus after the last one."""
    poses = np.array(poses, dtype=np.float64, copy=True)
    chis = [chi2(poses, ef, et, meas, info_upper)]
    for _ in range(iters):
        H, b, hidx = build_system(poses, fixed, ef, et, meas, info_upper)
        dx = spla.splu(H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0,
                       options=dict(SymmetricMode=True)).solve(b)
        free = hidx >= 0
        d = dx.reshape(-1, 3)
        poses[free, 0] += d[:, 0]
        poses[free, 1] += d[:, 1]
        poses[free, 2] = normalize_theta(poses[free, 2] + d[:, 2])
        chis.append(chi2(poses, ef, et, meas, info_upper))
    return poses, np.array(chis)


def marginals_dense(poses, fixed, ef, et, meas, info_upper, query):
    """3x3 diagonal blocks of H^-1 at the current linearisation point (dense)."""
    H, _, hidx = build_system(poses, fixed, ef, et, meas, info_upper)
    Hinv = np.linalg.inv(H.toarray())
    out = np.zeros((len(query), 3, 3))
    for k, v in enumerate(query):
        h = hidx[v]
        if h >= 0:
            out[k] = Hinv[3 * h:3 * h + 3, 3 * h:3 * h + 3]
    return out


# ---------------------------------------------------------------------------- yardsticks that need no second solver

U = np.finfo(np.float64).eps / 2            # unit roundoff of float64


def _edge_magnitudes(poses, ef, et, meas):
    """Componentwise magnitudes of the terms e and J_i, J_j are computed from (computeError / linearizeOplus of Appendix
    A): their rounding is relative to these, not to the results, which cancel -- e of a consistent edge is ~0 while its
    terms are the size of the edge.  (t_j - t_i and theta_j - theta_i are single roundings of exact inputs: relative to
    themselves; the raw angle difference also covers a normalisation by 2 pi.)"""
    d = np.abs(poses[et] - poses[ef])
    c, s = np.abs(np.cos(poses[ef, 2])), np.abs(np.sin(poses[ef, 2]))
    cz, sz = np.abs(np.cos(meas[:, 2])), np.abs(np.sin(meas[:, 2]))
    tx, ty = d[:, 0], d[:, 1]
    rx, ry = c * tx + s * ty + np.abs(meas[:, 0]), s * tx + c * ty + np.abs(meas[:, 1])
    e = np.stack([cz * rx + sz * ry, sz * rx + cz * ry, d[:, 2] + np.abs(meas[:, 2])], axis=1)
    E = len(ef)
    A = np.zeros((E, 3, 3))
    B = np.zeros((E, 3, 3))
    A[:, 0, 0] = c; A[:, 0, 1] = s; A[:, 0, 2] = s * tx + c * ty
    A[:, 1, 0] = s; A[:, 1, 1] = c; A[:, 1, 2] = c * tx + s * ty
    A[:, 2, 2] = 1
    B[:, 0, 0] = c; B[:, 0, 1] = s
    B[:, 1, 0] = s; B[:, 1, 1] = c
    B[:, 2, 2] = 1
    Z = np.zeros((E, 3, 3))
    Z[:, 0, 0] = cz; Z[:, 0, 1] = sz
    Z[:, 1, 0] = sz; Z[:, 1, 1] = cz
    Z[:, 2, 2] = 1
    return e, Z @ A, Z @ B


def _assemble_abs(poses, fixed, ef, et, meas, info_upper, hidx, n):
    """|H| and |b| as assembled: H_abs = sum_e |J_e|^T |Omega_e| |J_e|, b_abs = sum_e |J_e|^T |Omega_e| |e_e|, with |J|
    and |e| the magnitudes of the terms they are computed from (_edge_magnitudes): they bound the rounding of
    linearisation and summation."""
    e, Ji, Jj = _edge_magnitudes(poses, ef, et, meas)
    O = np.abs(info_full(info_upper))
    JiO, JjO = np.transpose(Ji, (0, 2, 1)) @ O, np.transpose(Jj, (0, 2, 1)) @ O
    Hii, Hij, Hjj = JiO @ Ji, JiO @ Jj, JjO @ Jj
    bi, bj = (JiO @ e[:, :, None])[:, :, 0], (JjO @ e[:, :, None])[:, :, 0]
    hi, hj = hidx[ef], hidx[et]
    mi, mj = hi >= 0, hj >= 0
    both = mi & mj
    rr, cc = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    rows = np.concatenate([(3 * h[m, None, None] + rr).ravel() for h, m in ((hi, mi), (hj, mj), (hi, both), (hj, both))])
    cols = np.concatenate([(3 * h[m, None, None] + cc).ravel() for h, m in ((hi, mi), (hj, mj), (hj, both), (hi, both))])
    vals = np.concatenate([Hii[mi].ravel(), Hjj[mj].ravel(), Hij[both].ravel(), np.transpose(Hij, (0, 2, 1))[both].ravel()])
    H_abs = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    b_abs = np.zeros(n)
    np.add.at(b_abs, (3 * hi[mi, None] + np.arange(3)).ravel(), bi[mi].ravel())
    np.add.at(b_abs, (3 * hj[mj, None] + np.arange(3)).ravel(), bj[mj].ravel())
    return H_abs, b_abs


def active_fixed(nV, fixed, ef, et):
    """The fixed flags with every vertex no edge touches added: such vertices are inactive (no row of H)."""
    touched = np.zeros(nV, dtype=bool)
    touched[np.asarray(ef)] = True
    touched[np.asarray(et)] = True
    return ((np.asarray(fixed) != 0) | ~touched).astype(np.uint8)


def step_backward_error(poses0, poses1, fixed, ef, et, meas, info_upper, H=None, b=None):
    """Componentwise backward error of the Gauss-Newton step poses0 -> poses1 as a solve of H dx = b (H, b assembled at
    poses0 by build_system, or given):

        omega = max_i max(|H dx - b|_i - (H_abs s)_i, 0) / (H_abs |dx| + b_abs)_i,   s = u (|poses0| + |poses1|)

    H_abs s is the residual the rounding of the pose update alone leaves (it does not shrink with the step: near the
    optimum it is the largest term, ~2000 u of the denominator on pg9000).  The residual is formed in long double.  A
    backward-stable solve gives omega of a few u; a step with one wrong term in it gives roughly that term's relative size
    -- as long as that exceeds the allowance.  From the initial guess a 1e-9 error in one block shows; once the steps are
    small (a 3rd iterate on) the allowance hides most such errors, and omega = 0 there means "below the allowance", not
    "exact".  Vertices no edge touches are left out."""
    poses0 = np.asarray(poses0, dtype=np.float64)
    poses1 = np.asarray(poses1, dtype=np.float64)
    fx = active_fixed(len(poses0), fixed, ef, et)
    H0, b0, hidx = build_system(poses0, fx, ef, et, meas, info_upper)
    if H is None:
        H, b = H0, b0
    n = H.shape[0]
    if n == 0:
        return 0.0
    free = hidx >= 0
    d = poses1[free] - poses0[free]
    d[:, 2] = normalize_theta(d[:, 2])
    # the update normalises the heading: a far-from-optimum step that turns a vertex by more than pi comes back 2 pi short.
    # The branch is taken from a reference solve (a multiple of 2 pi: it cannot hide an error smaller than pi)
    ref = spla.splu(sp.csc_matrix(H), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0,
                    options=dict(SymmetricMode=True)).solve(np.asarray(b, dtype=np.float64)).reshape(-1, 3)
    d[:, 2] += 2 * np.pi * np.round((ref[:, 2] - d[:, 2]) / (2 * np.pi))
    dx = d.ravel()
    Hc = sp.coo_matrix(H)
    r = -np.asarray(b, dtype=np.longdouble).copy()
    np.add.at(r, Hc.row, Hc.data.astype(np.longdouble) * dx[Hc.col].astype(np.longdouble))
    H_abs, b_abs = _assemble_abs(poses0, fx, ef, et, meas, info_upper, hidx, n)
    den = H_abs @ np.abs(dx) + b_abs
    # the update rounds poses0 + dx into poses1 (and the heading by a normalisation): dx comes back off by up to
    # u (|poses0| + |poses1|) (+ 2 pi u for the heading) whatever the solve did -- an absolute allowance, not scaled by omega
    slack = U * (np.abs(poses0[free]) + np.abs(poses1[free]))
    slack[:, 2] += 2 * np.pi * U
    res = np.maximum(np.abs(r).astype(np.float64) - H_abs @ slack.ravel(), 0.0)
    ok = den > 0
    if np.any(res[~ok] != 0):
        return float("inf")
    return float(np.max(res[ok] / den[ok])) if ok.any() else 0.0


def _refine_solve(H, lu, B, steps=2):
    """X with H X = B by the LU factor `lu`, then `steps` rounds of iterative refinement with the residual in long double.
    Returns (X, the last correction)."""
    X = lu.solve(B)
    Hc = sp.coo_matrix(H)
    hv = Hc.data.astype(np.longdouble)
    D = np.zeros_like(X)
    for _ in range(steps):
        R = np.asarray(B, dtype=np.longdouble).copy()
        np.subtract.at(R, Hc.row, hv[:, None] * X[Hc.col].astype(np.longdouble))
        D = lu.solve(R.astype(np.float64))
        X = X + D
    return X, D


def marginal_blocks_ref(H, hidx, query):
    """3x3 diagonal blocks of H^-1 for the query vertices: the 3 columns of each query solved with SuperLU and refined
    twice (residual in long double, whose 64-bit mantissa bounds what refinement reaches: ~cond(H) 2^-64, 1.3e-12 of a
    block on a 1500-vertex C2-recipe graph).  Returns (blocks[nq,3,3], err[nq]): err is the Frobenius norm of the block's last correction relative
    to the block's own -- the block's own error estimate.  Fixed / inactive queries (hidx < 0) give zeros."""
    query = np.asarray(query)
    out = np.zeros((len(query), 3, 3))
    err = np.zeros(len(query))
    live = [k for k, v in enumerate(query) if hidx[v] >= 0]
    if not live:
        return out, err
    H = sp.csc_matrix(H)
    lu = spla.splu(H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    n = H.shape[0]
    for c0 in range(0, len(live), 64):                        # 64 queries (192 columns) at a time
        ks = live[c0:c0 + 64]
        B = np.zeros((n, 3 * len(ks)))
        for j, k in enumerate(ks):
            h = hidx[query[k]]
            B[3 * h:3 * h + 3, 3 * j:3 * j + 3] = np.eye(3)
        X, D = _refine_solve(H, lu, B)
        for j, k in enumerate(ks):
            h = hidx[query[k]]
            out[k] = X[3 * h:3 * h + 3, 3 * j:3 * j + 3]
            err[k] = np.linalg.norm(D[3 * h:3 * h + 3, 3 * j:3 * j + 3]) / np.linalg.norm(out[k])
    return out, err


def _se2_inv(a):
    c, s = np.cos(a[..., 2]), np.sin(a[..., 2])
    return np.stack([-(c * a[..., 0] + s * a[..., 1]), -(-s * a[..., 0] + c * a[..., 1]), -a[..., 2]], axis=-1)


def _se2_mul(a, b):
    c, s = np.cos(a[..., 2]), np.sin(a[..., 2])
    return np.stack([a[..., 0] + c * b[..., 0] - s * b[..., 1], a[..., 1] + s * b[..., 0] + c * b[..., 1],
                     normalize_theta(a[..., 2] + b[..., 2])], axis=-1)


def label_edges_ut(xg, xv, Sigma, alpha=1e-3, beta=2.0, kappa=0.0):
    """The unscented labelling of star edges gauge -> v (EdgeLabeler): z := xg^-1 xv; the 2n+1 = 7
    sigma points of N(0, Sigma) with lambda = alpha^2 (n + kappa) as the appendix states (alpha^2 n for kappa = 0),
    L = chol((n + lambda) Sigma), points 0, +-L[:, i]; each applied to v by oplus, the edge error e = z^-1 (xg^-1 xv')
    taken; their weighted mean and covariance (w_m, w_c about that mean); information = covariance^-1.

    xg (3,) or (K,3), xv (K,3), Sigma (K,3,3).  Returns (z[K,3], info_upper[K,6], not_pd[K]): where (n + lambda) Sigma
    has no Cholesky factor the edge keeps identity information and not_pd is set."""
    xv = np.atleast_2d(np.asarray(xv, dtype=np.float64))
    K = len(xv)
    xg = np.broadcast_to(np.asarray(xg, dtype=np.float64), (K, 3))
    Sigma = np.asarray(Sigma, dtype=np.float64).reshape(K, 3, 3)
    n = 3
    lam = alpha * alpha * (n + kappa)
    wm = np.full(2 * n + 1, 1.0 / (2 * (n + lam)))
    wc = wm.copy()
    wm[0] = lam / (n + lam)
    wc[0] = wm[0] + (1 - alpha * alpha + beta)
    z = _se2_mul(_se2_inv(xg), xv)
    iu = np.tile([1.0, 0, 0, 1, 0, 1], (K, 1))
    not_pd = np.zeros(K, dtype=bool)
    for k in range(K):
        try:
            L = np.linalg.cholesky((n + lam) * Sigma[k])
        except np.linalg.LinAlgError:
            not_pd[k] = True
            continue
        pts = np.concatenate([np.zeros((1, 3)), np.stack([s * L[:, i] for i in range(n) for s in (1.0, -1.0)])])
        xs = xv[k] + pts
        xs[:, 2] = normalize_theta(xs[:, 2])
        P = np.concatenate([xg[k][None], xs])
        e = edge_errors(P, np.zeros(7, np.int64), np.arange(1, 8), np.tile(z[k], (7, 1)))
        mean = wm @ e
        dev = e - mean
        C = (wc[:, None, None] * dev[:, :, None] * dev[:, None, :]).sum(axis=0)
        I = np.linalg.inv(C)
        iu[k] = [I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]]
    return z, iu, not_pd


def condense_ref(poses, ef, et, meas, info_upper, gauge, query, initial_guess):
    """CondensedGraphCreator::compute restated: the gauge alone fixed, the spanning-tree guess (`initial_guess`, a callable
    with oracle.initial_guess's signature: the linearisation point), H and b there, one step solved with SuperLU, the
    refined marginal blocks of that H, the star edges labelled at the stepped poses.  Query entries equal to the gauge are
    dropped.  Returns a dict: to, est, iu, not_pd, cov, cov_err, guess, poses1."""
    nV = len(poses)
    fixed = np.zeros(nV, np.uint8)
    fixed[gauge] = 1
    guess = np.asarray(initial_guess(poses, fixed, ef, et, meas), dtype=np.float64)
    fx = active_fixed(nV, fixed, ef, et)
    H, _, hidx = build_system(guess, fx, ef, et, meas, info_upper)
    poses1, _ = gn_optimize(guess, fx, ef, et, meas, info_upper, 1)
    to = np.array([q for q in query if q != gauge], dtype=np.int32)
    cov, cov_err = marginal_blocks_ref(H, hidx, to)
    est, iu, bad = label_edges_ut(poses1[gauge], poses1[to], cov)
    return dict(to=to, est=est, iu=iu, not_pd=bad, cov=cov, cov_err=cov_err, guess=guess, poses1=poses1)
