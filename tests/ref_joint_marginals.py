"""Float64 numpy reference for the joint / pairwise marginal covariances and the relative-pose uncertainty built on them
(cgmr_marginals_joint, cgmr_marginals_pairs, cgmr_relative_covariance).  TEST INFRASTRUCTURE ONLY.

Blocks of H^-1: the dense inverse of ref_numpy.build_system's H on tiny graphs; on larger ones full columns of H^-1 solved
with SuperLU and refined twice with a long double residual (ref_numpy._refine_solve), whose last correction is the
reference's own error estimate.  The relative pose z = x_a^-1 x_b, its Jacobians for the additive (x, y, theta) update and
the first-order covariance and Mahalanobis distance are written out from their definitions."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import ref_numpy as R


# ------------------------------------------------------------------------------------------- the hand-worked chain
CHAIN_N = 6
CHAIN_INFO = (100.0, 100.0, 1000.0)


def chain_graph():
    """6 poses at (k, 0, 0), vertex 0 fixed, odometry edges k -> k + 1 measuring (1, 0, 0) with information
    diag(100, 100, 1000).  With every heading zero the free poses are a random walk over independent steps (dx_i, dy_i, dth_i),
    i = 1..k: x_k = sum dx_i, th_k = sum dth_i, y_k = sum dy_i + sum (k - i) dth_i (step i turns every unit step behind it), so

        cov(x_j, x_k) = min(j, k) / 100                     cov(th_j, th_k) = min(j, k) / 1000
        cov(th_j, y_k) = sum_{i <= min(j, k)} (k - i) / 1000

    e.g. Sigma_24[2, 1] = cov(th_2, y_4) = (3 + 2) / 1000 and Sigma_24[1, 2] = cov(y_2, th_4) = 1 / 1000: not symmetric."""
    n = CHAIN_N
    poses = np.zeros((n, 3))
    poses[:, 0] = np.arange(n)
    fixed = np.zeros(n, dtype=np.uint8)
    fixed[0] = 1
    ef = np.arange(n - 1, dtype=np.int32)
    et = ef + 1
    meas = np.tile([1.0, 0.0, 0.0], (n - 1, 1))
    info = np.tile([CHAIN_INFO[0], 0.0, 0.0, CHAIN_INFO[1], 0.0, CHAIN_INFO[2]], (n - 1, 1))
    return dict(poses=poses, fixed=fixed, edge_from=ef, edge_to=et, meas=meas, info=info)


# ------------------------------------------------------------------------------------------- blocks of H^-1
def _system(poses, fixed, ef, et, meas, info):
    fx = R.active_fixed(len(poses), fixed, ef, et)
    H, _, hidx = R.build_system(np.asarray(poses, dtype=np.float64), fx, ef, et, meas, info)
    return H, hidx


def _gather(cols, hidx, query):
    """[3 nK, 3 nK] in query order from `cols[v]` = the 3 columns of H^-1 of live vertex v (n x 3)."""
    nK = len(query)
    out = np.zeros((3 * nK, 3 * nK))
    for k, vk in enumerate(query):
        if hidx[vk] < 0:
            continue
        for l, vl in enumerate(query):
            if hidx[vl] < 0:
                continue
            out[3 * k:3 * k + 3, 3 * l:3 * l + 3] = cols[int(vl)][3 * hidx[vk]:3 * hidx[vk] + 3]
    return out


def joint_dense(poses, fixed, ef, et, meas, info, query):
    """The joint covariance [3 nK, 3 nK] of the query vertices from np.linalg.inv of the dense H.  Fixed / inactive
    vertices: zero rows and columns."""
    H, hidx = _system(poses, fixed, ef, et, meas, info)
    Hinv = np.linalg.inv(H.toarray())
    cols = {int(v): Hinv[:, 3 * hidx[v]:3 * hidx[v] + 3] for v in set(int(q) for q in query) if hidx[v] >= 0}
    return _gather(cols, hidx, query)


def joint_refined(poses, fixed, ef, et, meas, info, query):
    """The same from refined columns of H^-1.  Returns (cov [3 nK, 3 nK], err [3 nK, 3 nK]): err holds the last correction
    of the refinement, gathered the same way -- the reference's own absolute error estimate, element by element."""
    H, hidx = _system(poses, fixed, ef, et, meas, info)
    live = sorted(set(int(v) for v in query if hidx[v] >= 0))
    cols, errs = {}, {}
    if live:
        H = sp.csc_matrix(H)
        lu = spla.splu(H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        n = H.shape[0]
        for c0 in range(0, len(live), 64):
            vs = live[c0:c0 + 64]
            B = np.zeros((n, 3 * len(vs)))
            for j, v in enumerate(vs):
                B[3 * hidx[v]:3 * hidx[v] + 3, 3 * j:3 * j + 3] = np.eye(3)
            X, D = R._refine_solve(H, lu, B)
            for j, v in enumerate(vs):
                cols[v] = X[:, 3 * j:3 * j + 3]
                errs[v] = D[:, 3 * j:3 * j + 3]
    return _gather(cols, hidx, query), _gather(errs, hidx, query)


def block_errors(got, ref):
    """Per 3x3 block (k, l) of two [3 nK, 3 nK] matrices: ||got - ref||_F / sqrt(||ref_kk||_F ||ref_ll||_F); blocks with a
    zero diagonal block in the reference (fixed / inactive vertices) must be exactly zero in `got` and report 0."""
    nK = ref.shape[0] // 3
    b = lambda M, k, l: M[3 * k:3 * k + 3, 3 * l:3 * l + 3]   # noqa: E731
    nd = np.array([np.linalg.norm(b(ref, k, k)) for k in range(nK)])
    err = np.zeros((nK, nK))
    for k in range(nK):
        for l in range(nK):
            if nd[k] == 0 or nd[l] == 0:
                assert np.all(b(got, k, l) == 0), (k, l)
                continue
            err[k, l] = np.linalg.norm(b(got, k, l) - b(ref, k, l)) / np.sqrt(nd[k] * nd[l])
    return err


# ------------------------------------------------------------------------------------------- relative pose
def relative_pose(xa, xb):
    """z = x_a^-1 x_b, arrays [..., 3]."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    c, s = np.cos(xa[..., 2]), np.sin(xa[..., 2])
    dx, dy = xb[..., 0] - xa[..., 0], xb[..., 1] - xa[..., 1]
    return np.stack([c * dx + s * dy, -s * dx + c * dy, R.normalize_theta(xb[..., 2] - xa[..., 2])], axis=-1)


def relative_jacobians(xa, xb):
    """(J_a, J_b) [..., 3, 3]: the derivatives of z = x_a^-1 x_b with respect to additive updates of (x, y, theta) of x_a and
    x_b (EdgeSE2's Jacobians with a zero measurement)."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    c, s = np.cos(xa[..., 2]), np.sin(xa[..., 2])
    dx, dy = xb[..., 0] - xa[..., 0], xb[..., 1] - xa[..., 1]
    Ja = np.zeros(xa.shape[:-1] + (3, 3))
    Jb = np.zeros_like(Ja)
    Ja[..., 0, 0] = -c; Ja[..., 0, 1] = -s; Ja[..., 0, 2] = -s * dx + c * dy
    Ja[..., 1, 0] = s; Ja[..., 1, 1] = -c; Ja[..., 1, 2] = -c * dx - s * dy
    Ja[..., 2, 2] = -1
    Jb[..., 0, 0] = c; Jb[..., 0, 1] = s
    Jb[..., 1, 0] = -s; Jb[..., 1, 1] = c
    Jb[..., 2, 2] = 1
    return Ja, Jb


def relative_cov(xa, xb, Saa, Sab, Sbb):
    """Sigma_z = J_a Saa J_a^T + J_a Sab J_b^T + J_b Sab^T J_a^T + J_b Sbb J_b^T, arrays [..., 3, 3]."""
    Ja, Jb = relative_jacobians(xa, xb)
    T = lambda M: np.swapaxes(M, -1, -2)   # noqa: E731
    return Ja @ Saa @ T(Ja) + Ja @ Sab @ T(Jb) + Jb @ T(Sab) @ T(Ja) + Jb @ Sbb @ T(Jb)


def relative_cov_scale(xa, xb, Saa, Sab, Sbb):
    """||J_a||^2 ||Saa|| + 2 ||J_a|| ||J_b|| ||Sab|| + ||J_b||^2 ||Sbb|| (Frobenius): the size of the terms Sigma_z is the sum
    of -- for nearby poses they cancel, and rounding errors scale with them, not with the result."""
    Ja, Jb = relative_jacobians(xa, xb)
    nrm = lambda M: np.linalg.norm(M, axis=(-2, -1))   # noqa: E731
    return nrm(Ja) ** 2 * nrm(Saa) + 2 * nrm(Ja) * nrm(Jb) * nrm(Sab) + nrm(Jb) ** 2 * nrm(Sbb)


def hypothesis_error(z, zh):
    """(e, J_e): the EdgeSE2 error of the measurement zh at the relative pose z, e = zh^-1 z, and de / dz."""
    z, zh = np.asarray(z, dtype=np.float64), np.asarray(zh, dtype=np.float64)
    c, s = np.cos(zh[..., 2]), np.sin(zh[..., 2])
    tx, ty = z[..., 0] - zh[..., 0], z[..., 1] - zh[..., 1]
    e = np.stack([c * tx + s * ty, -s * tx + c * ty, R.normalize_theta(z[..., 2] - zh[..., 2])], axis=-1)
    Je = np.zeros(z.shape[:-1] + (3, 3))
    Je[..., 0, 0] = c; Je[..., 0, 1] = s
    Je[..., 1, 0] = -s; Je[..., 1, 1] = c
    Je[..., 2, 2] = 1
    return e, Je


def mahalanobis(z, Sz, zh, info_upper=None):
    """d2 = e^T (J_e Sigma_z J_e^T + Omega^-1)^-1 e per pair (no Omega term with info_upper None); NaN where that matrix is
    not positive definite.  Returns (d2 [n], S [n, 3, 3])."""
    e, Je = hypothesis_error(z, zh)
    S = Je @ Sz @ np.swapaxes(Je, -1, -2)
    if info_upper is not None:
        S = S + np.linalg.inv(R.info_full(np.asarray(info_upper, dtype=np.float64).reshape(-1, 6)))
    d2 = np.full(len(e), np.nan)
    for k in range(len(e)):
        Sk = 0.5 * (S[k] + S[k].T)
        if np.all(np.isfinite(Sk)) and np.linalg.eigvalsh(Sk).min() > 0:
            d2[k] = e[k] @ np.linalg.solve(Sk, e[k])
    return d2, S
