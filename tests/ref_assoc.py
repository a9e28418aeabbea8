"""Float64 numpy reference of the typed factors with bearing-only observations, and of landmark data association.
TEST INFRASTRUCTURE ONLY.

The system is tests/ref_typed.py's -- true dimensions, SuperLU, g2o's steps -- with one more factor:
  kind 2  EDGE_BEARING_SE2_XY   e = normalize(atan2(ry, rx) - z0),  (rx, ry) = R(theta_i)^T (l - t_i)           (1)
  J_i = (-ry / q) A[0] + (rx / q) A[1] (its theta entry is -1), J_l = (-ry / q) B[0] + (rx / q) B[1], q = rx^2 + ry^2, A / B the
  EDGE_SE2_XY Jacobians; with the point on the pose (q == 0) e = normalize(-z0) and the Jacobians are zero.  Omega = info[0].
ref_typed is not edited: its per-edge functions (errors, Jacobians, information, magnitudes) are wrapped here, and its drivers
(build_system, gn / lm / dl_optimize, step_backward_error, marginal_blocks) run with the wrapped ones in place for the
duration of a call.

Data association: the predicted observation of a vertex from a pose, S = J Sigma J^T from marginal_blocks(pairs=) -- the refined
solves, no device output -- and d2 = e^T (S + Omega^-1)^-1 e in the factor's own dimension."""
from __future__ import annotations

import contextlib
import functools

import numpy as np

import ref_numpy as R
import ref_typed as T

U = T.U
BEARING = 2
_ORIG = dict(edge_errors=T.edge_errors, jacobians=T.jacobians, info_typed=T.info_typed, _magnitudes=T._magnitudes)


def _rel(poses, ef, et, m):
    xi, xj = poses[ef][m], poses[et][m]
    c, s = np.cos(xi[:, 2]), np.sin(xi[:, 2])
    dx, dy = xj[:, 0] - xi[:, 0], xj[:, 1] - xi[:, 1]
    return c, s, dx, dy, c * dx + s * dy, -s * dx + c * dy


def info_typed(info_upper, ek):
    ek = np.asarray(ek)
    O = _ORIG["info_typed"](info_upper, ek)
    m = ek == BEARING
    keep = O[m, 0, 0].copy()
    O[m] = 0.0
    O[m, 0, 0] = keep
    return O


def edge_errors(poses, ef, et, meas, ek):
    poses = np.asarray(poses, dtype=np.float64)
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 3)
    ek = np.asarray(ek)
    e = _ORIG["edge_errors"](poses, ef, et, meas, ek)
    m = ek == BEARING
    if m.any():
        _, _, _, _, rx, ry = _rel(poses, np.asarray(ef), np.asarray(et), m)
        b = np.where(rx * rx + ry * ry > 0, np.arctan2(ry, rx), 0.0)
        e[m] = np.stack([R.normalize_theta(b - meas[m, 0]), np.zeros(m.sum()), np.zeros(m.sum())], axis=1)
    return e


def jacobians(poses, ef, et, meas, ek):
    poses = np.asarray(poses, dtype=np.float64)
    ek = np.asarray(ek)
    Ji, Jj = _ORIG["jacobians"](poses, ef, et, meas, ek)          # (kind 2: zeroed as every typed kind)
    m = ek == BEARING
    if m.any():
        c, s, dx, dy, rx, ry = _rel(poses, np.asarray(ef), np.asarray(et), m)
        q = rx * rx + ry * ry
        ok = q > 0
        qq = np.where(ok, q, 1.0)
        ua, ub = np.where(ok, -ry / qq, 0.0), np.where(ok, rx / qq, 0.0)
        Ji[m, 0, 0] = ua * -c + ub * s
        Ji[m, 0, 1] = ua * -s + ub * -c
        Ji[m, 0, 2] = np.where(ok, -1.0, 0.0)
        Jj[m, 0, 0] = ua * c + ub * -s
        Jj[m, 0, 1] = ua * s + ub * c
    return Ji, Jj


def _magnitudes(poses, ef, et, meas, ek):
    ek = np.asarray(ek)
    e, Ji, Jj = _ORIG["_magnitudes"](poses, ef, et, meas, ek)
    m = ek == BEARING
    if m.any():
        c, s, dx, dy, rx, ry = _rel(poses, ef, et, m)
        c, s, tx, ty = np.abs(c), np.abs(s), np.abs(dx), np.abs(dy)
        ax, ay = c * tx + s * ty, s * tx + c * ty               # |rx|, |ry| as the magnitudes of their terms
        q = rx * rx + ry * ry
        ok = q > 0
        qq = np.where(ok, q, 1.0)
        ua, ub = np.where(ok, ay / qq, 0.0), np.where(ok, ax / qq, 0.0)
        e[m] = np.stack([np.abs(np.arctan2(ry, rx)) + np.abs(meas[m, 0]), np.zeros(m.sum()), np.zeros(m.sum())], axis=1)
        Ji[m, 0, 0] = ua * c + ub * s
        Ji[m, 0, 1] = ua * s + ub * c
        Ji[m, 0, 2] = ua * ay + ub * ax
        Jj[m, 0, 0] = ua * c + ub * s
        Jj[m, 0, 1] = ua * s + ub * c
    return e, Ji, Jj


_MINE = dict(edge_errors=edge_errors, jacobians=jacobians, info_typed=info_typed, _magnitudes=_magnitudes)


@contextlib.contextmanager
def _bearing():
    """ref_typed's drivers see the bearing-aware per-edge functions while the block runs."""
    saved = {k: getattr(T, k) for k in _MINE}
    for k, f in _MINE.items():
        setattr(T, k, f)
    try:
        yield
    finally:
        for k, f in saved.items():
            setattr(T, k, f)


def _wrap(fn):
    @functools.wraps(fn)
    def call(*a, **kw):
        with _bearing():
            return fn(*a, **kw)
    return call


edge_chi2 = _wrap(T.edge_chi2)
chi2 = _wrap(T.chi2)
weights = _wrap(T.weights)
build_system = _wrap(T.build_system)
gn_optimize = _wrap(T.gn_optimize)
lm_optimize = _wrap(T.lm_optimize)
dl_optimize = _wrap(T.dl_optimize)
step_backward_error = _wrap(T.step_backward_error)
marginal_blocks = _wrap(T.marginal_blocks)
active_fixed, apply_step, splu_solve, Layout = T.active_fixed, T.apply_step, T.splu_solve, T.Layout


def padded_system(poses, fixed, ef, et, meas, info, vk, ek):
    """The 3-per-vertex system the device carries: a point's dummy third unknown decoupled by the sum over its observations of
    H_jj(0,0) (a kind-1 edge whose H_jj(0,0) is not positive: 1.0; a bearing: its H_jj(0,0), whatever it is), right-hand side
    0.  Returns (H csc, b, Layout with every vertex 3 wide)."""
    vk, ek = np.asarray(vk), np.asarray(ek)
    Hp, bp, lay = build_system(poses, fixed, ef, et, meas, info, np.zeros_like(vk), ek)
    Jj = jacobians(poses, ef, et, meas, ek)[1]
    O = info_typed(info, ek)
    hxx = np.einsum("ea,eab,eb->e", Jj[:, :, 0], O, Jj[:, :, 0])
    Hp = Hp.tolil()
    for v in np.flatnonzero((vk == 1) & (lay.off >= 0)):
        o = lay.off[v]
        assert Hp[o + 2, o + 2] == 0 and bp[o + 2] == 0
        d = 0.0
        for k in np.flatnonzero(np.asarray(et) == v):
            if ek[k] == 1:
                d += hxx[k] if hxx[k] > 0 else 1.0
            elif ek[k] == BEARING:
                d += hxx[k]
        Hp[o + 2, o + 2] = d
    return Hp.tocsc(), bp, lay


# ------------------------------------------------------------------ data association

def predict(poses, a, b, kind):
    """(z [3], J [dim, 3 + db]) of vertex b seen from pose a as a factor of ``kind``: 0 the relative pose (db = 3), 1 the
    point in the pose's frame, 2 its bearing (db = 2).  z is padded with zeros.  A bearing of a point on the pose: z = 0, J NaN."""
    xa, xb = np.asarray(poses[a], dtype=np.float64), np.asarray(poses[b], dtype=np.float64)
    c, s = np.cos(xa[2]), np.sin(xa[2])
    dx, dy = xb[0] - xa[0], xb[1] - xa[1]
    rx, ry = c * dx + s * dy, -s * dx + c * dy
    A = np.array([[-c, -s, ry], [s, -c, -rx], [0, 0, -1.0]])
    B = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])
    if kind == 0:
        return np.array([rx, ry, float(R.normalize_theta(xb[2] - xa[2]))]), np.hstack([A, B])
    J1 = np.hstack([A[:2], B[:2, :2]])
    if kind == 1:
        return np.array([rx, ry, 0.0]), J1
    q = rx * rx + ry * ry
    if not q > 0:
        return np.zeros(3), np.full((1, 5), np.nan)
    J = (-ry / q) * J1[0] + (rx / q) * J1[1]
    J[2] = -1.0
    return np.array([np.arctan2(ry, rx), 0.0, 0.0]), J[None, :]


def joint_cov(diag_a, cross, diag_b, db):
    """The (3 + db)-square joint covariance of (x_a, x_b) from its padded 3x3 blocks."""
    return np.block([[diag_a, cross[:, :db]], [cross[:, :db].T, diag_b[:db, :db]]])


def gate(z, S, kind, zh, info_upper=None):
    """d2 = e^T (S + Omega^-1)^-1 e of the hypothesis ``zh`` [3] (``info_upper`` [6] or None) in the factor's own dimension
    (kinds 1 and 2; S padded 3x3); NaN where that matrix is not positive definite."""
    d = 2 if kind == 1 else 1
    e = (z - np.asarray(zh, dtype=np.float64))[:d]
    if kind == BEARING:
        e = np.array([float(R.normalize_theta(e[0]))])
    M = np.array(S[:d, :d], dtype=np.float64)
    if info_upper is not None:
        u = np.asarray(info_upper, dtype=np.float64)
        M = M + np.linalg.inv(np.array([[u[0], u[1]], [u[1], u[3]]])[:d, :d])
    if not np.all(np.isfinite(M)):
        return float("nan")
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return float("nan")
    y = np.linalg.solve(L, e)
    return float(y @ y)


def observations(poses, fixed, ef, et, meas, info, vk, ek, pairs, kinds, hyp_meas=None, hyp_info=None, blocks=None):
    """(z [n, 3], S [n, 3, 3], d2 [n] or None, J norms [n], (Saa, Sab, Sbb) norms) for the (pose, vertex) ``pairs`` predicted as
    factors of ``kinds`` at ``poses``; the blocks from marginal_blocks(pairs=) unless ``blocks`` = (aa, ab, bb) [n, 3, 3] are
    given (the arithmetic alone, on someone else's blocks)."""
    pairs = [(int(a), int(b)) for a, b in pairs]
    if blocks is None:
        diag, cross, err = marginal_blocks(poses, fixed, ef, et, meas, info, vk, ek, pairs=pairs)
        assert err <= 1e-9, err
        blocks = (np.array([diag[a] for a, _ in pairs]), cross, np.array([diag[b] for _, b in pairs]))
    n = len(pairs)
    z, S, jn = np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros(n)
    d2 = None if hyp_meas is None else np.zeros(n)
    for k, (a, b) in enumerate(pairs):
        kind = int(kinds[k])
        z[k], J = predict(poses, a, b, kind)
        d = J.shape[0]
        Sg = joint_cov(blocks[0][k], blocks[1][k], blocks[2][k], J.shape[1] - 3)
        Sk = J @ Sg @ J.T
        S[k, :d, :d] = 0.5 * (Sk + Sk.T)
        jn[k] = np.linalg.norm(J)
        if d2 is not None:
            d2[k] = gate(z[k], S[k], kind, hyp_meas[k], None if hyp_info is None else hyp_info[k])
    return z, S, d2, jn, tuple(np.linalg.norm(b, axis=(1, 2)) for b in blocks)
