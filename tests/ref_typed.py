"""Float64 numpy reference of the typed factors (include/cgmr.h: cgmr_factor_types): SE2 poses and points, EDGE_SE2,
EDGE_SE2_XY, EDGE_PRIOR_SE2 and EDGE_PRIOR_SE2_XY.  TEST INFRASTRUCTURE ONLY.

The system is built with the TRUE dimensions: three unknowns per free pose, two per free point, no dummy.  It is solved
with SuperLU as ref_numpy does and stepped with g2o's rules (x, y += dx in the world frame, theta = normalize(theta + dtheta)).
Levenberg-Marquardt and dogleg are the policies of ref_lm.py / ref_dogleg.py run on this system (their module-level
``R`` and ``apply_step`` are swapped for the typed ones for the duration of the call); the marginals are
ref_numpy.marginal_blocks_ref's refined solves, widened to blocks of unequal size.

Factor definitions (pose i = (t_i, theta_i), point l, R the 2x2 rotation):
  kind 0  EDGE_SE2            as ref_numpy
  kind 1  EDGE_SE2_XY         e = R(theta_i)^T (l - t_i) - z
  kind 3  EDGE_PRIOR_SE2      e = (R(z_theta)^T (t_i - z_t), normalize(theta_i - z_theta)),  from == to
  kind 4  EDGE_PRIOR_SE2_XY   e = t_i - z,                                                    from == to
A 2-dimensional factor uses meas[:2] and the entries (0,0) (0,1) (1,1) of its information."""
from __future__ import annotations

import contextlib
import types

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import ref_numpy as R
import ref_robust

U = R.U
POSE, POINT = 0, 1
SE2, SE2_XY, PRIOR_SE2, PRIOR_XY = 0, 1, 3, 4


def _kinds(poses, ef, vk, ek):
    vk = np.zeros(len(poses), np.uint8) if vk is None else np.asarray(vk, dtype=np.uint8)
    ek = np.zeros(len(ef), np.uint8) if ek is None else np.asarray(ek, dtype=np.uint8)
    return vk, ek


def info_typed(info_upper, ek):
    """Omega [E, 3, 3]; a 2-dimensional factor keeps its top-left 2x2."""
    O = R.info_full(np.asarray(info_upper, dtype=np.float64).reshape(-1, 6))
    two = (ek == SE2_XY) | (ek == PRIOR_XY)
    O[two, 2, :] = 0.0
    O[two, :, 2] = 0.0
    return O


def edge_errors(poses, ef, et, meas, ek):
    """e [E, 3]; the third component of a 2-dimensional factor is 0."""
    poses = np.asarray(poses, dtype=np.float64)
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 3)
    e = R.edge_errors(poses, ef, et, meas) if len(ef) else np.zeros((0, 3))
    xi, xj = poses[ef], poses[et]
    m = ek == SE2_XY
    c, s = np.cos(xi[m, 2]), np.sin(xi[m, 2])
    dx, dy = xj[m, 0] - xi[m, 0], xj[m, 1] - xi[m, 1]
    e[m] = np.stack([c * dx + s * dy - meas[m, 0], -s * dx + c * dy - meas[m, 1], np.zeros(m.sum())], axis=1)
    m = ek == PRIOR_SE2
    cz, sz = np.cos(meas[m, 2]), np.sin(meas[m, 2])
    px, py = xi[m, 0] - meas[m, 0], xi[m, 1] - meas[m, 1]
    e[m] = np.stack([cz * px + sz * py, -sz * px + cz * py, R.normalize_theta(xi[m, 2] - meas[m, 2])], axis=1)
    m = ek == PRIOR_XY
    e[m] = np.stack([xi[m, 0] - meas[m, 0], xi[m, 1] - meas[m, 1], np.zeros(m.sum())], axis=1)
    return e


def jacobians(poses, ef, et, meas, ek):
    """(Ji, Jj) [E, 3, 3] with respect to the (x, y, theta) / (x, y, -) increments of the two ends; unused rows and columns are
    zero.  A prior is carried by Ji alone."""
    poses = np.asarray(poses, dtype=np.float64)
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 3)
    Ji, Jj = R.jacobians(poses, ef, et, meas) if len(ef) else (np.zeros((0, 3, 3)), np.zeros((0, 3, 3)))
    xi, xj = poses[ef], poses[et]
    typed = ek != SE2
    Ji[typed] = 0.0
    Jj[typed] = 0.0
    m = ek == SE2_XY
    c, s = np.cos(xi[m, 2]), np.sin(xi[m, 2])
    dx, dy = xj[m, 0] - xi[m, 0], xj[m, 1] - xi[m, 1]
    Ji[m, 0, 0] = -c; Ji[m, 0, 1] = -s; Ji[m, 0, 2] = -s * dx + c * dy
    Ji[m, 1, 0] = s; Ji[m, 1, 1] = -c; Ji[m, 1, 2] = -c * dx - s * dy
    Jj[m, 0, 0] = c; Jj[m, 0, 1] = s
    Jj[m, 1, 0] = -s; Jj[m, 1, 1] = c
    m = ek == PRIOR_SE2
    cz, sz = np.cos(meas[m, 2]), np.sin(meas[m, 2])
    Ji[m, 0, 0] = cz; Ji[m, 0, 1] = sz
    Ji[m, 1, 0] = -sz; Ji[m, 1, 1] = cz
    Ji[m, 2, 2] = 1.0
    m = ek == PRIOR_XY
    Ji[m, 0, 0] = 1.0
    Ji[m, 1, 1] = 1.0
    return Ji, Jj


def edge_chi2(poses, ef, et, meas, info, ek):
    e = edge_errors(poses, ef, et, meas, ek)
    return np.einsum("ei,eij,ej->e", e, info_typed(info, ek), e)


def chi2(poses, ef, et, meas, info, ek, kind=None, delta=None):
    """The plain chi2, or with a robust kernel the sum of rho0."""
    e2 = edge_chi2(poses, ef, et, meas, info, ek)
    return float(np.sum(e2 if kind is None else ref_robust.rho(kind, delta, e2)[0]))


def weights(poses, ef, et, meas, info, ek, kind, delta):
    return ref_robust.rho(kind, delta, edge_chi2(poses, ef, et, meas, info, ek))[1]


def active_fixed(nV, fixed, ef, et):
    return R.active_fixed(nV, fixed, ef, et)


class Layout:
    """Where every free vertex lies in the true-dimension system: off[v] (-1: not in it), dim[v] (3 or 2), n."""

    def __init__(self, fixed, vk):
        self.dim = np.where(np.asarray(vk) == POINT, 2, 3).astype(np.int64)
        free = np.asarray(fixed) == 0
        self.off = -np.ones(len(self.dim), dtype=np.int64)
        sizes = np.where(free, self.dim, 0)
        self.off[free] = (np.cumsum(sizes) - sizes)[free]
        self.n = int(sizes.sum())


def _scatter(blocks, lay, rv, cv, mask):
    """COO triplets of the 3x3 ``blocks`` of the (row vertex, column vertex) pairs, cut to the vertices' dimensions."""
    rows, cols, vals = [], [], []
    for k in np.flatnonzero(mask):
        r, c = rv[k], cv[k]
        dr, dc = lay.dim[r], lay.dim[c]
        rr, cc = np.meshgrid(lay.off[r] + np.arange(dr), lay.off[c] + np.arange(dc), indexing="ij")
        rows.append(rr.ravel())
        cols.append(cc.ravel())
        vals.append(blocks[k, :dr, :dc].ravel())
    if not rows:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def _assemble(Ji, Jj, O, e, lay, ef, et):
    """(H csc, b) from per-edge Jacobians, information and errors (also used with magnitudes)."""
    JiO = np.transpose(Ji, (0, 2, 1)) @ O
    JjO = np.transpose(Jj, (0, 2, 1)) @ O
    Hii, Hij, Hjj = JiO @ Ji, JiO @ Jj, JjO @ Jj
    bi = (JiO @ e[:, :, None])[:, :, 0]
    bj = (JjO @ e[:, :, None])[:, :, 0]
    ef, et = np.asarray(ef), np.asarray(et)
    mi, mj = lay.off[ef] >= 0, lay.off[et] >= 0
    unary = ef == et                                            # (carried by Ji alone: Jj, and with it Hij and Hjj, is zero)
    both = mi & mj & ~unary
    parts = [_scatter(Hii, lay, ef, ef, mi), _scatter(Hjj, lay, et, et, mj & ~unary), _scatter(Hij, lay, ef, et, both),
             _scatter(np.transpose(Hij, (0, 2, 1)), lay, et, ef, both)]
    rows, cols, vals = (np.concatenate([p[q] for p in parts]) for q in range(3))
    H = sp.coo_matrix((vals, (rows, cols)), shape=(lay.n, lay.n)).tocsc()
    b = np.zeros(lay.n)
    for k in np.flatnonzero(mi):
        v = ef[k]
        b[lay.off[v]:lay.off[v] + lay.dim[v]] += bi[k, :lay.dim[v]]
    for k in np.flatnonzero(mj & ~unary):
        v = et[k]
        b[lay.off[v]:lay.off[v] + lay.dim[v]] += bj[k, :lay.dim[v]]
    return H, b


def build_system(poses, fixed, ef, et, meas, info, vk=None, ek=None, kind=None, delta=None):
    """(H csc over the free scalars -- 3 per pose, 2 per point --, b = -J^T Omega e, the Layout).  ``fixed`` as given (use
    active_fixed to drop the vertices no edge touches).  kind / delta: a robust kernel, Omega scaled by rho1."""
    poses = np.asarray(poses, dtype=np.float64)
    vk, ek = _kinds(poses, ef, vk, ek)
    lay = Layout(fixed, vk)
    e = edge_errors(poses, ef, et, meas, ek)
    Ji, Jj = jacobians(poses, ef, et, meas, ek)
    O = info_typed(info, ek)
    if kind is not None:
        O = O * ref_robust.rho(kind, delta, np.einsum("ei,eij,ej->e", e, O, e))[1][:, None, None]
    H, b = _assemble(Ji, Jj, O, e, lay, ef, et)
    return H, -b, lay


def apply_step(poses, lay, dx):
    x = np.array(poses, dtype=np.float64, copy=True)
    for v in np.flatnonzero(lay.off >= 0):
        d = dx[lay.off[v]:lay.off[v] + lay.dim[v]]
        x[v, 0] += d[0]
        x[v, 1] += d[1]
        if lay.dim[v] == 3:
            x[v, 2] = R.normalize_theta(x[v, 2] + d[2])
    return x


def splu_solve(H, b):
    return spla.splu(sp.csc_matrix(H), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True)).solve(b)


def gn_optimize(poses, fixed, ef, et, meas, info, iters, vk=None, ek=None, kind=None, delta=None, solve=splu_solve):
    """(poses, chi2 [iters + 1], the poses every iteration started from)."""
    x = np.array(poses, dtype=np.float64, copy=True)
    vk, ek = _kinds(x, ef, vk, ek)
    fx = active_fixed(len(x), fixed, ef, et)
    chis, starts = [chi2(x, ef, et, meas, info, ek, kind, delta)], []
    for _ in range(iters):
        starts.append(x.copy())
        H, b, lay = build_system(x, fx, ef, et, meas, info, vk, ek, kind, delta)
        x = apply_step(x, lay, solve(H, b))
        chis.append(chi2(x, ef, et, meas, info, ek, kind, delta))
    return x, np.array(chis), starts


# ------------------------------------------------------------------ Levenberg-Marquardt and dogleg: the policies of ref_lm / ref_dogleg

@contextlib.contextmanager
def _typed_modules(vk, ek, kind, delta):
    """ref_lm / ref_dogleg see this module's system (their ``R``) and step (``apply_step``) while the block runs."""
    import ref_dogleg
    import ref_lm

    def _chi2(p, ef, et, meas, info):
        return chi2(p, ef, et, meas, info, ek, kind, delta)

    def _build(p, fx, ef, et, meas, info):
        return build_system(p, fx, ef, et, meas, info, vk, ek, kind, delta)

    shim = types.SimpleNamespace(active_fixed=active_fixed, chi2=_chi2, build_system=_build, normalize_theta=R.normalize_theta)
    saved = (ref_lm.R, ref_lm.apply_step, ref_dogleg.R)
    ref_lm.R, ref_lm.apply_step, ref_dogleg.R = shim, apply_step, shim
    try:
        yield ref_lm, ref_dogleg
    finally:
        ref_lm.R, ref_lm.apply_step, ref_dogleg.R = saved


def lm_optimize(poses, fixed, ef, et, meas, info, iters, vk=None, ek=None, kind=None, delta=None, **params):
    """ref_lm.lm_optimize's result on the typed system (robust: the robust chi2 and the scaled information)."""
    vk, ek = _kinds(np.asarray(poses), ef, vk, ek)
    with _typed_modules(vk, ek, kind, delta) as (ref_lm, _):
        return ref_lm.lm_optimize(poses, fixed, ef, et, meas, info, iters, **params)


def dl_optimize(poses, fixed, ef, et, meas, info, iters, vk=None, ek=None, kind=None, delta=None, **params):
    """ref_dogleg.dl_optimize's result on the typed system (the robust kernel enters through the shim, not ref_dogleg's own)."""
    vk, ek = _kinds(np.asarray(poses), ef, vk, ek)
    with _typed_modules(vk, ek, kind, delta) as (_, ref_dogleg):
        return ref_dogleg.dl_optimize(poses, fixed, ef, et, meas, info, iters, **params)


# ------------------------------------------------------------------ backward error (ref_numpy.step_backward_error's definition)

def _magnitudes(poses, ef, et, meas, ek):
    """|e|, |Ji|, |Jj| as the magnitudes of the terms they are computed from (ref_numpy._edge_magnitudes, with the typed
    factors' own terms)."""
    e, Ji, Jj = R._edge_magnitudes(poses, ef, et, meas) if len(ef) else (np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3, 3)))
    self0 = (ek == SE2) & (np.asarray(ef) == np.asarray(et))
    Ji[self0] += Jj[self0]
    Jj[self0] = 0
    xi, xj = poses[ef], poses[et]
    typed = ek != SE2
    Ji[typed] = 0.0
    Jj[typed] = 0.0
    m = ek == SE2_XY
    c, s = np.abs(np.cos(xi[m, 2])), np.abs(np.sin(xi[m, 2]))
    tx, ty = np.abs(xj[m, 0] - xi[m, 0]), np.abs(xj[m, 1] - xi[m, 1])
    e[m] = np.stack([c * tx + s * ty + np.abs(meas[m, 0]), s * tx + c * ty + np.abs(meas[m, 1]), np.zeros(m.sum())], axis=1)
    Ji[m, 0, 0] = c; Ji[m, 0, 1] = s; Ji[m, 0, 2] = s * tx + c * ty
    Ji[m, 1, 0] = s; Ji[m, 1, 1] = c; Ji[m, 1, 2] = c * tx + s * ty
    Jj[m, 0, 0] = c; Jj[m, 0, 1] = s
    Jj[m, 1, 0] = s; Jj[m, 1, 1] = c
    m = ek == PRIOR_SE2
    cz, sz = np.abs(np.cos(meas[m, 2])), np.abs(np.sin(meas[m, 2]))
    px, py = np.abs(xi[m, 0] - meas[m, 0]), np.abs(xi[m, 1] - meas[m, 1])
    e[m] = np.stack([cz * px + sz * py, sz * px + cz * py, np.abs(xi[m, 2] - meas[m, 2])], axis=1)
    Ji[m, 0, 0] = cz; Ji[m, 0, 1] = sz
    Ji[m, 1, 0] = sz; Ji[m, 1, 1] = cz
    Ji[m, 2, 2] = 1.0
    m = ek == PRIOR_XY
    e[m] = np.stack([np.abs(xi[m, 0] - meas[m, 0]), np.abs(xi[m, 1] - meas[m, 1]), np.zeros(m.sum())], axis=1)
    Ji[m, 0, 0] = 1.0
    Ji[m, 1, 1] = 1.0
    return e, Ji, Jj


def step_vector(poses0, poses1, lay, ref=None):
    """dx of the step poses0 -> poses1 in the layout's order; the heading's branch of 2 pi from the reference solve."""
    dx = np.zeros(lay.n)
    for v in np.flatnonzero(lay.off >= 0):
        o, d = lay.off[v], lay.dim[v]
        dx[o:o + 2] = poses1[v, :2] - poses0[v, :2]
        if d == 3:
            t = float(R.normalize_theta(poses1[v, 2] - poses0[v, 2]))
            if ref is not None:
                t += 2 * np.pi * np.round((ref[o + 2] - t) / (2 * np.pi))
            dx[o + 2] = t
    return dx


def step_backward_error(poses0, poses1, fixed, ef, et, meas, info, vk=None, ek=None, kind=None, delta=None):
    """ref_numpy.step_backward_error's omega for the step poses0 -> poses1 of the typed system assembled at poses0:

        omega = max_i max(|H dx - b|_i - (H_abs s)_i, 0) / (H_abs |dx| + b_abs)_i,   s = u (|poses0| + |poses1|) (+ 2 pi u, headings)

    with the residual in long double and H_abs, b_abs the absolute-value assembly of the typed terms."""
    poses0 = np.asarray(poses0, dtype=np.float64)
    poses1 = np.asarray(poses1, dtype=np.float64)
    vk, ek = _kinds(poses0, ef, vk, ek)
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 3)
    fx = active_fixed(len(poses0), fixed, ef, et)
    H, b, lay = build_system(poses0, fx, ef, et, meas, info, vk, ek, kind, delta)
    if lay.n == 0:
        return 0.0
    dx = step_vector(poses0, poses1, lay, splu_solve(H, b))
    Hc = sp.coo_matrix(H)
    r = -np.asarray(b, dtype=np.longdouble).copy()
    np.add.at(r, Hc.row, Hc.data.astype(np.longdouble) * dx[Hc.col].astype(np.longdouble))
    e_abs, Ji_abs, Jj_abs = _magnitudes(poses0, np.asarray(ef), np.asarray(et), meas, ek)
    O = info_typed(info, ek)
    if kind is not None:
        e = edge_errors(poses0, ef, et, meas, ek)
        O = O * ref_robust.rho(kind, delta, np.einsum("ei,eij,ej->e", e, O, e))[1][:, None, None]
    H_abs, b_abs = _assemble(Ji_abs, Jj_abs, np.abs(O), e_abs, lay, ef, et)
    den = H_abs @ np.abs(dx) + b_abs
    slack = np.zeros(lay.n)
    for v in np.flatnonzero(lay.off >= 0):
        o, d = lay.off[v], lay.dim[v]
        slack[o:o + d] = U * (np.abs(poses0[v, :d]) + np.abs(poses1[v, :d]))
        if d == 3:
            slack[o + 2] += 2 * np.pi * U
    res = np.maximum(np.abs(r).astype(np.float64) - H_abs @ slack, 0.0)
    ok = den > 0
    if np.any(res[~ok] != 0):
        return float("inf")
    return float(np.max(res[ok] / den[ok])) if ok.any() else 0.0


# ------------------------------------------------------------------ marginals

def marginal_blocks(poses, fixed, ef, et, meas, info, vk=None, ek=None, pairs=None, kind=None, delta=None):
    """Blocks of H^-1 of the true-dimension system at ``poses``, padded to 3x3 with zeros (a point's third row / column),
    by ref_numpy's refined solves.  Returns (diag [nV, 3, 3], cross [len(pairs), 3, 3] -- rows: pairs[k][0], columns:
    pairs[k][1] --, the largest relative last correction of a block: the reference's own error estimate).  Fixed and
    inactive vertices give zeros."""
    poses = np.asarray(poses, dtype=np.float64)
    vk, ek = _kinds(poses, ef, vk, ek)
    fx = active_fixed(len(poses), fixed, ef, et)
    H, _, lay = build_system(poses, fx, ef, et, meas, info, vk, ek, kind, delta)
    nV = len(poses)
    diag = np.zeros((nV, 3, 3))
    pairs = [] if pairs is None else [(int(a), int(b)) for a, b in pairs]
    cross = np.zeros((len(pairs), 3, 3))
    if lay.n == 0:
        return diag, cross, 0.0
    lu = spla.splu(H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    X, D = R._refine_solve(H, lu, np.eye(lay.n))                 # (the cases are small: every column)
    err = 0.0
    for v in np.flatnonzero(lay.off >= 0):
        o, d = lay.off[v], lay.dim[v]
        diag[v, :d, :d] = X[o:o + d, o:o + d]
        err = max(err, np.linalg.norm(D[o:o + d, o:o + d]) / np.linalg.norm(X[o:o + d, o:o + d]))
    for k, (a, b) in enumerate(pairs):
        if lay.off[a] >= 0 and lay.off[b] >= 0:
            oa, da, ob, db = lay.off[a], lay.dim[a], lay.off[b], lay.dim[b]
            cross[k, :da, :db] = X[oa:oa + da, ob:ob + db]
    return diag, cross, float(err)
