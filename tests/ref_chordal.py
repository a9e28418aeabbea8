"""Float64 numpy reference of chordal initialisation (include/cgmr.h: cgmr_chordal_initialize), written from
the two linear problems' formulas and not from the kernel.  TEST INFRASTRUCTURE ONLY.

Each stage builds the stacked system A x = b over the stage's free unknowns -- one square-root-information-weighted row block
per factor, fixed vertices (and vertices the stage leaves out) moved to the right-hand side as constants -- and solves it
twice: numpy.linalg.lstsq on A, and Cholesky on A^T A.  Nothing is linearised about the start: the unknowns are the absolute
(c, s) and the absolute positions, so the start enters only through what a stage holds constant.

  rotation     EDGE_SE2 (i, j)     sqrt(omega) (r_j - R(z_th) r_i) = 0,  omega = O(2,2)
               EDGE_PRIOR_SE2      sqrt(omega) (r_i - (cos z_th, sin z_th)) = 0
  translation  EDGE_SE2            W (R(z_th)^T R_i^T (t_j - t_i) - R(z_th)^T z_t) = 0,  W^T W = O[0:2, 0:2]
               EDGE_SE2_XY         W (R_i^T (l - t_i) - z) = 0
               EDGE_PRIOR_SE2      W (R(z_th)^T t_i - R(z_th)^T z_t) = 0
               EDGE_PRIOR_SE2_XY   W (t_i - z) = 0
A factor all of whose information entries for the stage are zero touches nothing; a free vertex no factor of the stage touches
is left out of it and keeps its estimate."""
import numpy as np

ROTATION, TRANSLATION = 1, 2


def _R(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s], [s, c]])


def _sqrt_info(o00, o01, o11):
    """W with W^T W = the symmetric positive semi-definite 2x2 (o00 o01; o01 o11)."""
    w, V = np.linalg.eigh(np.array([[o00, o01], [o01, o11]]))
    return np.sqrt(np.maximum(w, 0.0))[:, None] * V.T


def factors(stage, poses, ef, et, meas, info, ek=None):
    """The stage's terms: a list of (i, Ji, j or -1, Jj, c, W) meaning W (Ji x_i + Jj x_j - c), x the stage's 2-vector."""
    ek = np.zeros(len(ef), dtype=np.uint8) if ek is None else np.asarray(ek)
    out = []
    I2 = np.eye(2)
    for k in range(len(ef)):
        i, j, kind, z, u = int(ef[k]), int(et[k]), int(ek[k]), meas[k], info[k]
        if stage == ROTATION:
            if kind not in (0, 3) or u[5] == 0.0:
                continue
            W = np.sqrt(u[5]) * I2
            if kind == 0:
                out.append((i, -_R(z[2]), j, I2, np.zeros(2), W))
            else:
                out.append((i, I2, -1, None, np.array([np.cos(z[2]), np.sin(z[2])]), W))
        else:
            if kind == 2 or (u[0] == 0.0 and u[1] == 0.0 and u[3] == 0.0):
                continue
            W = _sqrt_info(u[0], u[1], u[3])
            RiT = _R(poses[i, 2]).T
            RzT = _R(z[2]).T
            if kind == 0:
                M = RzT @ RiT
                out.append((i, -M, j, M, RzT @ z[:2], W))
            elif kind == 1:
                out.append((i, -RiT, j, RiT, np.array(z[:2]), W))
            elif kind == 3:
                out.append((i, RzT, -1, None, RzT @ z[:2], W))
            else:
                out.append((i, I2, -1, None, np.array(z[:2]), W))
    return out


def stage_system(stage, poses, fixed, ef, et, meas, info, ek=None):
    """(A, b, the vertices that are unknowns of the stage in column order)."""
    fs = factors(stage, poses, ef, et, meas, info, ek)
    nV = poses.shape[0]
    touched = np.zeros(nV, dtype=bool)
    for i, _, j, _, _, _ in fs:
        touched[i] = True
        if j >= 0:
            touched[j] = True
    unknown = np.flatnonzero(touched & (np.asarray(fixed) == 0))
    col = -np.ones(nV, dtype=np.int64)
    col[unknown] = np.arange(len(unknown))
    if stage == ROTATION:
        const = np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])], axis=1)
    else:
        const = poses[:, :2]
    A = np.zeros((2 * len(fs), 2 * len(unknown)))
    b = np.zeros(2 * len(fs))
    for r, (i, Ji, j, Jj, c, W) in enumerate(fs):
        rhs = W @ c
        for v, J in ((i, Ji), (j, Jj)):
            if v < 0:
                continue
            if col[v] >= 0:
                A[2 * r:2 * r + 2, 2 * col[v]:2 * col[v] + 2] += W @ J
            else:
                rhs = rhs - W @ J @ const[v]
        b[2 * r:2 * r + 2] = rhs
    return A, b, unknown


class Singular(Exception):
    """A stage without a gauge: A has a null space."""


def solve(A, b, how):
    n = A.shape[1]
    if n == 0:
        return np.zeros(0)
    if how == "lstsq":
        x, _, rank, _ = np.linalg.lstsq(A, b, rcond=None)
        if rank < n:
            raise Singular(f"rank {rank} of {n}")
        return x
    try:
        L = np.linalg.cholesky(A.T @ A)
    except np.linalg.LinAlgError as e:
        raise Singular(str(e))
    return np.linalg.solve(L.T, np.linalg.solve(L, A.T @ b))


def initialize(poses, fixed, ef, et, meas, info, stages=3, vk=None, ek=None, how="lstsq"):
    """The stages of ``stages`` (bit 0 rotation, bit 1 translation) in that order, each solved by ``how`` ("lstsq" or
    "cholesky").  Returns dict(poses, counts [3]: unknown vertices of the rotation stage, of the translation stage, degenerate
    headings; cost: the stages' own minimal costs).  Raises Singular."""
    p = np.array(poses, dtype=np.float64, copy=True)
    counts = [0, 0, 0]
    cost = {}
    if stages & ROTATION:
        A, b, unk = stage_system(ROTATION, p, fixed, ef, et, meas, info, ek)
        x = solve(A, b, how).reshape(-1, 2)
        counts[0] = len(unk)
        n2 = (x ** 2).sum(1)
        bad = (n2 == 0.0) | ~np.isfinite(n2)
        counts[2] = int(bad.sum())
        p[unk[~bad], 2] = np.arctan2(x[~bad, 1], x[~bad, 0])
        cost[ROTATION] = float(((A @ x.ravel() - b) ** 2).sum())
    if stages & TRANSLATION:
        A, b, unk = stage_system(TRANSLATION, p, fixed, ef, et, meas, info, ek)
        x = solve(A, b, how).reshape(-1, 2)
        counts[1] = len(unk)
        p[unk, :2] = x
        cost[TRANSLATION] = float(((A @ x.ravel() - b) ** 2).sum())
    return dict(poses=p, counts=np.array(counts, dtype=np.int32), cost=cost)


def wrap(t):
    """An angle difference into (-pi, pi]."""
    return np.arctan2(np.sin(t), np.cos(t))


def differences(a, b):
    """(largest position difference, largest wrapped heading difference) of two estimates."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a[:, :2] - b[:, :2]).max()), float(np.abs(wrap(a[:, 2] - b[:, 2])).max())
