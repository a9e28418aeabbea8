"""Float64 reference of the robust-kernel contract (g2o's RobustKernel* [g2o-recalled]; include/cgmr.h, cgmr_robust).

An edge with error e and information O has e2 = e^T O e; its kernel maps e2 to (rho0, rho1).  At a fixed linearisation point
the robust system is the plain one with every edge's information scaled by rho1 (g2o's robustInformation, no second-order
term), and the robust chi2 is the sum of rho0.  So every float64 helper of ref_numpy checks a robust step given
``info * w[:, None]``, w taken at the step's start poses."""
import numpy as np
import scipy.sparse as sp

import ref_lm
import ref_numpy as R
from cg_mrslam_amd import synth

KINDS = {"none": 0, "huber": 1, "pseudohuber": 2, "cauchy": 3, "welsch": 4, "tukey": 5, "saturated": 6, "dcs": 7}


def rho(kind, delta, e2):
    """(rho0, rho1) of kernel ``kind`` (code, or per-edge codes) with ``delta`` at ``e2`` (arrays broadcast), the formulas of
    include/cgmr.h in the same order."""
    kind, delta, e2 = np.broadcast_arrays(np.atleast_1d(np.asarray(kind, dtype=np.int64)),
                                          np.atleast_1d(np.asarray(delta, dtype=np.float64)),
                                          np.atleast_1d(np.asarray(e2, dtype=np.float64)))
    r0 = e2.copy()
    r1 = np.ones_like(e2)
    d2 = delta * delta
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = (kind == 1) & (e2 > d2)
        se = np.sqrt(e2[m])
        r0[m] = 2 * se * delta[m] - d2[m]
        r1[m] = delta[m] / se
        m = kind == 2
        a = np.sqrt(e2[m] / d2[m] + 1.0)
        r0[m] = 2 * d2[m] * (a - 1.0)
        r1[m] = 1.0 / a
        m = kind == 3
        a = e2[m] / d2[m] + 1.0
        r0[m] = d2[m] * np.log(a)
        r1[m] = 1.0 / a
        m = kind == 4
        a = np.exp(-(e2[m] / d2[m]))
        r0[m] = d2[m] * (1.0 - a)
        r1[m] = a
        m = kind == 5
        inside = m & (np.sqrt(e2) <= delta)
        a = 1.0 - e2[inside] / d2[inside]
        r0[inside] = d2[inside] * (1.0 - a * a * a) / 3.0
        r1[inside] = a * a
        out = m & ~inside
        r0[out] = d2[out] / 3.0
        r1[out] = 0.0
        m = (kind == 6) & (e2 > d2)
        r0[m] = d2[m]
        r1[m] = 0.0
        m = kind == 7
        sc = 2 * delta[m] / (delta[m] + e2[m])
        low = sc < 1.0
        idx = np.flatnonzero(m)[low]
        r1[idx] = sc[low] * sc[low]
        r0[idx] = r1[idx] * e2[idx]
    return r0, r1


def edge_chi2(poses, ef, et, meas, info):
    """e^T O e of every edge."""
    e = R.edge_errors(np.asarray(poses, dtype=np.float64), ef, et, meas)
    return np.einsum("ei,eij,ej->e", e, R.info_full(np.asarray(info, dtype=np.float64)), e)


def weights(poses, ef, et, meas, info, kind, delta):
    """rho1 of every edge at ``poses``."""
    return rho(kind, delta, edge_chi2(poses, ef, et, meas, info))[1]


def robust_chi2(poses, ef, et, meas, info, kind, delta):
    """g2o's activeRobustChi2: the sum of rho0 over the edges."""
    return float(np.sum(rho(kind, delta, edge_chi2(poses, ef, et, meas, info))[0]))


def scaled_info(poses, ef, et, meas, info, kind, delta):
    """The information of the robust system at ``poses``: info * rho1."""
    return np.asarray(info, dtype=np.float64) * weights(poses, ef, et, meas, info, kind, delta)[:, None]


def gn_optimize(poses, fixed, ef, et, meas, info, kind, delta, iters):
    """Robust Gauss-Newton through ref_numpy.build_system with scaled information.  Returns (poses, robust chi2 [iters+1],
    the poses every iteration started from).  Stops (poses as they stand) when a factorisation fails, returning the
    iteration it failed in as the fourth value (None otherwise)."""
    x = np.array(poses, dtype=np.float64, copy=True)
    fx = R.active_fixed(len(x), fixed, ef, et)
    chis, starts = [robust_chi2(x, ef, et, meas, info, kind, delta)], []
    for it in range(iters):
        starts.append(x.copy())
        H, b, hidx = R.build_system(x, fx, ef, et, meas, scaled_info(x, ef, et, meas, info, kind, delta))
        dx = ref_lm.cholesky_solve(H, b)
        if dx is None:
            return x, np.array(chis), starts, it
        x = ref_lm.apply_step(x, hidx, dx)
        chis.append(robust_chi2(x, ef, et, meas, info, kind, delta))
    return x, np.array(chis), starts, None


def lm_optimize(poses, fixed, ef, et, meas, info, kind, delta, iters, **params):
    """ref_lm.lm_optimize's contract (g2o's OptimizationAlgorithmLevenberg) on the robust chi2 and the robust system (information
    scaled by rho1 at the iteration's start).  Returns the same dict as ref_lm.lm_optimize (trace without systems)."""
    P = dict(ref_lm.DEFAULTS, **params)
    x = np.array(poses, dtype=np.float64, copy=True)
    fx = R.active_fixed(len(x), fixed, ef, et)
    chi = lambda p: robust_chi2(p, ef, et, meas, info, kind, delta)   # noqa: E731
    lam, nu = 0.0, 2.0
    cur = chi(x)
    chis, lams, trials, trace = [cur], [], [], []
    terminated = False
    for i in range(iters):
        cur = chi(x)
        H, b, hidx = R.build_system(x, fx, ef, et, meas, scaled_info(x, ef, et, meas, info, kind, delta))
        n = H.shape[0]
        if i == 0:
            lam = float(P["initial_lambda"]) if P["initial_lambda"] > 0 else \
                float(P["tau"]) * (float(np.max(np.abs(H.diagonal()))) if n else 0.0)
            nu = 2.0
        q = 0
        while True:
            dx = ref_lm.cholesky_solve(H + lam * sp.identity(n, format="csc"), b)
            failed = dx is None
            if failed:
                temp, rho_ = ref_lm.DBL_MAX, -np.inf
            else:
                x1 = ref_lm.apply_step(x, hidx, dx)
                temp = chi(x1)
                rho_ = (cur - temp) / (float(np.dot(dx, lam * dx + b)) + 1e-3)
            accept = bool(rho_ > 0 and np.isfinite(temp))
            brk = False
            rec = dict(iteration=i, trial=q, **{"lambda": lam}, failed=failed, current=cur, temp=temp, rho=rho_, accept=accept,
                       x0=x.copy())
            if accept:
                lam *= max(P["good_step_lower"], min(1.0 - (2 * rho_ - 1) ** 3, P["good_step_upper"]))
                nu = 2.0
                cur = temp
                x = x1
            else:
                lam *= nu
                nu *= 2.0
                brk = not np.isfinite(lam)
            rec["lambda_after"] = lam
            trace.append(rec)
            q += 1
            if brk or not (rho_ < 0 and q < P["max_trials"]):
                break
        lams.append(lam)
        trials.append(q)
        chis.append(cur)
        if q >= P["max_trials"] or rho_ == 0 or not np.isfinite(lam):
            terminated = True
            break
    chis = chis + [chis[-1]] * (iters + 1 - len(chis))
    return dict(poses=x, chi2=np.array(chis), lambdas=np.array(lams), trials=np.array(trials, dtype=np.int64),
                iters_done=len(lams), terminated=terminated, trace=trace)


# ------------------------------------------------------------------------------------------------ the outlier recipe
def outlier_graph(nV=2000, nE=8000, seed=7, frac=100, rng_seed=1):
    """synth.make_pose_graph(nV, nE, seed) with n_lc // frac of its loop closures corrupted: +-U(3, 10) m on x and y, theta
    replaced by U(-pi, pi).  Returns (graph, corrupted edge indices, closure mask)."""
    g = synth.make_pose_graph(nV, nE, seed=seed)
    ef = g["edge_from"]
    closure = np.arange(len(ef)) >= nV - 1                  # (the odometry chain comes first)
    lc = np.flatnonzero(closure)
    rng = np.random.default_rng(rng_seed)
    bad = np.sort(rng.choice(lc, len(lc) // frac, replace=False))
    meas = g["meas"].copy()
    sgn = rng.choice([-1.0, 1.0], size=(len(bad), 2))
    meas[bad, :2] += sgn * rng.uniform(3, 10, size=(len(bad), 2))
    meas[bad, 2] = rng.uniform(-np.pi, np.pi, size=len(bad))
    g = dict(g, meas=meas)
    return g, bad, closure


def clean_optimum(g, bad, iters=15):
    """Plain Gauss-Newton on the graph without the corrupted edges."""
    keep = np.ones(len(g["edge_from"]), dtype=bool)
    keep[bad] = False
    p, _ = R.gn_optimize(g["poses"], g["fixed"], g["edge_from"][keep], g["edge_to"][keep], g["meas"][keep], g["info"][keep], iters)
    return p


def rms(a, b):
    return float(np.sqrt(np.mean(np.sum((np.asarray(a)[:, :2] - np.asarray(b)[:, :2]) ** 2, axis=1))))
