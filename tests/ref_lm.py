"""Float64 reference of the Levenberg-Marquardt contract (g2o's OptimizationAlgorithmLevenberg::solve inside
SparseOptimizer::optimize [g2o-recalled]; include/cgmr.h, cgmr_lm_optimize), on ref_numpy.build_system.

optimize(n) runs outer iterations i = 0 .. n-1 and stops early on termination:
  1. currentChi = chi2(x); H, b = build_system(x) with b = -J^T Omega e; fixed and inactive vertices stay out of the system.
  2. i == 0: lambda = initial_lambda if > 0, else tau * max |H_jj|; nu = 2.
  3. trials q = 0, 1, ...: solve (H + lambda I) dx = b by a Cholesky factorisation; x' = x (+) dx (angle wrapped);
     tempChi = chi2(x'), or DBL_MAX when the factorisation fails; rho = (currentChi - tempChi) / (dx^T (lambda dx + b) + 1e-3),
     -inf when it fails (the step is garbage then, whatever the scale).  rho > 0 and tempChi finite: accept, lambda *=
     max(lower, min(upper, 1 - (2 rho - 1)^3)), nu = 2, currentChi = tempChi.  Otherwise restore x, lambda *= nu, nu *= 2,
     and leave the loop if lambda is no longer finite.  Repeat while rho < 0 and q + 1 < max_trials.
  4. Terminate if the iteration ran max_trials trials, or rho == 0, or lambda is not finite.
The trial count of an iteration counts every factorisation (g2o's levenbergIteration, except that a trial that leaves the
loop on an infinite lambda counts as well; termination is the same either way)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import ref_numpy as R

DBL_MAX = np.finfo(np.float64).max
DEFAULTS = dict(tau=1e-5, initial_lambda=-1.0, max_trials=10, good_step_lower=1.0 / 3, good_step_upper=2.0 / 3)


def cholesky_solve(A, b):
    """dx of A dx = b by a symmetric factorisation without pivoting (SuperLU in symmetric mode with diagonal pivots), or
    None when A is not positive definite: a pivot that is not positive, an exactly singular matrix, or a row exchange."""
    n = A.shape[0]
    if n == 0:
        return np.zeros(0)
    try:
        lu = spla.splu(sp.csc_matrix(A), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    except RuntimeError:
        return None
    if not np.array_equal(lu.perm_r, lu.perm_c):
        return None
    if not np.all(lu.U.diagonal() > 0):
        return None
    x = lu.solve(np.asarray(b, dtype=np.float64))
    return x if np.all(np.isfinite(x)) else None


def apply_step(poses, hidx, dx):
    x = np.array(poses, dtype=np.float64, copy=True)
    free = hidx >= 0
    d = dx.reshape(-1, 3)
    x[free, 0] += d[:, 0]
    x[free, 1] += d[:, 1]
    x[free, 2] = R.normalize_theta(x[free, 2] + d[:, 2])
    return x


def lm_optimize(poses, fixed, ef, et, meas, info, iters, keep_systems=False, **params):
    """Returns dict(poses, chi2 [iters+1] (the last value repeated past the iterations run), lambdas / trials [iters_done],
    iters_done, terminated, trace): trace holds one dict per trial (iteration, trial, lambda (the damping it used),
    failed, current, temp, rho, accept, lambda_after); with keep_systems each trial also keeps (H, b, hidx) of its
    iteration and the poses it started from."""
    P = dict(DEFAULTS, **params)
    x = np.array(poses, dtype=np.float64, copy=True)
    ef = np.asarray(ef)
    et = np.asarray(et)
    fx = R.active_fixed(len(x), fixed, ef, et)
    lam, nu = 0.0, 2.0
    cur = R.chi2(x, ef, et, meas, info)
    chis, lams, trials, trace = [cur], [], [], []
    terminated = False
    for i in range(iters):
        cur = R.chi2(x, ef, et, meas, info)
        H, b, hidx = R.build_system(x, fx, ef, et, meas, info)
        n = H.shape[0]
        if i == 0:
            if P["initial_lambda"] > 0:
                lam = float(P["initial_lambda"])
            else:
                lam = float(P["tau"]) * (float(np.max(np.abs(H.diagonal()))) if n else 0.0)
            nu = 2.0
        q = 0
        while True:
            dx = cholesky_solve(H + lam * sp.identity(n, format="csc"), b)
            failed = dx is None
            if failed:
                temp, rho = DBL_MAX, -np.inf
            else:
                x1 = apply_step(x, hidx, dx)
                temp = R.chi2(x1, ef, et, meas, info)
                scale = float(np.dot(dx, lam * dx + b)) + 1e-3
                rho = (cur - temp) / scale
            rec = dict(iteration=i, trial=q, **{"lambda": lam}, failed=failed, current=cur, temp=temp, rho=rho)
            if keep_systems:
                rec.update(H=H, b=b, hidx=hidx, x0=x.copy())
            accept = bool(rho > 0 and np.isfinite(temp))
            brk = False
            if accept:
                alpha = 1.0 - (2 * rho - 1) ** 3
                alpha = min(alpha, P["good_step_upper"])
                lam *= max(P["good_step_lower"], alpha)
                nu = 2.0
                cur = temp
                x = x1
            else:
                lam *= nu
                nu *= 2.0
                brk = not np.isfinite(lam)
            rec.update(accept=accept, lambda_after=lam)
            trace.append(rec)
            q += 1
            if brk or not (rho < 0 and q < P["max_trials"]):
                break
        lams.append(lam)
        trials.append(q)
        chis.append(cur)
        if q >= P["max_trials"] or rho == 0 or not np.isfinite(lam):
            terminated = True
            break
    done = len(lams)
    chis = chis + [chis[-1]] * (iters + 1 - len(chis))
    return dict(poses=x, chi2=np.array(chis), lambdas=np.array(lams), trials=np.array(trials, dtype=np.int64), iters_done=done,
                terminated=terminated, trace=trace)
