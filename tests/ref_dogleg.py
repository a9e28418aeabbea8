"""Float64 reference of the dogleg contract (g2o's OptimizationAlgorithmDogleg::solve inside SparseOptimizer::optimize
[g2o-recalled]: recalled from g2o, not read from its source; include/cgmr.h, cgmr_dl_optimize), on ref_numpy.build_system.

At the start of a call: delta = initial_delta, currentLambda = initial_lambda, wasPD = true.  optimize(n) runs outer
iterations i = 0 .. n-1 and stops early on Terminate or Fail:
  1. currentChi = (robust) chi2(x); H, b = build_system(x) with b = -J^T Omega e; fixed and inactive vertices stay out.
  2. alpha = |b|^2 / (b^T H b), hsd = alpha b (H undamped).
  3. First trial only: the Gauss-Newton step.  Loop: if not wasPD, factorise H + currentLambda I, else H; wasPD &= ok;
     if not wasPD: ok -> currentLambda = max(1e-12, currentLambda / (0.5 lambda_factor)); failed -> currentLambda *=
     lambda_factor, and above 1e3 it is set to 1e3 and the call fails (g2o's Fail).  Repeat until ok.  hgn = the solution.
  4. |hgn| < delta: h = hgn (GN); else |hsd| > delta: h = delta / |hsd| hsd (SD); else h = hsd + beta (hgn - hsd) (DL),
     beta from g2o's two branches on c = hsd^T (hgn - hsd), so that |h| = delta.
  5. linearGain = -h^T H h + 2 b^T h (H undamped), 1e-12 if its magnitude is below 1e-12.
  6. x' = x (+) h; rho = (currentChi - chi2(x')) / linearGain; rho > 0 keeps x', otherwise x is restored.
  7. rho > 0.75: delta = max(delta, 3 |h|); rho < 0.25: delta *= 0.5.
  8. Repeat from 4 while the step is not good and numTries < max_trials.
  9. Terminate when numTries == max_trials (an accepted step on the last try included) or no step was good; the
     terminating iteration counts as run.
Edge cases, as the C++ evaluates them: nothing free (an empty system: alpha = 0/0, hsd empty, |hsd| = 0, hgn empty) and a
graph at its optimum (b = 0: alpha = 0/0 = NaN, hgn = 0) both take GN steps of length 0 with rho = 0 until max_trials:
one iteration, delta halved max_trials times, Terminate.  iters == 0 runs nothing."""
import numpy as np
import scipy.sparse as sp

import ref_lm
import ref_numpy as R
import ref_robust

DEFAULTS = dict(initial_delta=1e4, max_trials=100, initial_lambda=1e-7, lambda_factor=10.0)
STEP_SD, STEP_GN, STEP_DL = 1, 2, 3          # g2o's STEP_* order (include/cgmr.h: CGMR_DL_STEP_*)


def dl_optimize(poses, fixed, ef, et, meas, info, iters, kind=None, delta=None, **params):
    """Returns dict(poses, chi2 [iters+1] (the last value repeated past the iterations run), deltas / trials / steps
    [iters_done] (delta after the iteration, its trials, the kind of its last step), iters_done, terminated, failed (the
    iteration g2o's Fail came in, or None), lambdas (currentLambda after every factorisation: the damping trace), trace).
    trace holds one dict per trial: iteration, trial, step, delta (before), delta_after, hgn_norm, hsd_norm, h_norm, alpha,
    current, temp, lin_gain, rho, accept.  kind / delta: a robust kernel (ref_robust) for every edge."""
    P = dict(DEFAULTS, **params)
    x = np.array(poses, dtype=np.float64, copy=True)
    ef = np.asarray(ef)
    et = np.asarray(et)
    fx = R.active_fixed(len(x), fixed, ef, et)
    robust = kind is not None

    def chi(p):
        return ref_robust.robust_chi2(p, ef, et, meas, info, kind, delta) if robust else R.chi2(p, ef, et, meas, info)

    dlt, lam, was_pd = float(P["initial_delta"]), float(P["initial_lambda"]), True
    chis, deltas, trials, steps, lams, trace = [chi(x)], [], [], [], [], []
    terminated, failed = False, None
    for i in range(iters):
        cur = chi(x)
        inf_i = ref_robust.scaled_info(x, ef, et, meas, info, kind, delta) if robust else info
        H, b, hidx = R.build_system(x, fx, ef, et, meas, inf_i)
        n = H.shape[0]
        with np.errstate(invalid="ignore", divide="ignore"):       # (b = 0: alpha = 0/0)
            alpha = np.float64(np.dot(b, b)) / np.float64(np.dot(b, H @ b))
            hsd = alpha * b
        hsd_norm = float(np.linalg.norm(hsd))
        while True:
            A = H if was_pd else H + lam * sp.identity(n, format="csc")
            hgn = ref_lm.cholesky_solve(A, b)
            ok = hgn is not None
            was_pd = was_pd and ok
            if not was_pd:
                if ok:
                    lam = max(1e-12, lam / (0.5 * P["lambda_factor"]))
                else:
                    lam *= P["lambda_factor"]
                    if lam > 1e3:
                        lam = 1e3
                        lams.append(lam)
                        failed = i
                        break
                lams.append(lam)
            if ok:
                break
        if failed is not None:
            break
        hgn_norm = float(np.linalg.norm(hgn))
        q, good = 0, False
        with np.errstate(invalid="ignore", divide="ignore"):
            while True:
                q += 1
                if hgn_norm < dlt:
                    h, step = hgn, STEP_GN
                elif hsd_norm > dlt:
                    h, step = dlt / hsd_norm * hsd, STEP_SD
                else:
                    aux = hgn - hsd
                    c = np.float64(np.dot(hsd, aux))                # (numpy scalars: 0/0 and x/0 as the C++ has them)
                    bma2 = np.float64(np.dot(aux, aux))
                    hsd2 = np.float64(np.dot(hsd, hsd))
                    if c <= 0:
                        beta = (-c + np.sqrt(c * c + bma2 * (dlt * dlt - hsd2))) / bma2
                    else:
                        beta = (dlt * dlt - hsd2) / (c + np.sqrt(c * c + bma2 * (dlt * dlt - hsd2)))
                    h, step = hsd + beta * (hgn - hsd), STEP_DL
                lin = -float(np.dot(h, H @ h)) + 2 * float(np.dot(b, h))
                x1 = ref_lm.apply_step(x, hidx, h)
                temp = chi(x1)
                if abs(lin) < 1e-12:
                    lin = 1e-12
                rho = (cur - temp) / lin
                good = bool(rho > 0)
                h_norm = float(np.linalg.norm(h))
                rec = dict(iteration=i, trial=q - 1, step=step, delta=dlt, hgn_norm=hgn_norm, hsd_norm=hsd_norm, h_norm=h_norm,
                           alpha=alpha, current=cur, temp=temp, lin_gain=lin, rho=rho, accept=good)
                if good:
                    x = x1
                    cur = temp
                if rho > 0.75:
                    dlt = max(dlt, 3.0 * h_norm)
                elif rho < 0.25:
                    dlt *= 0.5
                rec["delta_after"] = dlt
                trace.append(rec)
                if good or q >= P["max_trials"]:
                    break
        deltas.append(dlt)
        trials.append(q)
        steps.append(step)
        chis.append(cur)
        if q == P["max_trials"] or not good:
            terminated = True
            break
    done = len(deltas)
    chis = chis + [chis[-1]] * (iters + 1 - len(chis))
    return dict(poses=x, chi2=np.array(chis), deltas=np.array(deltas), trials=np.array(trials, dtype=np.int64),
                steps=np.array(steps, dtype=np.int64), iters_done=done, terminated=terminated, failed=failed,
                lambdas=np.array(lams), trace=trace)
