"""Float64 numpy reference of graduated non-convexity (include/cgmr.h: cgmr_gnc_optimize): the executable statement of the
contract.  TEST INFRASTRUCTURE ONLY.

The formulas are recalled from Yang, Antonante, Tzoumas, Carlone, "Graduated Non-Convexity for Robust Spatial Perception"
(RA-L 2020) and from GTSAM's GncOptimizer, not read from either text; this file, not the paper, is what the device is held to.
It is built on ref_typed: ``edge_chi2`` for r_k = e_k^T Omega_k e_k (the factor's own dimension) and one ``gn_optimize``
iteration at a time on ``info * w``.

Every floating-point expression is written in the order the device evaluates it (csrc/gnc_device.h: gnc_weight;
csrc/gnc_kernels.hip), one rounding per operation, so that a branch can differ only where r itself differs."""
import numpy as np

import ref_typed as T

TLS, GM = 0, 1
LOSS = {"tls": TLS, "gm": GM}
# chi2 0.99 quantiles by the factor's dimension (scipy.stats.chi2.ppf(0.99, d))
QUANTILE = {1: 6.634896601021213, 2: 9.21034037197618, 3: 11.344866730144373}
DIM_OF_KIND = {0: 3, 1: 2, 2: 1, 3: 3, 4: 2}
DEFAULTS = dict(mu_factor=1.4, max_outer=100, inner_iters=1)


def default_barc_sq(ek, nE):
    ek = np.zeros(nE, np.uint8) if ek is None else np.asarray(ek)
    return np.array([QUANTILE[DIM_OF_KIND[int(k)]] for k in ek], dtype=np.float64)


def band(loss, mu, c):
    """(lo, up) of the TLS band at mu."""
    return mu / (mu + 1.0) * c, (mu + 1.0) / mu * c


def weights(loss, mu, c, r, known):
    """w [nE] from r at mu; known inliers 1."""
    r = np.asarray(r, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    if loss == TLS:
        lo, up = band(loss, mu, c)
        with np.errstate(divide="ignore", invalid="ignore"):
            mid = np.sqrt(c * mu * (mu + 1.0) / r) - mu
        w = np.where(r >= up, 0.0, np.where(r <= lo, 1.0, mid))
    else:
        mc = mu * c
        q = mc / (r + mc)
        w = q * q
    return np.where(np.asarray(known) != 0, 1.0, w)


def mu_start(loss, c, r, known):
    """(mu0, nothing to reject)."""
    free = np.asarray(known) == 0
    if loss == TLS:
        d = 2.0 * r - c
        m = free & (d > 0)
        if not m.any():
            return 0.0, True
        return float(np.min(c[m] / d[m])), False
    if not free.any():
        return 0.0, True
    mu0 = float(np.max(2.0 * r[free] / c[free]))
    return (0.0, True) if not mu0 > 1.0 else (mu0, False)


class Singular(Exception):
    pass


def _solve(H, b):
    """ref_typed's SuperLU solve; a non-positive diagonal entry is the device's non-positive pivot (an exactly zero block: every
    edge of a free vertex has weight 0)."""
    if H.shape[0] and np.any(H.diagonal() <= 0.0):
        raise Singular
    return T.splu_solve(H, b)


def gnc_optimize(poses, fixed, ef, et, meas, info, vk=None, ek=None, loss="tls", barc_sq=None, known=None, **params):
    """dict(poses, mu [max_outer], cost [max_outer + 1], partial [max_outer], outer_done, weights, edge_chi2, failed (None or the
    failing inner iteration, counted over the call), trace: per outer iteration dict(mu, r, w, x0))."""
    P = dict(DEFAULTS, **params)
    loss = LOSS[loss] if isinstance(loss, str) else int(loss)
    f, max_outer, inner = float(P["mu_factor"]), int(P["max_outer"]), int(P["inner_iters"])
    x = np.array(poses, dtype=np.float64, copy=True)
    nE = len(ef)
    vk, ek = T._kinds(x, ef, vk, ek)
    info = np.asarray(info, dtype=np.float64).reshape(-1, 6)
    c = default_barc_sq(ek, nE) if barc_sq is None else np.broadcast_to(np.asarray(barc_sq, dtype=np.float64), (nE,)).copy()
    known = np.zeros(nE, np.uint8) if known is None else np.asarray(known, dtype=np.uint8)
    free = known == 0
    chi = lambda p: T.edge_chi2(p, ef, et, meas, info, ek)   # noqa: E731
    mu, nothing = mu_start(loss, c, chi(x), known)
    mus, costs, partials, trace = np.zeros(max_outer), np.zeros(max_outer + 1), np.zeros(max_outer, dtype=np.int64), []
    failed, inner_total, t = None, 0, 0
    w = np.ones(nE)
    while True:
        r = chi(x)
        w = np.ones(nE) if nothing else weights(loss, mu, c, r, known)
        mus[t] = 0.0 if nothing else mu
        costs[t] = float(np.sum(w * r))
        partials[t] = int(np.sum(free & (w > 0.0) & (w < 1.0)))
        trace.append(dict(mu=mu, r=r, w=w, x0=x.copy()))
        last = nothing or (partials[t] == 0 if loss == TLS else mu == 1.0) or t == max_outer - 1
        for _ in range(inner):
            try:
                x, _, _ = T.gn_optimize(x, fixed, ef, et, meas, info * w[:, None], 1, vk, ek, solve=_solve)
            except Singular:
                failed = inner_total
                break
            inner_total += 1
        t += 1
        if failed is not None or last:
            break
        mu = mu * f if loss == TLS else max(1.0, mu / f)
    r_end = chi(x)
    costs[t:] = float(np.sum(w * r_end))
    return dict(poses=x, mu=mus, cost=costs, partial=partials, outer_done=t, weights=w, edge_chi2=r_end, failed=failed,
                inner_total=inner_total, trace=trace, barc_sq=c, known=known, nothing=nothing)


def margins(res, loss="tls"):
    """The smallest relative distance, over every outer iteration and free edge, of r from the TLS band's ends lo and up
    (in units of c): a rounding difference below it cannot change a branch."""
    c, free = res["barc_sq"], res["known"] == 0
    worst = np.inf
    if res["nothing"]:
        return worst
    for rec in res["trace"]:
        lo, up = band(TLS, rec["mu"], c)
        d = np.minimum(np.abs(rec["r"] - lo), np.abs(rec["r"] - up)) / c
        if free.any():
            worst = min(worst, float(d[free].min()))
    return worst
