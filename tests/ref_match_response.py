"""Test infrastructure: the float64 yardstick of the scan matcher's response surface (include/cgmr.h, "Scan-match
covariance"), numpy over the CPU oracle's own candidate list.  Never the code under test: not imported by anything
under ``cg_mrslam_amd/`` and importing nothing from it.

``candidates`` asks ``oracle.greedy_search`` for EVERY candidate of a region -- no score bound, result bins a quarter
of the search steps wide, so that every candidate sits in a bin of its own -- and ``response`` applies the definition
to that list in float64.
"""
import math

import numpy as np

# the configuration the helper was checked on when it was written: [-5, 5]^2 at 0.05 m, kernel range 0.2
GRID = ((-5.0, -5.0), (5.0, 5.0), 0.05, 0.2, 128)            # (ll, ur, resolution, kernel_range, kscale)
THETA_RES = 0.02
HALF = (0.2, 0.2, 0.04)                                       # the window's half-widths


def region_around(centre, half=HALF):
    c = np.asarray(centre, dtype=np.float64)
    h = np.asarray(half, dtype=np.float64)
    return np.concatenate([c - h, c + h]).astype(np.float32)


def corridor():
    """Walls y = +-1, x in [-3, 3) every 0.05 m: 240 points."""
    x = -3.0 + 0.05 * np.arange(120)
    return np.concatenate([np.stack([x, np.full_like(x, -1.0)], axis=1), np.stack([x, np.full_like(x, 1.0)], axis=1)])


def room():
    """The corridor plus end walls x = +-3, y in [-1, 1)."""
    y = -1.0 + 0.05 * np.arange(40)
    return np.concatenate([corridor(), np.stack([np.full_like(y, -3.0), y], axis=1), np.stack([np.full_like(y, 3.0), y], axis=1)])


def turned(pts, angle):
    """The points as a scanner turned by ``angle`` sees them: matching them back needs theta = angle."""
    c, s = math.cos(-angle), math.sin(-angle)
    p = np.asarray(pts, dtype=np.float64)
    return np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]], axis=1)


def steps_of(grid, step):
    """(xSteps, the grid's float resolution as double): chargrid.cpp:214-221."""
    res32 = float(np.float32(grid[2]))
    step = res32 if step is None else float(step)
    return max(int(step / res32), 1), res32


def candidates(oracle, grid, ref_pts, qry_pts, region, theta_res, step=None, cap=4096):
    """Every candidate of CharGrid::greedySearch over the region as rows (x, y, theta, score), ascending score: row 0 is
    the winner the search returns."""
    ll, ur, res, kr, ks = grid
    xs, res32 = steps_of(grid, step)
    n, r = oracle.greedy_search(ll, ur, res, res, kr, ref_pts, qry_pts, np.asarray(region, dtype=np.float32).reshape(1, 6),
                                res32 if step is None else float(step), theta_res, 1e6, xs * res32 / 4, xs * res32 / 4,
                                theta_res / 4, kscale=ks, cap=cap)
    assert n <= cap, f"{n} candidates, cap {cap}"
    return r


def information(cov, theta_star, step_x_m, step_y_m, theta_res):
    floor = np.diag([step_x_m ** 2 / 12.0, step_y_m ** 2 / 12.0, theta_res ** 2 / 12.0])
    c, s = math.cos(theta_star), math.sin(theta_star)
    J = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])       # blockdiag(R(theta*)^T, 1)
    return np.linalg.inv(J @ (np.asarray(cov, dtype=np.float64).reshape(3, 3) + floor) @ J.T)


def response(cands, winner, T, grid, theta_res, step=None):
    """The definition in float64 over ``cands`` (rows x, y, theta, score).  Returns the dict the device call returns."""
    xs, res32 = steps_of(grid, step)
    zero = dict(mean=np.zeros(3), cov=np.zeros((3, 3)), info=np.zeros((3, 3)), mass=0.0, border_mass=0.0, n_candidates=0)
    if winner is None:
        return dict(zero, status=2)
    if len(cands) == 0:
        return dict(zero, status=1)
    win = np.asarray(winner, dtype=np.float64)
    w = np.exp(-(cands[:, 3] - win[3]) / T)
    d = cands[:, :3] - win[:3]
    mass = w.sum()
    u = (w[:, None] * d).sum(axis=0) / mass
    cov = (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(axis=0) / mass - np.outer(u, u)
    border = np.zeros(len(cands), dtype=bool)
    for a in range(3):                                               # first or last of its range along x, y or theta
        border |= (cands[:, a] == cands[:, a].min()) | (cands[:, a] == cands[:, a].max())
    return dict(mean=win[:3] + u, cov=cov, info=information(cov, win[2], xs * res32, xs * res32, theta_res), mass=float(mass),
                border_mass=float(w[border].sum() / mass), n_candidates=len(cands), status=0)
