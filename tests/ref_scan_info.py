"""Test infrastructure: a float64 reference of the scan ranking and the greedy pruning (cgmr_scan_information, cgmr_scan_prune),
written from the definitions alone, on top of tests/ref_occupancy.py (``integrate_scan`` per scan) and of nothing else -- not
from the HIP kernels, not from their host layer.  Nothing under ``cg_mrslam_amd/`` imports this file and it imports nothing from there.

Definitions.  Everything is over the FrequencyMap counters exactly as the occupancy map produces them: ``hits`` with ``gain``,
``misses``, the 9 x 9 fillRobotPose cells, cropping, the infinity filling range, ``square_size``, clipping to the map.

  cell entropy (nats)   f(h, m) = -p ln p - (1 - p) ln(1 - p), p = (h + 1) / (h + m + 2): the Bernoulli entropy of the posterior
                        mean under a uniform prior.  f(0, 0) = ln 2.  In double.  (Not the raw h / (h + m): one observation would
                        make a cell certain.)
  map entropy           H(T) = sum over all rows x cols cells of f(H_c, M_c), T the totals.
  a scan's own counts   (h_s,c, m_s,c): what integrateScan + fillRobotPose of scan s alone adds to cell c.
  information           dH_s(T) = sum over {c : h_s,c + m_s,c > 0} of f(H_c - h_s,c, M_c - m_s,c) - f(H_c, M_c), T containing s:
                        the entropy the map gains if s is dropped.  May be negative: a scan that contradicts the others.
  greedy pruning        All scans alive, T their sum.  Each round: among the alive scans with protected[s] == 0 the minimum of
                        dH_s(T) under the total order (dH, s).  Stop BEFORE taking it if max_remove scans have been removed, or
                        there is no candidate, or max_entropy_increase >= 0 and the cumulative sum of the taken deltas plus this
                        one exceeds it.  Otherwise order[k] = s, delta[k] = dH_s, T loses the scan's counts, s is dead.

Sums are ``math.fsum`` (exactly rounded), so what a comparison measures is the other side's error.  Every sum also reports the
sum of the absolute values of its terms -- the f values that enter it, each counted once -- which is what a floating-point
error of the sum is relative to.
"""
import math

import numpy as np

import ref_occupancy as RO

LN2 = math.log(2.0)


def f(h, m):
    p = (h + 1) / (h + m + 2)
    return -p * math.log(p) - (1 - p) * math.log(1 - p)


def scan_counts(rows, cols, resolution, offset, scans, robot_poses, first_beam_angle, angular_step, laser_max_range,
                laser_pose=(0.0, 0.0, 0.0), max_range=-1.0, usable_range=-1.0, infinity_filling_range=-1.0, gain=1, square_size=1):
    """Per scan (hits, misses), int64 [rows, cols]: the scan integrated alone into an empty map."""
    out = []
    for ranges, pose in zip(scans, robot_poses):
        h = np.zeros((rows, cols), dtype=np.int64)
        m = np.zeros((rows, cols), dtype=np.int64)
        RO.integrate_scan(h, m, resolution, offset, ranges, pose, first_beam_angle, angular_step, laser_max_range, laser_pose,
                          max_range, usable_range, infinity_filling_range, int(gain), int(square_size))
        out.append((h, m))
    return out


def totals(counts, shape, alive=None):
    H = np.zeros(shape, dtype=np.int64)
    M = np.zeros(shape, dtype=np.int64)
    for s, (h, m) in enumerate(counts):
        if alive is None or alive[s]:
            H += h
            M += m
    return H, M


def map_entropy(H, M):
    """(H(T), sum of |terms|)."""
    terms = [f(int(h), int(m)) for h, m in zip(H.ravel().tolist(), M.ravel().tolist())]
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


def delta(h, m, H, M):
    """(dH_s(T), sum of |terms|) of the scan with counts (h, m) against totals (H, M) that contain it."""
    plus, minus = [], []
    for c in np.argwhere((h + m) > 0):
        c = tuple(c)
        plus.append(f(int(H[c] - h[c]), int(M[c] - m[c])))
        minus.append(f(int(H[c]), int(M[c])))
    return math.fsum(plus + [-t for t in minus]), math.fsum(abs(t) for t in plus + minus)


def window(h, m):
    """The bounding box (x0, y0, x1, y1), inclusive, of the cells the scan touches, or None."""
    cells = np.argwhere((h + m) > 0)
    if len(cells) == 0:
        return None
    return int(cells[:, 0].min()), int(cells[:, 1].min()), int(cells[:, 0].max()), int(cells[:, 1].max())


def window_bytes(h, m):
    """What the scan's window takes of the scratch: an int32 pair per cell of the bounding box."""
    w = window(h, m)
    return 0 if w is None else 8 * (w[2] - w[0] + 1) * (w[3] - w[1] + 1)


def chunks(bytes_per_scan, limit):
    """How cgmr_scan_information shares the scans out under a scratch limit (include/cgmr.h): chunks of consecutive scans, each
    filled in scan order until the next window would not fit.  Returns the first scan of every chunk."""
    first, used = [], 0
    for s, b in enumerate(bytes_per_scan):
        if not first or used + b > limit:
            first.append(s)
            used = 0
        used += b
    return first


def information(counts, shape):
    """dict(delta [n], scale [n], cells [n], hit_sum [n], miss_sum [n], hits, misses, map_entropy, map_scale)."""
    H, M = totals(counts, shape)
    d = [delta(h, m, H, M) for h, m in counts]
    e, es = map_entropy(H, M)
    return dict(delta=np.array([v[0] for v in d]), scale=np.array([v[1] for v in d]),
                cells=np.array([int(((h + m) > 0).sum()) for h, m in counts], dtype=np.int64),
                hit_sum=np.array([int(h.sum()) for h, _ in counts], dtype=np.int64),
                miss_sum=np.array([int(m.sum()) for _, m in counts], dtype=np.int64), hits=H, misses=M, map_entropy=e, map_scale=es)


def greedy(counts, shape, max_remove, max_entropy_increase=-1.0, protected=None):
    """The greedy loop.  dict(order, delta, scale (sum of |terms| per taken delta), entropy_before, entropy_after, before_scale,
    after_scale, hits, misses (the final totals), rounds).  ``rounds``: per decision -- the last one is the decision to stop,
    unless max_remove ended the loop -- dict(pick_margin, tie, stop_margin, took): ``pick_margin`` the lowest dH that differs
    from the best minus the best (inf without one), ``tie`` the scans whose dH is bit-equal to the best, the best included,
    ``stop_margin`` the distance of cum + dH from the budget (inf without a budget)."""
    n = len(counts)
    if math.isnan(max_entropy_increase) or max_remove < 0:
        raise ValueError("greedy: bad argument")
    protected = [False] * n if protected is None else [bool(p) for p in protected]
    alive = [True] * n
    H, M = totals(counts, shape)
    before, before_scale = map_entropy(H, M)
    order, deltas, scales, rounds = [], [], [], []
    cum = 0.0
    while len(order) < max_remove:
        cand = sorted((delta(*counts[s], H, M) + (s,) for s in range(n) if alive[s] and not protected[s]), key=lambda t: (t[0], t[2]))
        if not cand:
            break
        d, sc, s = cand[0]
        other = [t[0] for t in cand if t[0] != d]
        rnd = dict(pick_margin=(min(other) - d) if other else math.inf, tie=[t[2] for t in cand if t[0] == d],
                   stop_margin=abs(cum + d - max_entropy_increase) if max_entropy_increase >= 0 else math.inf)
        rnd["took"] = not (max_entropy_increase >= 0 and cum + d > max_entropy_increase)
        rounds.append(rnd)
        if not rnd["took"]:
            break
        order.append(s)
        deltas.append(d)
        scales.append(sc)
        cum += d
        alive[s] = False
        H = H - counts[s][0]
        M = M - counts[s][1]
    after, after_scale = map_entropy(H, M)
    return dict(order=order, delta=np.array(deltas), scale=np.array(scales), entropy_before=before, entropy_after=after,
                before_scale=before_scale, after_scale=after_scale, hits=H, misses=M, rounds=rounds, alive=alive)
