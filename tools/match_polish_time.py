"""Time of polishing a batch of loop-closure matches in one launch (k_match_polish) next to the two generic calls on the same
winners (k_match_refine, then k_match_response + its finish): the 6 x 2 m room of 320 wall points on the loop-closure grid
([-35, 35]^2 at 0.1 m, kernel range 0.5), seen from (0.167, -0.243, 0.0369) with noise of a different seed per job, 160 query
points each; two winners per job -- the search's over scanMatchingLC's region and the same moved by one step in x -- and the
window +-(0.5, 0.5, 0.2) of 1 700 candidates.  The two routes alternate in one process after a warm-up; per route the HIP-event
kernel time of its calls and the host's wall time around them (each call ends with its own synchronisation).
Usage: match_polish_time.py [jobs] [repeats]"""
import math
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cg_mrslam_amd import Context
from cg_mrslam_amd.matcher import LCScanMatcher, PolishParams, RefineParams

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 7
THETA_RES, T = 0.025, 0.01
SEARCH_HALF, WINDOW = np.array([0.5, 1.5, 0.8]), (0.5, 0.5, 0.2)
TRUE = (0.167, -0.243, 0.0369)
x = -3.0 + 0.05 * np.arange(120)
y = -1.0 + 0.05 * np.arange(40)
room = np.concatenate([np.stack([x, np.full_like(x, -1.0)], 1), np.stack([x, np.full_like(x, 1.0)], 1),
                       np.stack([np.full_like(y, -3.0), y], 1), np.stack([np.full_like(y, 3.0), y], 1)])
ctx = Context(0)
m = LCScanMatcher(ctx, 1081, -2.35, 0.004, 30.0)
region = np.concatenate([-SEARCH_HALF, SEARCH_HALF]).astype(np.float32)
c, s = math.cos(TRUE[2]), math.sin(TRUE[2])
p = room[::2] - np.array(TRUE[:2])
seen = np.stack([c * p[:, 0] + s * p[:, 1], -s * p[:, 0] + c * p[:, 1]], 1)
polish_jobs, refine_jobs, response_jobs = [], [], []
for seed in range(N):
    qry = seen + np.random.default_rng(seed).normal(0, 0.01, size=seen.shape)
    win = m.greedySearch(room, qry, region, THETA_RES, 1e6, 0.5, 0.5, 0.5)[0]
    wins = [win, win + np.array([0.1, 0.0, 0.0, 0.0])]
    polish_jobs.append((room, qry, wins))
    for w in wins:
        h = np.array(WINDOW)
        refine_jobs.append((room, qry, w))
        response_jobs.append((room, qry, np.concatenate([(w[:3] - h).astype(np.float32), (w[:3] + h).astype(np.float32)]), w))
par = PolishParams(T=T, window=WINDOW, refine=RefineParams())
k_one, w_one, k_two, w_two, k_ref, k_resp = [], [], [], [], [], []
for _ in range(REP + 1):
    t0 = time.perf_counter()
    pol = m.matchPolishBatch(polish_jobs, THETA_RES, par)
    w_one.append(time.perf_counter() - t0)
    k_one.append(m.last_kernel_seconds())
    t0 = time.perf_counter()
    ref = m.matchRefineBatch(refine_jobs, THETA_RES, RefineParams())
    k_ref.append(m.last_kernel_seconds())
    resp = m.matchResponseBatch(response_jobs, THETA_RES, T)
    w_two.append(time.perf_counter() - t0)
    k_resp.append(m.last_kernel_seconds())
    k_two.append(k_ref[-1] + k_resp[-1])


def fig(v):
    v = 1e6 * np.asarray(v[1:])
    return f"median {np.median(v):.1f} us (min {v.min():.1f}, max {v.max():.1f})"


flat = [e for job in pol for e in job]
same = all(np.array_equal(a["refined"]["pose"], b["pose"]) and a["refined"]["cost"] == b["cost"] for a, b in zip(flat, ref))
print(f"{N} jobs x 2 winners, {REP} timed rounds after one warm-up; statuses refined {sorted({e['refined']['status'] for e in flat})} "
      f"response {sorted({e['response']['status'] for e in flat})}, candidates per window {sorted({e['response']['n_candidates'] for e in flat})}, "
      f"refined poses equal to the refinement call's: {same}")
print(f"one launch  (matchPolishBatch):                    kernel {fig(k_one)}, wall {fig(w_one)}")
print(f"two calls   (matchRefineBatch + matchResponseBatch): kernels {fig(k_two)} [refine {fig(k_ref)}; response {fig(k_resp)}], wall {fig(w_two)}")
