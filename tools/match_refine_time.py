"""HIP-event time of a batch of refinements (k_match_refine) next to the response surface (k_match_response) on the same jobs:
a 6 x 2 m room of 320 wall points on the [-5, 5]^2 grid at 0.05 m, seen from 64 poses within half a cell of the origin, 160
query points each, the winner by the generic search.  Usage: match_refine_time.py [jobs] [repeats]"""
import math
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cg_mrslam_amd import Context
from cg_mrslam_amd.matcher import RefineParams, ScanMatcher

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
THETA_RES, HALF = 0.02, np.array([0.2, 0.2, 0.04])
x = -3.0 + 0.05 * np.arange(120)
y = -1.0 + 0.05 * np.arange(40)
room = np.concatenate([np.stack([x, np.full_like(x, -1.0)], 1), np.stack([x, np.full_like(x, 1.0)], 1),
                       np.stack([np.full_like(y, -3.0), y], 1), np.stack([np.full_like(y, 3.0), y], 1)])
ctx = Context(0)
m = ScanMatcher(ctx, 1081, -2.35, 0.004, 30.0, resolution=0.05, kernel_range=0.2)
m.initializeGrid((-5.0, -5.0), (5.0, 5.0), 0.05)
rng = np.random.default_rng(3)
region = np.concatenate([-HALF, HALF]).astype(np.float32)
refine_jobs, response_jobs = [], []
for _ in range(N):
    px, py, pt = rng.uniform(-0.025, 0.025), rng.uniform(-0.025, 0.025), rng.uniform(-0.01, 0.01)
    c, s = math.cos(pt), math.sin(pt)
    p = room[::2] - np.array([px, py])
    qry = np.stack([c * p[:, 0] + s * p[:, 1], -s * p[:, 0] + c * p[:, 1]], 1) + rng.normal(0, 0.01, size=(160, 2))
    win = m.greedySearch(room, qry, region, THETA_RES, 1e6, 0.5, 0.5, 0.5)[0]
    refine_jobs.append((room, qry, win))
    response_jobs.append((room, qry, region, win))
t_ref, t_resp = [], []
for _ in range(REP + 1):
    r = m.matchRefineBatch(refine_jobs, THETA_RES, RefineParams())
    t_ref.append(m.last_kernel_seconds())
    m.matchResponseBatch(response_jobs, THETA_RES, 0.01)
    t_resp.append(m.last_kernel_seconds())
moves = [q["n_iters"] + q["n_halvings"] + 1 for q in r]
print(f"{N} jobs, {REP} timed calls after one warm-up: refine min {1e6 * min(t_ref[1:]):.1f} us median {1e6 * np.median(t_ref[1:]):.1f} us "
      f"(evaluations per job: mean {np.mean(moves):.1f}, max {max(moves)}; status {sorted({q['status'] for q in r})}); "
      f"response min {1e6 * min(t_resp[1:]):.1f} us median {1e6 * np.median(t_resp[1:]):.1f} us")
