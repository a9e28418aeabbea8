#!/usr/bin/env python3
"""What ranking and pruning laser scans costs beside the occupancy map itself, on the map of DESIGN.md section 8 row f4: 400 scans
x 1081 beams into 700 x 520 cells.

    python tools/gpu_scan_info_time.py [--reps 7] [--prune 100] [--out FILE]

One run, warm (two calls of each before the clock starts), the median of `reps` calls: cgmr_occupancy_map, cgmr_scan_information
and cgmr_scan_prune of `prune` scans -- each as the whole call (staging, launches, results back) and as the device time the call
reports (HIP events around its launches) -- the bytes of the scan windows, and the ratios to the map.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cg_mrslam_amd import Context, synth  # noqa: E402
from cg_mrslam_amd.occupancy import Graph2occupancy  # noqa: E402


def _median(fn, reps):
    for _ in range(2):
        fn()
    wall, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        d = fn()
        wall.append(time.perf_counter() - t0)
        dev.append(d)
    return 1e3 * float(np.median(wall)), 1e3 * float(np.median(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prune", type=int, default=100)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    tr = synth.make_trajectory(400, laps=1.0)
    ctx = Context(0)
    g = Graph2occupancy(ctx, tr["truth"], tr["scans"], tr["angle_min"], tr["angle_inc"], tr["max_range"], rows=700, cols=520, angle=0.0,
                        infinityFillingRange=5.0, usableRange=8.0)

    def occupancy():
        assert g.computeMap()
        return g.kernel_seconds

    occ_call, occ_dev = _median(occupancy, o.reps)
    info_call, info_dev = _median(lambda: g.scanInformation()["kernel_seconds"], o.reps)
    window_bytes, chunks, largest, _ = ctx.scan_info_last_stats()
    prune_call, prune_dev = _median(lambda: g.pruneScans(o.prune)["kernel_seconds"], o.reps)
    info, pruned = g.scanInformation(), g.pruneScans(o.prune)
    assert info["hits"].tobytes() == g.hits.tobytes() and info["misses"].tobytes() == g.misses.tobytes()
    r = dict(scans=len(tr["truth"]), beams=int(tr["scans"].shape[1]), rows=700, cols=520,
             occupancy_call_ms=round(occ_call, 3), occupancy_device_ms=round(occ_dev, 3),
             information_call_ms=round(info_call, 3), information_device_ms=round(info_dev, 3),
             prune_scans=o.prune, pruned=len(pruned["order"]), prune_call_ms=round(prune_call, 3), prune_device_ms=round(prune_dev, 3),
             prune_device_ms_per_round=round(prune_dev / max(len(pruned["order"]), 1), 4),
             window_bytes=window_bytes, window_bytes_mean=int(window_bytes / len(tr["truth"])), window_bytes_largest=largest, chunks=chunks,
             information_over_occupancy=round(info_dev / occ_dev, 2), prune_over_occupancy=round(prune_dev / occ_dev, 2),
             delta_min=float(info["delta"].min()), delta_median=float(np.median(info["delta"])), delta_max=float(info["delta"].max()),
             map_entropy=info["map_entropy"], entropy_after=pruned["entropy_after"], entropy_rise=float(pruned["delta"].sum()))
    line = json.dumps(r)
    print(line, flush=True)
    if o.out:
        with open(o.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
