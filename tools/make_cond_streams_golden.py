#!/usr/bin/env python3
"""How tests/golden/cond_streams_r4x6.npz was once recorded: what the per-stream condensed-graph passes computed, on an MI355X.
A record of provenance, not a tool that runs on this tree: the switch it sets, CGMR_COND_BATCH, went with the retired path and
is not in the library's switch table (cg_mrslam_amd/csrc/switches.h), so no library built from this tree is accepted.

    CGMR_LIB=/abs/path/to/parent/libcgmr.so python tools/make_cond_streams_golden.py [--out tests/golden/cond_streams_r4x6.npz]

The passes on streams (every condensed graph as its own stream of launches, CGMR_COND_BATCH=0) are retired; this tool made the
committed record from the last library that had them and stays as its provenance.  Only a library that still has the switch
can make the record again, so CGMR_LIB must name one (a build of the commit before the retirement); any other is refused.  The
run is the child process of tests/test_multirobot_gpu.py's
test_condensed_graphs_as_one_batch_equal_the_recorded_passes_on_streams, script and all, with the switch set: 4 robots, 6 rounds
of 150 vertices on one context.  The fixture holds data only: every robot's wire message, poses and condensed graphs, the
graphs built per round, and a SHA-256 of the world's input arrays.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_multirobot_gpu as T   # noqa: E402

NR = 4


def expected_keys(nr=NR):
    keys = ["built", "world_sha256"]
    for r in range(nr):
        keys += ["wire%d" % r, "poses%d" % r]
        keys += ["%s%d_%d" % (p, r, q) for p in ("to", "est", "iu") for q in range(nr) if q != r]
    return sorted(keys)


def record(lib):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "streams.npz")
        env = dict(os.environ, CGMR_LIB=lib, CGMR_COND_BATCH="0", PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-c", T._BATCH_CHILD, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0 or "rounds ok" not in r.stdout:
            raise RuntimeError("the recording run failed:\n" + r.stderr[-2000:])
        return dict(np.load(path))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=T.COND_STREAMS_GOLDEN)
    a = ap.parse_args()
    lib = os.environ.get("CGMR_LIB")
    if not lib or not os.path.isfile(lib):
        sys.exit("CGMR_LIB must name a libcgmr.so built from a commit that still has the passes on streams")
    if b"CGMR_COND_BATCH" not in open(lib, "rb").read():
        sys.exit(f"{lib} does not read CGMR_COND_BATCH: it has no passes on streams to record")
    fx = record(lib)
    assert sorted(fx) == expected_keys(), sorted(fx)
    n_edges = sum(len(v) for k, v in fx.items() if k.startswith("to"))
    assert fx["built"].sum() > 10 and n_edges > 30, (fx["built"], n_edges)     # what the test asks of its run, of the record alone
    np.savez_compressed(a.out, **fx)
    print(f"{a.out}: {int(fx['built'].sum())} graphs built, {n_edges} condensed edges, world {str(fx['world_sha256'])[:16]}..., "
          f"{os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
