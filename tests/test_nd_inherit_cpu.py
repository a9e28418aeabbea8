"""Nested dissection, CGMR_ND_INHERIT (csrc/gn_symbolic.cpp: NDGiven): a node whose first sweep would repeat, bit for bit, a
sweep its caller already holds -- the near half of a level structure, the first component of a disconnected range -- takes
the caller's instead.  Nothing the analysis gives out may differ from a run that sweeps anew (CGMR_ND_INHERIT=0): the
permutation, the front table and every info field but the two times, on one host thread and on eight.  No device.

The switch is read by the call, CGMR_HOST_THREADS once per process: each of the four settings analyses every graph in a
child process of its own (the four run side by side), under CGMR_SYM_TRACE, whose "nd: sweeps inherited" line says how many
nodes took a caller's sweep -- a comparison that passes with the feature dead proves nothing."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys, json, hashlib, numpy as np
sys.path.insert(0, sys.argv[1])
from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import gn_symbolic_info, gn_symbolic_info_grown, gn_front_table

def digest(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()

def sizes(info):
    return {k: v for k, v in info.items() if not k.endswith("_us")}

def mark(name):
    sys.stderr.write("GRAPH %s\n" % name); sys.stderr.flush()

def analyse(name, V, ef, et, fixed=None):
    fixed = np.zeros(V, np.uint8) if fixed is None else fixed
    ef, et = np.asarray(ef, np.int32), np.asarray(et, np.int32)
    mark(name)
    info, perm = gn_symbolic_info(V, fixed, ef, et, want_perm=True)
    mark("(front table of %s)" % name)
    out[name] = dict(perm=digest(perm), fronts=digest(gn_front_table(V, fixed, ef, et)), info=sizes(info))

def joined(parts):
    # disjoint pose graphs side by side: the vertices of the first part first
    ef, et, base = [], [], 0
    for (V, E, seed) in parts:
        g = synth.make_pose_graph(V, E, seed=seed)
        ef.append(g["edge_from"] + base); et.append(g["edge_to"] + base); base += V
    return base, np.concatenate(ef), np.concatenate(et)

out = {}
for (V, E, seeds) in ((40, 60, (1, 2, 3, 4, 5)), (300, 1100, (1, 2, 3, 7)), (2000, 8000, (1, 2, 7)), (10000, 40000, (12345, 1))):
    for seed in seeds:
        g = synth.make_pose_graph(V, E, seed=seed, strict=(V == 10000))
        analyse("pose %d seed %d" % (V, seed), V, g["edge_from"], g["edge_to"], g["fixed"])
# three components: the one the range starts in (its first sweep's) is the largest, the smallest, the middle one; and a
# first component of a size at which the root runs its side-by-side sweeps and keeps them
analyse("components 900+300+500", *joined(((900, 3400, 1), (300, 1100, 2), (500, 1800, 3))))
analyse("components 300+900+500", *joined(((300, 1100, 2), (900, 3400, 1), (500, 1800, 3))))
analyse("components 500+900+300", *joined(((500, 1800, 3), (900, 3400, 1), (300, 1100, 2))))
analyse("components 3000+1200+700", *joined(((3000, 11000, 5), (1200, 4500, 6), (700, 2600, 8))))
# a hub (a peer's star: 60 edges at one vertex) kept out of the dissection
g = synth.make_pose_graph(2000, 8000, seed=9)
rng = np.random.default_rng(4)
ends = [int(v) for v in rng.choice(2000, size=60, replace=False) if int(v) != 777]
analyse("hub", 2000, np.concatenate([g["edge_from"], np.minimum(777, ends)]), np.concatenate([g["edge_to"], np.maximum(777, ends)]), g["fixed"])
# a path; a star below the hub rule's degree and one above it (its rays: a range of single vertices, no edge among them)
analyse("path", 700, np.arange(699), np.arange(1, 700))
analyse("star 24", 25, np.zeros(24, np.int32), np.arange(1, 25))
analyse("star 200", 201, np.zeros(200, np.int32), np.arange(1, 201))
# a grown sequence: chunks of 50 (a multi-robot round) and key frame by key frame at the end of the trajectory, where the
# last leaf outgrows its two panels again and again and is dissected anew
g = synth.make_pose_graph(3000, 11000, seed=8)
k = np.argsort(np.maximum(g["edge_from"], g["edge_to"]), kind="stable")
ef, et = np.ascontiguousarray(g["edge_from"][k]), np.ascontiguousarray(g["edge_to"][k])
last = np.maximum(ef, et)
for chunk, v0 in ((50, 600), (1, 2900)):
    nv = np.arange(v0 + chunk, 3000 + 1, chunk)
    mark("grown by %d" % chunk)
    info, perm, n_ext = gn_symbolic_info_grown(v0, int(np.searchsorted(last, v0, side="left")), nv, np.searchsorted(last, nv, side="left"), ef, et)
    out["grown by %d" % chunk] = dict(perm=digest(perm), fronts="", info=dict(sizes(info), steps_extended=n_ext))
print(json.dumps(out))
"""

SETTINGS = [(inherit, threads) for threads in ("1", "8") for inherit in ("0", "1")]


@pytest.fixture(scope="module")
def runs():
    """{(inherit, threads): (results per graph, {graph: (near halves, first components) taken from their callers})}"""
    procs = {}
    for s in SETTINGS:
        env = dict(os.environ, CGMR_ND_INHERIT=s[0], CGMR_HOST_THREADS=s[1], CGMR_SYM_TRACE="1")
        procs[s] = subprocess.Popen([sys.executable, "-c", _CHILD, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    got = {}
    for s, p in procs.items():
        stdout, stderr = p.communicate(timeout=300)
        assert p.returncode == 0, stderr[-2000:]
        taken, name = {}, None
        for line in stderr.splitlines():
            m = re.match(r"GRAPH (.*)", line)
            if m:
                name = m.group(1)
            m = re.search(r"nd: sweeps inherited\s+(\d+) near halves, (\d+) first components", line)
            if m:
                near, first = taken.get(name, (0, 0))
                taken[name] = (near + int(m.group(1)), first + int(m.group(2)))
        got[s] = (json.loads(stdout.strip().splitlines()[-1]), taken)
    return got


@pytest.mark.parametrize("threads", ["1", "8"])
def test_inherited_sweeps_change_nothing(runs, threads):
    anew, taken = runs[("0", threads)][0], runs[("1", threads)][0]
    assert len(anew) == 24 and sorted(anew) == sorted(taken)
    for name in anew:
        for piece in ("perm", "fronts", "info"):
            assert anew[name][piece] == taken[name][piece], (name, piece, anew[name][piece], taken[name][piece])


def test_result_does_not_depend_on_the_thread_count(runs):
    assert runs[("1", "1")][0] == runs[("1", "8")][0]


@pytest.mark.parametrize("threads", ["1", "8"])
def test_the_sweeps_are_really_inherited(runs, threads):
    """On the benchmark graph (10 000 poses, seed 12345) every inner node below the root has a near half -- hundreds of them --
    and the far half of the root is a disconnected range: both kinds must have been taken, by the same nodes whatever the
    thread count; and a named component graph takes its first component's.  With the switch off, none."""
    on, off = runs[("1", threads)][1], runs[("0", threads)][1]
    assert all(v == (0, 0) for v in off.values()) and "pose 10000 seed 12345" in off
    near, first = on["pose 10000 seed 12345"]
    assert near >= 100 and first >= 1, (near, first)
    assert on["pose 10000 seed 1"][0] >= 100
    for name in ("components 900+300+500", "components 300+900+500", "components 500+900+300"):
        assert on[name][1] >= 1 and on[name][0] >= 10, (name, on[name])
    assert on["components 3000+1200+700"][1] >= 1                     # (the 1200 of the rest; the 3000 keep the root's four sweeps)
    assert on == runs[("1", "1")][1]
