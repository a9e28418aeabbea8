"""The host analysis on path graphs around the 2048-vertex threshold of the root's multi-start sweep (gn_symbolic.cpp, nd()).

On a chain swept from one end the level structure has as many levels as vertices; the root copied one count more than the
range's scratch slice holds -- four bytes past a vector of nf ints, from 2048 poses on.  Two checks:
  * the chains through every host entry that analyses (gn_symbolic_info, gn_front_table, the host half of
    cgmr_debug_asm_lists), several rounds in one process: the library once aborted in glibc ("double free or corruption") on
    such a sequence.  No sanitizer: what this pins is that the results are consistent and repeat.
  * tests/host/symbolic_sweep.cpp, the stand-alone harness, built with the host AddressSanitizer and
    UndefinedBehaviorSanitizer and run as its own process with one and with four analysis threads; beside it, built and run the
    same way, tests/host/wire_sweep.cpp: the host's writer and reader of the inter-robot wire format (wire_format.h) on hostile
    slices.  Host code only: skipped where a GPU is visible, or where the compiler or its sanitizer runtime is missing."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cg_mrslam_amd import load_library
from cg_mrslam_amd._lib import gn_front_table, gn_symbolic_info
from test_gn_gpu import _asm_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = (2047, 2048, 2049, 4096, 32769, 32770)
ROUNDS = 3


def _check_chain(V, info, perm, t, ptr, src):
    assert info["free_poses"] == V and info["offdiag_blocks"] == V - 1
    assert np.array_equal(np.sort(perm), np.arange(V))                      # a bijection onto the columns
    c0, nc, ns, parent, level, nchild = t.T
    assert len(t) == info["fronts"] and np.array_equal(c0, np.r_[0, np.cumsum(nc)[:-1]]) and c0[-1] + nc[-1] == V
    assert np.all((nc >= 1) & (nc <= 16)) and np.array_equal(parent < 0, ns == 0)
    has = parent >= 0
    assert np.all(parent[has] > np.flatnonzero(has)) and np.all(level[parent[has]] > level[has])
    assert np.array_equal(np.bincount(parent[has], minlength=len(t)), nchild) and np.array_equal(nchild == 0, level == 0)
    assert level.max() + 1 == info["levels"]
    # the assembly lists: V diagonal blocks (the two ends: one term, the others two), V - 1 off-diagonal ones (one term)
    assert len(ptr) == 2 * V and ptr[0] == 0 and ptr[-1] == len(src) == 3 * (V - 1) and np.all(np.diff(ptr) >= 1)
    assert np.array_equal(np.sort(np.diff(ptr[:V + 1])), np.r_[1, 1, np.full(V - 2, 2)]) and np.all(np.diff(ptr[V:]) == 1)
    assert np.array_equal(np.bincount(src >> 2, minlength=V - 1), np.full(V - 1, 3))


def test_chains_across_the_multi_start_threshold_repeat_in_one_process():
    lib = load_library()
    first = {}
    for _ in range(ROUNDS):
        for V in CHAINS:
            ef, et = np.arange(V - 1, dtype=np.int32), np.arange(1, V, dtype=np.int32)
            fixed = np.zeros(V, dtype=np.uint8)
            info, perm = gn_symbolic_info(V, fixed, ef, et, want_perm=True)
            t = gn_front_table(V, fixed, ef, et)
            ptr, src = _asm_lists(lib, None, V, ef, et)
            _check_chain(V, info, perm, t, ptr, src)
            got = (perm, t, ptr, src)
            if V in first:
                assert all(np.array_equal(a, b) for a, b in zip(first[V], got)), V
            first[V] = got


def _gpu_visible():
    if os.path.exists("/dev/kfd"):
        return True
    try:
        import torch
        return bool(torch.cuda.is_available())
    except Exception:
        return False


def test_sanitized_host_harness(tmp_path):
    if _gpu_visible():
        pytest.skip("host sanitizers run on machines without a GPU only")
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx or not shutil.which("make"):
        pytest.skip("no clang++ / make")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler's sanitizer runtime is missing")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "host"), "BUILD=" + str(tmp_path / "build"), "CXX=" + cxx, "check"],
                       capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    done = [l for l in r.stdout.splitlines() if l.startswith("symbolic_sweep:") and "analyses checked" in l]
    assert len(done) == 2 and all(l.endswith(" 0 failed") for l in done), done
    # the second program of `make check`: the wire format's writer and reader (tests/host/wire_sweep.cpp)
    wire = [l for l in r.stdout.splitlines() if l.startswith("wire_sweep:") and l.endswith(" cases checked")]
    assert len(wire) == 1 and int(wire[0].split()[1]) > 1000, wire
