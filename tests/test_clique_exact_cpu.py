"""The exact maximum-clique entry points (cgmr_max_clique_exact, cgmr_closure_consistency_exact) as the header, the library
and the Python layers declare them, and the bit-set branch and bound of ref_clique.py against Bron-Kerbosch
(ref_pcm.max_clique_exact); no GPU needed.  tests/test_clique_exact_gpu.py checks what the entry points compute."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import oracle_backend as OB
import ref_clique as R
import ref_pcm as P
from cg_mrslam_amd import _lib
from cg_mrslam_amd.graph import GraphSLAM
from cg_mrslam_amd.slam import GraphSLAMDriver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cgmr_max_clique_exact": 8, "cgmr_closure_consistency_exact": 22}      # name: arguments


def _header():
    return open(os.path.join(ROOT, "include", "cgmr.h")).read()


def test_symbols_declared_listed_and_exported_version_105():
    lib = _lib.load_library()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    assert lib.cgmr_version() == 105


def test_header_argument_counts_and_the_binding_agree():
    """The declarations carry the issue's argument lists: the greedy call's with node_limit, proven_out (and nodes_out); the
    binding passes that many (the context included)."""
    hdr = _header()
    for n, count in NAMES.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == count, (n, args)
        assert "int64_t node_limit" in args and "int32_t* proven_out" in args
    greedy = re.search(r"\bint\s+cgmr_closure_consistency\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")
    exact = re.search(r"\bint\s+cgmr_closure_consistency_exact\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")
    upto = [a.strip() for a in greedy[:17]]                          # ctx .. adj_out
    assert [a.strip() for a in exact[:17]] == upto and upto[-1] == "uint64_t* adj_out"
    assert [a.strip() for a in exact[17:]] == ["int64_t node_limit", "int32_t* clique_out", "int32_t* clique_size_out",
                                               "int32_t* proven_out", "const cgmr_robust* rk"]
    d = re.search(r"#define\s+CGMR_EXACT_DEFAULT_NODE_LIMIT\s+(\d+)", hdr)
    assert d and int(d.group(1)) == _lib.EXACT_DEFAULT_NODE_LIMIT
    lim = _lib.EXACT_DEFAULT_NODE_LIMIT
    assert lim > 0 and lim & (lim - 1) == 0                          # a power of two
    r = re.search(r"#define\s+CGMR_EXACT_ROUNDS\s+(\d+)", open(os.path.join(ROOT, "cg_mrslam_amd", "csrc", "pcm_device.h")).read())
    assert r and int(r.group(1)) == _lib.EXACT_ROUNDS


def test_null_context_is_invalid():
    lib = _lib.load_library()
    e_invalid = int(re.search(r"#define\s+CGMR_E_INVALID\s+\((-?\d+)\)", _header()).group(1))
    null = ctypes.c_void_p(0)
    graph = [null, ctypes.c_int(1), null, null, ctypes.c_int(0), null, null, null, null]
    args = graph + [ctypes.c_int(0), null, null, null, null, ctypes.c_double(1.0), null, null, ctypes.c_int64(1)] + [null] * 4
    assert len(args) == NAMES["cgmr_closure_consistency_exact"]
    assert lib.cgmr_closure_consistency_exact(*args) == e_invalid
    assert lib.cgmr_max_clique_exact(null, ctypes.c_int(0), null, ctypes.c_int64(1), null, null, null, null) == e_invalid


def test_python_layers_expose_the_calls():
    for n in ("closure_consistency_exact", "max_clique_exact"):
        assert callable(getattr(_lib.Context, n, None)), n
    assert inspect.signature(_lib.Context.max_clique_exact).parameters["node_limit"].default == _lib.EXACT_DEFAULT_NODE_LIMIT
    sig = inspect.signature(GraphSLAM.closureConsistency).parameters
    assert sig["exact"].default is False and "node_limit" in sig
    assert inspect.signature(GraphSLAM.consistentClosures).parameters["exact"].default is False
    d = GraphSLAMDriver(OB.OracleContext(), None, None, closure_check=("pcm-exact", 9.0))
    assert d.closure_check == ("pcm-exact", 9.0)
    for bad in (("pcm-exact", 0), ("pcm-exact", -1.0), ("pcm-exactly", 9.0), ("pcm-exact",)):
        with pytest.raises(ValueError) as ei:
            GraphSLAMDriver(OB.OracleContext(), None, None, closure_check=bad)
        assert "pcm-exact" in str(ei.value)
    assert GraphSLAMDriver(OB.OracleContext(), None, None).closure_check == "voting"
    assert GraphSLAMDriver(OB.OracleContext(), None, None, closure_check=("pcm", 9.0)).closure_check == ("pcm", 9.0)


# ------------------------------------------------------------------------------------------- the reference
def _small_cases():
    """Every n <= 20 graph tests/test_clique_exact_gpu.py uses."""
    for n in (1, 2, 3, 20):
        rng = np.random.default_rng(n)
        for dens in (0.1, 0.5, 0.9):
            yield (n, dens), P.random_graph(n, dens, rng)
    yield "greedy misses", P.random_graph(20, 0.5, np.random.default_rng(20187))
    yield "two triangles", P.two_triangles()
    for n in (1, 5):
        yield ("empty", n), np.zeros((n, n), dtype=bool)
        yield ("complete", n), ~np.eye(n, dtype=bool)


def test_reference_equals_bron_kerbosch_on_the_small_cases():
    for name, A in _small_cases():
        members, nodes = R.max_clique(A)
        assert R.is_clique(A, members) and len(members) == len(P.max_clique_exact(A)) and nodes >= 1, name
        assert R.omega(A) == (len(members), nodes)


def test_reference_equals_bron_kerbosch_on_200_random_graphs():
    rng = np.random.default_rng(2018)
    for t in range(200):
        n = int(rng.integers(1, 17))
        A = P.random_graph(n, float(rng.uniform(0.05, 0.95)), rng)
        members, _ = R.max_clique(A)
        assert R.is_clique(A, members) and len(members) == len(P.max_clique_exact(A)), (t, n)


def test_reference_lower_bound_and_trivial_graphs():
    assert R.max_clique(np.zeros((0, 0), dtype=bool))[0] == []
    assert len(R.max_clique(np.zeros((4, 4), dtype=bool))[0]) == 1
    assert R.max_clique(~np.eye(6, dtype=bool)) == ([0, 1, 2, 3, 4, 5], 7)
    A = P.random_graph(20, 0.5, np.random.default_rng(20187))
    assert P.greedy_clique(A)[1] == 4 and R.omega(A)[0] == 5           # the case the greedy heuristic misses
    assert len(R.max_clique(A, lower_bound=4)[0]) == 5 and R.max_clique(A, lower_bound=5)[0] == []
    assert not R.is_clique(A, [0, 0]) and not R.is_clique(P.two_triangles(), [0, 1, 2]) and R.is_clique(P.two_triangles(), [1, 3, 5])
