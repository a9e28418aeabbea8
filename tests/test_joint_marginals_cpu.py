"""The joint / pairwise marginals and relative-covariance entry points as the header, the library and the Python layers declare
them, and the float64 reference (ref_joint_marginals.py) against a hand-worked chain and finite differences; no GPU needed.
tests/test_joint_marginals_gpu.py checks what the entry points compute."""
import ctypes
import os
import re

import numpy as np
import pytest

import ref_joint_marginals as J
from cg_mrslam_amd import _lib
from cg_mrslam_amd.graph import GraphSLAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cgmr_marginals_joint", "cgmr_marginals_pairs", "cgmr_relative_covariance"]


def _header():
    return open(os.path.join(ROOT, "include", "cgmr.h")).read()


def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/cgmr.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_symbols_declared_listed_and_exported_version_105():
    lib = _lib.load_library()
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and n in _lib._SYMBOLS and hasattr(lib, n), n
    assert lib.cgmr_version() == 105


@pytest.mark.parametrize("name,nargs", [("cgmr_marginals_joint", 13), ("cgmr_marginals_pairs", 16), ("cgmr_relative_covariance", 18)])
def test_prototypes_take_the_graph_arguments_then_a_nullable_robust_description(name, nargs):
    args = _prototype(name)
    ref = _prototype("cgmr_marginals")
    assert len(args) == nargs, args
    strip = lambda a: re.sub(r"\s*\w+$", "", a)   # noqa: E731  (the type without the parameter's name)
    assert [strip(a) for a in args[:9]] == [strip(a) for a in ref[:9]]
    assert args[-1].startswith("const cgmr_robust*")


def test_header_states_the_limit_python_agrees():
    m = re.search(r"#define\s+CGMR_JOINT_MAX_QUERIES\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.JOINT_MAX_QUERIES


def test_null_context_is_invalid():
    lib = _lib.load_library()
    e_invalid = int(re.search(r"#define\s+CGMR_E_INVALID\s+\((-?\d+)\)", _header()).group(1))
    null = ctypes.c_void_p(0)
    tails = {"cgmr_marginals_joint": 3, "cgmr_marginals_pairs": 6, "cgmr_relative_covariance": 8}
    for n, k in tails.items():
        args = [null, ctypes.c_int(1), null, null, ctypes.c_int(0), null, null, null, null, ctypes.c_int(0)] + [null] * k
        assert getattr(lib, n)(*args) == e_invalid, n


def test_python_layers_expose_the_calls():
    for n in ("marginals_joint", "marginals_pairs", "relative_covariance"):
        assert callable(getattr(_lib.Context, n, None)), n
    for n in ("computeMarginalBlocks", "jointMarginal", "relativeCovariance", "computeMarginals"):
        assert callable(getattr(GraphSLAM, n, None)), n


def _chain_joint(query):
    g = J.chain_graph()
    return g, J.joint_dense(g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"], query)


def test_reference_reproduces_the_hand_worked_chain():
    q = [4, 0, 2, 5, 2, 1, 3]
    g, S = _chain_joint(q)
    blk = lambda j, k: S[3 * q.index(j):3 * q.index(j) + 3, 3 * q.index(k):3 * q.index(k) + 3]   # noqa: E731
    for j in range(1, 6):
        for k in range(1, 6):
            assert abs(blk(j, k)[0, 0] - min(j, k) / 100) <= 1e-12
            assert abs(blk(j, k)[2, 2] - min(j, k) / 1000) <= 1e-12
    assert abs(blk(2, 4)[1, 2] - 0.001) <= 1e-12 and abs(blk(2, 4)[2, 1] - 0.005) <= 1e-12
    assert np.abs(blk(4, 2) - blk(2, 4).T).max() <= 1e-15
    i0 = 3 * q.index(0)
    assert np.all(S[i0:i0 + 3] == 0) and np.all(S[:, i0:i0 + 3] == 0)
    assert np.array_equal(S[6:9], S[12:15])                                     # vertex 2, listed twice
    want = np.array([[.03, 0, 0], [0, .035, .003], [0, .003, .003]])
    p = g["poses"]
    for a, b in [(1, 4), (2, 5), (0, 3)]:
        Sz = J.relative_cov(p[a], p[b], blk(a, a), blk(a, b), blk(b, b))
        assert np.abs(Sz - want).max() <= 1e-12, (a, b)
    assert np.abs(J.relative_cov(p[3], p[4], blk(3, 3), blk(3, 4), blk(4, 4)) - np.diag([.01, .01, .001])).max() <= 1e-12
    assert np.abs(J.relative_cov(p[3], p[3], blk(3, 3), blk(3, 3), blk(3, 3))).max() <= 1e-15


def test_reference_mahalanobis_on_the_chain():
    """d2 of a hypothesis one standard deviation off in x, with and without its own noise."""
    q = [3, 4]
    g, S = _chain_joint(q)
    p = g["poses"]
    Sz = J.relative_cov(p[3], p[4], S[0:3, 0:3], S[0:3, 3:6], S[3:6, 3:6])[None]
    z = J.relative_pose(p[3], p[4])[None]
    zh = z + np.array([[0.1, 0, 0]])
    d2, _ = J.mahalanobis(z, Sz, zh)
    assert abs(d2[0] - 1.0) <= 1e-9                                              # 0.1^2 / 0.01
    d2, _ = J.mahalanobis(z, Sz, zh, np.array([[100.0, 0, 0, 100.0, 0, 1000.0]]))
    assert abs(d2[0] - 0.5) <= 1e-9                                              # 0.1^2 / (0.01 + 0.01)
    d2, _ = J.mahalanobis(z, -Sz, zh)
    assert np.isnan(d2[0])


def test_reference_jacobians_match_central_differences():
    rng = np.random.default_rng(5)
    xa = rng.uniform(-3, 3, (20, 3))
    xb = rng.uniform(-3, 3, (20, 3))
    Ja, Jb = J.relative_jacobians(xa, xb)
    h = 1e-6
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        da = (J.relative_pose(xa + d, xb) - J.relative_pose(xa - d, xb))
        db = (J.relative_pose(xa, xb + d) - J.relative_pose(xa, xb - d))
        for dd in (da, db):
            dd[:, 2] = (dd[:, 2] + np.pi) % (2 * np.pi) - np.pi
        # central difference: error h^2 |z'''| / 6 ~ 1e-12 |x|, rounding u |z| / h ~ 1e-9
        assert np.abs(da / (2 * h) - Ja[:, :, k]).max() <= 1e-8
        assert np.abs(db / (2 * h) - Jb[:, :, k]).max() <= 1e-8
