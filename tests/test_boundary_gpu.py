"""The solve paths on the boundary sweeps of tests/boundary_cases.py: a front's border, the top block's width, a front's child
count, one assembly list's length and the number of assembly keys stepped through every value around the kernels' tile, chunk
and list constants.  tests/test_boundary_cpu.py proves on the CPU that every constant has a case on either side.  The
yardsticks and their bars are the suite's own: ref_numpy.step_backward_error at OMEGA_MAX, np.linalg.inv of the numpy H at
MARG_TAU (diagonal, edge and joint blocks), ref_lm and ref_dogleg traces, and the host's structure, entry for entry.  One test
per family and check; every case is small."""
import ctypes

import numpy as np
import pytest

import boundary_cases as B
import ref_dogleg
import ref_joint_marginals as J
import ref_lm
import ref_numpy as R
import reference_cases as C
import test_dogleg_gpu as DL
import test_lm_gpu as LM
import test_topology_gpu as TG
from reference_cases import OMEGA_MAX
from test_gn_gpu import _asm_lists, _work_records
from test_joint_marginals_gpu import MARG_TAU as JOINT_TAU
from test_reference_gpu import MARG_TAU
from test_reference_gpu import ctx_resident_only  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

SOLVED = [f for f in B.FAMILIES if f not in B.STRUCTURE_ONLY]
JOINT = ["clique", "blobs", "forest2", "forest9"]


# ------------------------------------------------------------------------------------------------ 1. Gauss-Newton step
@pytest.mark.parametrize("family", list(B.FAMILIES))
def test_gn_step_backward_error(ctx, ctx_resident_only, family):
    """One step from the initial guess on both contexts; fixed vertices keep their bits."""
    worst, at = 0.0, None
    for name in B.FAMILIES[family]:
        g = B.graph(name)
        a = C.args(g)
        dead = TG._dead(g)
        for c in (ctx, ctx_resident_only):
            rc, p1, _ = c.gn_optimize(*a, 1)
            assert rc == 0, name
            assert np.array_equal(p1[dead], g["poses"][dead]), name
            if name in B.NO_STEP_CHECK:
                continue
            w = R.step_backward_error(g["poses"], p1, *a[1:])
            if w > worst:
                worst, at = w, name
            assert w <= OMEGA_MAX, (name, w / R.U)
    print(f"{family}: largest omega {worst / R.U:.1f} u ({at})")


# ---------------------------------------------------------------------------------------------------------- 2. marginals
@pytest.mark.parametrize("family", SOLVED)
def test_marginals_against_the_dense_inverse(ctx, family):
    """Cases of up to DENSE_UP_TO vertices: marginals_all (blocks and cross) and marginals over every vertex."""
    worst, at, n = 0.0, None, 0
    for name in B.FAMILIES[family]:
        g = B.graph(name)
        p = g["poses"]
        V = len(p)
        if V > B.DENSE_UP_TO:
            continue
        n += 1
        a = C.args(g)
        ef, et = g["edge_from"], g["edge_to"]
        hidx, blk = TG._inverse_blocks(g, p)
        cov, cross = ctx.marginals_all(p, g["fixed"], *a[2:], cross=True)
        q = ctx.marginals(p, g["fixed"], *a[2:], np.arange(V, dtype=np.int32))
        w = 0.0
        for v in range(V):
            if hidx[v] < 0:
                assert np.all(cov[v] == 0) and np.all(q[v] == 0), (name, v)
                continue
            nb = np.linalg.norm(blk(v, v))
            w = max(w, np.linalg.norm(cov[v] - blk(v, v)) / nb, np.linalg.norm(q[v] - blk(v, v)) / nb)
        nd = np.array([np.linalg.norm(blk(v, v)) if hidx[v] >= 0 else 0.0 for v in range(V)])
        for k in range(len(ef)):
            if hidx[ef[k]] < 0 or hidx[et[k]] < 0:
                assert np.all(cross[k] == 0), (name, k)
                continue
            w = max(w, np.linalg.norm(cross[k] - blk(ef[k], et[k])) / np.sqrt(nd[ef[k]] * nd[et[k]]))
        if w > worst:
            worst, at = w, name
        assert w <= MARG_TAU, (name, w)
        TG._spd(cov, hidx >= 0)
    assert n >= 4
    print(f"{family}: {n} cases, largest error against the dense inverse {worst:.2e} ({at})")


# ---------------------------------------------------------------------------------------------------- 3. joint marginals
def _spread(g, nK):
    """nK vertices spread evenly over the elimination order: the first leaf's first column .. the last column of the root."""
    from cg_mrslam_amd._lib import gn_symbolic_info
    V = len(g["poses"])
    _, perm = gn_symbolic_info(V, g["fixed"], g["edge_from"], g["edge_to"], want_perm=True)
    order = np.argsort(perm)
    return order[np.unique(np.linspace(0, V - 1, nK).round().astype(int))].astype(np.int32)


@pytest.mark.parametrize("family", JOINT)
def test_joint_marginals_straddle_the_leaf_the_mid_front_and_the_top_block(ctx, family):
    worst, at = 0.0, None
    for name in list(B.FAMILIES[family])[::4]:
        g = B.graph(name)
        p = g["poses"]
        a = C.args(g)
        H, hidx = J._system(p, *a[1:])                            # (J.joint_dense, the inverse taken once for both query sets)
        Hinv = np.linalg.inv(H.toarray())
        for nK in (5, 17):
            q = _spread(g, nK)
            S = ctx.marginals_joint(p, *a[1:], q)
            cols = {int(v): Hinv[:, 3 * hidx[v]:3 * hidx[v] + 3] for v in q if hidx[v] >= 0}
            err = J.block_errors(S, J._gather(cols, hidx, q)).max()
            if err > worst:
                worst, at = err, (name, nK)
            assert np.array_equal(S, S.T), (name, nK)
            assert err <= JOINT_TAU, (name, nK, err)
    print(f"{family}: largest joint block error against the dense inverse {worst:.2e} {at}")


# ------------------------------------------------------------------------------------------- 4. device-built structure
def _worklist(lib, c, n_fronts):
    cap = 8 * n_fronts + 64
    front, chunk = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    parent, level, ns = (np.zeros(n_fronts, np.int32) for _ in range(3))
    P = lambda x: ctypes.c_void_p(x.ctypes.data)   # noqa: E731
    lib.cgmr_debug_worklist.restype = ctypes.c_int
    n = lib.cgmr_debug_worklist(c.h, P(front), P(chunk), ctypes.c_int(cap), P(parent), P(level), P(ns), ctypes.c_int(n_fronts))
    assert 0 < n <= cap
    return front[:n], chunk[:n], parent, level, ns


@pytest.mark.parametrize("family", list(B.FAMILIES))
def test_structure_built_on_the_device_equals_the_hosts(ctx, family):
    """Assembly lists (k_asm_*), row maps, destinations and work records (k_build_maps) against the host's, entry for entry;
    and the work items of the context (front, chunk) are those the chunk lengths of boundary_cases.shape() predict."""
    from cg_mrslam_amd import load_library
    lib = load_library()
    for name in B.FAMILIES[family]:
        g = B.graph(name)
        s = B.shape(name)
        nV, ef, et = len(g["poses"]), g["edge_from"], g["edge_to"]
        ctx.set_symbolic_cache(False)
        try:
            rc, _, _ = ctx.gn_optimize(*C.args(g), 1)
        finally:
            ctx.set_symbolic_cache(True)
        assert rc == 0, name
        ptr_d, src_d = _asm_lists(lib, ctx.h, nV, ef, et)
        ptr_h, src_h = _asm_lists(lib, None, nV, ef, et)
        assert len(src_h) > 0 and np.array_equal(ptr_d, ptr_h) and np.array_equal(src_d, src_h), name
        assert len(ptr_h) - 1 == s["keys"] and np.diff(ptr_h).max() == s["longest_list"], name
        assert np.array_equal(TG._maps(lib, ctx.h, nV, ef, et), TG._maps(lib, None, nV, ef, et)), name
        w_d, w_h = _work_records(lib, ctx.h)
        assert np.array_equal(w_d, w_h), name
        t = s["table"]
        front, chunk, parent, level, ns = _worklist(lib, ctx, len(t))
        assert np.array_equal(parent, t[:, 3]) and np.array_equal(level, t[:, 4]) and np.array_equal(ns, t[:, 2]), name
        rows = [s["chunk"][l] if l < len(s["chunk"]) else B.CHUNK_ROWS for l in t[:, 4]]
        want = {f: max(1, -(-3 * int(t[f, 2]) // rows[f])) for f in range(len(t))}
        got = dict(zip(*np.unique(front, return_counts=True)))
        assert got == want, name
        assert all(np.array_equal(chunk[front == f], np.arange(want[f])) for f in want), name


# --------------------------------------------------------------------------------- 5. Levenberg-Marquardt and dogleg
@pytest.mark.parametrize("name", B.TRACE_CASES)
def test_levenberg_trace_matches_reference(ctx, name):
    g = B.graph(name)
    a = C.args(g)
    ref = ref_lm.lm_optimize(*a, LM.ITERS)
    rc, poses, chi, lam, tri, done = ctx.lm_optimize(*a, LM.ITERS)
    assert rc == 0
    k = LM.check_trace(name, ref, chi, lam, tri, done, LM.rounding_floor(g))
    assert k >= 1, (name, "nothing compared")
    assert np.array_equal(poses[TG._dead(g)], g["poses"][TG._dead(g)])


@pytest.mark.parametrize("name", B.TRACE_CASES)
def test_dogleg_trace_matches_reference(ctx, name):
    g = B.graph(name)
    a = C.args(g)
    ref = ref_dogleg.dl_optimize(*a, DL.ITERS)
    rc, poses, chi, dlt, tri, stp, done = ctx.dl_optimize(*a, DL.ITERS)
    assert rc == 0
    k = DL.check_trace(name, ref, chi, dlt, tri, stp, done, LM.rounding_floor(g))
    assert k >= 1, (name, "nothing compared")
    assert np.array_equal(poses[TG._dead(g)], g["poses"][TG._dead(g)])
