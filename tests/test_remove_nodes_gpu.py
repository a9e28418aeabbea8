"""cgmr_remove_nodes on the device against the float64 reference (tests/ref_remove_nodes.py) on the cases
tests/test_remove_nodes_cpu.py has proved: offsets, ends and flags exactly (the reference's decision margin makes that fair),
the measurements at MEAS_ATOL, the informations at INFO_MARGIN times the gap first measured, the weights within half the
decision margin; two calls byte for byte; every refusal through the bare C ABI; GraphSLAM.removeVertices on the ring.

Measured on an MI355X (the largest over the cases): measurements 1.8e-15, weights 6.8e-13 nats (the smallest decision margin:
2.9e-4), information 3.556e-13 of its norm (the 300-vertex lattice; 8.4e-14 at 16 neighbours, 1.4e-15 or less at two) --
remove_nodes_cases.INFO_GAP, the bar ten times it; optimize(5) after removeVertices against the reference's pruned optimum
2.6e-11 (one round) and 7.6e-10 (two)."""
import ctypes as C

import numpy as np
import pytest

import ref_numpy as R
import ref_remove_nodes as RN
import remove_nodes_cases as K
from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
from cg_mrslam_amd._lib import CgmrError
from condense_tree_cases import info_full as _full
from reference_cases import EST_ATOL

pytestmark = pytest.mark.gpu

E_INVALID = -1
_DEV = {}


def _dev(ctx, name):
    """Context.remove_nodes on a case, once (never modified)."""
    if name not in _DEV:
        nV, ef, et, meas, info, remove = K.case(name)
        _DEV[name] = ctx.remove_nodes(ef, et, meas, info, remove, num_vertices=nV)
    return _DEV[name]


def info_gap(iu, ref):
    """The largest ||I - I_ref||_F / ||I_ref||_F over the edges (0 with none)."""
    return max([np.linalg.norm(_full(a) - _full(b)) / np.linalg.norm(_full(b)) for a, b in zip(iu, ref)] + [0.0])


@pytest.mark.parametrize("name", list(K.CASES))
def test_device_against_the_reference(ctx, name):
    off, fr, to, z, iu, w, fl = _dev(ctx, name)
    r = K.reference(name)
    assert np.array_equal(fl, r["flags"]) and np.all(fl == K.FLAGS.get(name, 0))
    assert np.array_equal(off, r["off"]) and np.array_equal(fr, r["fr"]) and np.array_equal(to, r["to"])
    d = z - r["est"]
    d[:, 2] = R.normalize_theta(d[:, 2])
    dz = np.abs(d).max() if len(d) else 0.0
    dw = np.abs(w - r["weight"]).max() if len(w) else 0.0
    gap = info_gap(iu, r["iu"])
    print(f"{name}: {len(to)} edges, meas {dz:.2e}, weights {dw:.2e} nats, information {gap:.3e} of its norm")
    assert dz <= K.MEAS_ATOL
    assert dw <= 0.5 * K.MARGIN_MIN                                # (within it no weight can change the reference's tree)
    assert gap <= K.INFO_MARGIN * K.INFO_GAP


@pytest.mark.parametrize("name", ["deg16", "lattice300"])
def test_two_calls_give_identical_bytes(ctx, name):
    nV, ef, et, meas, info, remove = K.case(name)
    a = _dev(ctx, name)
    b = ctx.remove_nodes(ef, et, meas, info, remove, num_vertices=nV)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def _raw(ctx, nV, ef, et, meas, info, remove, cap=None, nE=None, nR=None, null=()):
    """The bare C ABI with the outputs sized for `cap` edges; null: the names of pointers passed as NULL."""
    nE = len(ef) if nE is None else nE
    nR = len(remove) if nR is None else nR
    cap = 64 if cap is None else cap
    a = dict(ef=np.ascontiguousarray(ef, np.int32), et=np.ascontiguousarray(et, np.int32), meas=np.ascontiguousarray(meas, np.float64),
             info=np.ascontiguousarray(info, np.float64), remove=np.ascontiguousarray(remove, np.int32),
             off=np.zeros(max(nR, 0) + 1, np.int32), fr=np.zeros(max(cap, 1), np.int32), to=np.zeros(max(cap, 1), np.int32),
             z=np.zeros((max(cap, 1), 3)), iu=np.zeros((max(cap, 1), 6)), w=np.zeros(max(cap, 1)), fl=np.zeros(max(nR, 1), np.int32))
    p = {k: (C.c_void_p(0) if k in null else C.c_void_p(v.ctypes.data)) for k, v in a.items()}
    rc = ctx.lib.cgmr_remove_nodes(ctx.h, C.c_int(nV), C.c_int(nE), p["ef"], p["et"], p["meas"], p["info"], C.c_int(nR), p["remove"],
                                   C.c_int(cap), p["off"], p["fr"], p["to"], p["z"], p["iu"], p["w"], p["fl"])
    return rc, a


def test_refusals_through_the_c_abi(ctx):
    nV, ef, et, meas, info, remove = K.case("deg5")
    v = int(remove[0])
    ok, a = _raw(ctx, nV, ef, et, meas, info, remove)
    assert ok == 4 and a["off"].tolist() == [0, 4]
    rc, a = _raw(ctx, nV, ef, et, meas, info, remove, null=("w",))          # weight_out is nullable
    assert rc == 4
    assert _raw(ctx, nV, ef, et, meas, info, remove, cap=4)[0] == 4          # the sum of m - 1 suffices
    assert ctx.lib.cgmr_remove_nodes(None, *([C.c_int(0)] * 2), *([C.c_void_p(0)] * 4), C.c_int(0), C.c_void_p(0), C.c_int(0),
                                     *([C.c_void_p(0)] * 7)) == E_INVALID
    for null in ("ef", "et", "meas", "info", "remove", "off", "fl", "fr", "to", "z", "iu"):
        assert _raw(ctx, nV, ef, et, meas, info, remove, null=(null,))[0] == E_INVALID, null
    assert _raw(ctx, 0, ef, et, meas, info, remove)[0] == E_INVALID
    assert _raw(ctx, nV, ef, et, meas, info, remove, nE=-1)[0] == E_INVALID
    assert _raw(ctx, nV, ef, et, meas, info, remove, nR=-1)[0] == E_INVALID
    assert _raw(ctx, nV, ef, et, meas, info, remove, cap=-1)[0] == E_INVALID
    assert _raw(ctx, nV, ef, et, meas, info, remove, cap=3)[0] == E_INVALID  # cap_out too small
    bad = ef.copy(); bad[2] = nV
    assert _raw(ctx, nV, bad, et, meas, info, remove)[0] == E_INVALID
    bad = et.copy(); bad[0] = -1
    assert _raw(ctx, nV, ef, bad, meas, info, remove)[0] == E_INVALID
    assert _raw(ctx, nV, ef, et, meas, info, [nV])[0] == E_INVALID
    assert _raw(ctx, nV, ef, et, meas, info, [-1])[0] == E_INVALID
    assert _raw(ctx, nV, ef, et, meas, info, [v, 3, v])[0] == E_INVALID     # repeated
    assert "twice" in ctx.lib.cgmr_last_error(ctx.h).decode()
    se, st_ = np.r_[ef, v].astype(np.int32), np.r_[et, v].astype(np.int32)   # a self edge on the removed vertex
    assert _raw(ctx, nV, se, st_, np.vstack([meas, meas[:1]]), np.vstack([info, info[:1]]), remove)[0] == E_INVALID
    assert "itself" in ctx.lib.cgmr_last_error(ctx.h).decode()
    assert _raw(ctx, *K.not_independent())[0] == E_INVALID                   # two removed vertices joined by an edge
    assert "independent" in ctx.lib.cgmr_last_error(ctx.h).decode()
    with pytest.raises(CgmrError):
        ctx.remove_nodes(*K.not_independent()[1:], num_vertices=K.not_independent()[0])
    rc, a = _raw(ctx, nV, ef, et, meas, info, remove, nR=0)
    assert rc == 0
    off, fr, to, z, iu, w, fl = ctx.remove_nodes(ef, et, meas, info, [], num_vertices=nV)
    assert off.tolist() == [0] and len(fr) == 0 and len(fl) == 0
    # a self edge elsewhere in the graph is none of this call's business
    se, st_ = np.r_[ef, 39].astype(np.int32), np.r_[et, 39].astype(np.int32)
    assert _raw(ctx, nV, se, st_, np.vstack([meas, meas[:1]]), np.vstack([info, info[:1]]), remove)[0] == 4


# --------------------------------------------------------------------------------------- GraphSLAM.removeVertices on the ring
def _ring_slam(ctx):
    (poses, fixed, ef, et, meas, info), remove = K.ring_case()
    n = len(poses)
    g = PoseGraph(100 + 7 * np.arange(n), poses, fixed, ef, et, meas, info)
    g.lasers = {v: f"laser of {v}" for v in range(n)}
    return GraphSLAM(g, ctx), (poses, fixed, ef, et, meas, info), remove


@pytest.mark.parametrize("request_", [[1, 3, 5, 7, 9], [9, 2, 1, 3, 5, 7]], ids=["independent", "two_rounds"])
def test_remove_vertices_rewrites_the_graph(ctx, request_):
    slam, (poses, fixed, ef, et, meas, info), _ = _ring_slam(ctx)
    n = len(poses)
    slam.setRobustKernel("Huber", 1.5, edges=[0, 4, 11])
    index_map, new_edges, skipped = slam.removeVertices(request_)
    # the reference: the same rounds on bare arrays, the old indices kept
    pe, pt, pm, pi, rskip = RN.remove_vertices(n, ef, et, meas, info, request_)
    assert skipped == [] and rskip == []
    want_map = RN.compact(n, request_)
    assert np.array_equal(index_map, want_map)
    g = slam.graph
    keep = want_map >= 0
    assert g.n_vertices == int(keep.sum()) and np.array_equal(g.ids, (100 + 7 * np.arange(n))[keep])
    assert np.array_equal(g.poses, poses[keep]) and np.array_equal(g.fixed, fixed[keep])
    assert g.lasers == {int(want_map[v]): f"laser of {v}" for v in range(n) if keep[v]}
    assert np.array_equal(g.edge_from, want_map[pe]) and np.array_equal(g.edge_to, want_map[pt])
    assert g.edge_from.dtype == np.int32 and np.all(g.edge_level == 0) and len(g.edge_level) == g.n_edges
    n_old = int((keep[ef] & keep[et]).sum())
    assert np.array_equal(new_edges, np.arange(n_old, g.n_edges)) and g.n_edges == len(pe)
    assert np.array_equal(g.meas[:n_old], pm[:n_old]) and np.array_equal(g.info[:n_old], pi[:n_old])
    d = g.meas[n_old:] - pm[n_old:]
    d[:, 2] = R.normalize_theta(d[:, 2])
    assert np.abs(d).max() <= K.MEAS_ATOL
    assert info_gap(g.info[n_old:], pi[n_old:]) <= K.INFO_MARGIN * K.INFO_GAP
    # the kernels of the old edges that stay, none on the new ones
    old_kept = np.flatnonzero(keep[ef] & keep[et])
    assert np.array_equal(slam._rk_kind[:n_old] != 0, np.isin(old_kept, [0, 4, 11])) and not slam._rk_kind[n_old:].any()
    assert len(slam._rk_kind) == g.n_edges == len(slam._rk_delta)
    if len(request_) == 6:                                         # 2 went in the second round, between 0 and 4 by then
        assert g.n_edges == 12 - 6 and sorted(zip(g.edge_from.tolist(), g.edge_to.tolist()))[0] == (0, 1)
    slam.clearRobustKernels()
    slam.optimize(5)
    want = K.optimum(poses, fixed, pe, pt, pm, pi)[keep]
    d = g.poses - want
    d[:, 2] = R.normalize_theta(d[:, 2])
    print(f"{len(request_)} removed: optimize(5) against the reference's pruned optimum {np.abs(d).max():.2e}")
    assert slam.last_status == 0 and np.abs(d).max() <= EST_ATOL


def test_remove_vertices_refuses(ctx):
    slam, (poses, fixed, ef, et, meas, info), _ = _ring_slam(ctx)
    with pytest.raises(ValueError, match="fixed"):
        slam.removeVertices([0, 3])
    with pytest.raises(ValueError, match="out of range"):
        slam.removeVertices([12])
    with pytest.raises(ValueError, match="max_degree"):
        slam.removeVertices([3], max_degree=17)
    slam.graph.add_edge(3, 8, [0.0, 0.0, 0.0], [1.0, 0, 0, 1, 0, 1], level=2)
    with pytest.raises(ValueError, match="another level"):
        slam.removeVertices([3])
    index_map, new_edges, skipped = slam.removeVertices([5], max_degree=1)   # two neighbours: left in place, flag 2
    assert skipped == [(5, 2)] and len(new_edges) == 0 and np.array_equal(index_map, np.arange(12)) and slam.graph.n_edges == 13
    index_map, new_edges, skipped = slam.removeVertices([5])
    assert skipped == [] and index_map[5] == -1 and slam.graph.n_edges == 12 and slam.graph.edge_level.tolist().count(2) == 1
    slam.graph.set_edge_mixture(0, [(1.0, meas[0], info[0]), (0.5, meas[0], info[0])])
    with pytest.raises(ValueError, match="mixture"):
        slam.removeVertices([7])
    typed = GraphSLAM(PoseGraph(np.arange(12), poses, fixed, ef, et, meas, info), ctx)
    typed.addLandmark(99, [1.0, 1.0])
    typed.addObservation(3, 12, [0.5, 0.5], [1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="pose graphs only"):
        typed.removeVertices([7])
