"""Graduated non-convexity on the robot graph, without a device: the reach predicates of tests/robot_gnc_cases.py on the float64
reference alone (tests/ref_gnc.py on ``solved_system``), the setters' refusals on a host-only graph, and the new symbols."""
import ctypes as C

import numpy as np
import pytest

import ref_gnc
import robot_gnc_cases as RC
from cg_mrslam_amd import _lib
from cg_mrslam_amd._lib import CgmrError
from cg_mrslam_amd.condensed import RobotGraph

E_INVALID, E_NO_DEVICE = -1, -2
NEW = ("cgmr_graph_set_edge_gnc", "cgmr_graph_set_received_gnc", "cgmr_graph_optimize_gnc", "cgmr_graph_gnc_weights",
       "cgmr_graph_keep_gnc_weights", "cgmr_graph_set_condensed_gnc")


def reached(nV, ef, et, root):
    """Vertices a breadth-first walk from ``root`` over the edges reaches."""
    adj = [[] for _ in range(nV)]
    for a, b in zip(ef.tolist(), et.tolist()):
        adj[a].append(b)
        adj[b].append(a)
    seen = np.zeros(nV, bool)
    seen[root] = True
    queue = [root]
    for u in queue:
        for w in adj[u]:
            if not seen[w]:
                seen[w] = True
                queue.append(w)
    return seen


@pytest.mark.parametrize("name", ["pair", "trio"])
def test_tls_reference_rejects_exactly_the_corrupted_set(name):
    c = RC.host_case(name)
    ref = RC.reference(name, "tls")
    w = ref["weights"]
    assert ref["failed"] is None and ref["outer_done"] < 100
    assert np.array_equal(np.flatnonzero(w == 0.0), c.bad) and np.all(np.delete(w, c.bad) == 1.0)
    assert np.any(c.bad >= c.n_own) and np.any(c.bad < c.n_own)                  # a rejection in either segment
    assert ref_gnc.margins(ref) > 1e-6                                           # no branch hangs on a rounding difference
    # the recipe's sizes: the second workgroup of the linearisation is partly filled
    assert c.n_own >= 257 and len(w) % 256 != 0 and len(c.poses0) >= 120
    # no corrupted edge was followed: each is wrong by more than 3 m, the estimate lies within half a metre of the truth
    d = ref["poses"] - c.truth
    assert np.abs(d[:, :2]).max() < 0.5


@pytest.mark.parametrize("name", ["pair", "trio"])
def test_every_vertex_keeps_a_full_weight_edge_and_the_kept_own_edges_connect(name):
    c = RC.host_case(name)
    s, w = c.sys, RC.reference(name, "tls")["weights"]
    nV = len(c.poses0)
    full = np.zeros(nV, bool)
    full[s["ef"][w == 1.0]] = full[s["et"][w == 1.0]] = True
    assert full.all()
    # from each gauge a condensed graph may take (any requested vertex) the kept own edges reach every vertex with an own edge
    own_ef, own_et, keep = s["ef"][:c.n_own], s["et"][:c.n_own], w[:c.n_own] > 0.0
    touched = np.zeros(nV, bool)
    touched[own_ef] = touched[own_et] = True
    index = c.rg.index
    for p in c.peers:
        assert len(c.want[p]) >= 2
        for vid in c.want[p]:
            assert np.array_equal(reached(nV, own_ef[keep], own_et[keep], index[int(vid)]), touched)
    # every peer vertex ends a true inter-robot closure among the own edges
    peer_vertices = np.flatnonzero(c.ids >= RC.PEER_BASE)
    for v in peer_vertices:
        assert np.any((own_et == v) & keep)


@pytest.mark.parametrize("name", ["pair", "trio"])
def test_gm_reference_leaves_the_corrupted_edges_below_1e_3(name):
    c = RC.host_case(name)
    ref = RC.reference(name, "gm")
    w = ref["weights"]
    assert ref["failed"] is None and np.all(w[c.bad] < 1e-3) and np.all(w > 0.0)
    assert np.array_equal(np.flatnonzero(w < 1e-3), c.bad)                       # drop_below = 1e-3 removes exactly these
    assert np.delete(w, c.bad).min() > 0.5


def test_clean_has_nothing_to_reject():
    for loss in ("tls", "gm"):
        ref = RC.reference("clean", loss)
        assert ref["nothing"] and ref["outer_done"] == 1 and np.all(ref["weights"] == 1.0)


def test_starved_reference_fails_with_both_edges_of_the_lone_vertex_at_zero():
    c = RC.host_case("starved")
    ref = RC.reference("starved", "tls")
    assert ref["failed"] is not None and ref["weights"][c.bad].tolist() == [0.0, 0.0]
    s = c.sys
    at_lone = np.flatnonzero((s["ef"] == c.lone) | (s["et"] == c.lone))
    assert np.array_equal(at_lone, c.bad) and s["fixed"][c.lone] == 0


def test_setters_refusals_and_defaults_on_a_host_only_graph():
    c = RC.build("pair")
    g = c.rg.g
    try:
        nA = c.n_own
        assert np.array_equal(g.gnc_weights(), np.ones(nA))                      # before any GNC solve
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(CgmrError) as e:
                g.set_edge_gnc(np.where(np.arange(4) == 2, bad, 5.0), first=3)
            assert e.value.code == E_INVALID, bad
        for first, n in ((0, nA + 1), (nA, 1), (nA - 1, 2), (-1, 1)):            # ranges past the own edges
            assert g.lib.cgmr_graph_set_edge_gnc(g.h, C.c_int(first), C.c_int(n), C.c_void_p(0), C.c_void_p(0)) == E_INVALID
        g.set_edge_gnc(np.full(nA, 7.0), np.zeros(nA, np.uint8))                 # ... and what is accepted
        g.set_edge_gnc(None, None, first=nA - 2, n=2)
        g.set_edge_gnc(first=nA, n=0)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(CgmrError) as e:
                g.set_received_gnc(bad)
            assert e.value.code == E_INVALID
        g.set_received_gnc(0.0)
        g.set_received_gnc(9.0, True)
        # each of the two condensed switches refuses while the other is on
        g.set_condensed_gnc(True, 1e-3)
        with pytest.raises(CgmrError) as e:
            g.set_condensed_robust(True)
        assert e.value.code == E_INVALID
        g.set_condensed_robust(False)
        g.set_condensed_gnc(False)
        g.set_condensed_robust(True)
        with pytest.raises(CgmrError) as e:
            g.set_condensed_gnc(True)
        assert e.value.code == E_INVALID
        g.set_condensed_robust(False)
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(CgmrError):
                g.set_condensed_gnc(True, bad)
        g.keep_gnc_weights(True)
        g.keep_gnc_weights(False)
        # edges appended later are default, free and of weight 1
        i0, i1 = int(c.ids[5]), int(c.ids[40])
        g.add_edges([i0], [i1], np.zeros((1, 3)), RC.INFO[None])
        assert np.array_equal(g.gnc_weights(), np.ones(nA + 1))
        # no context: the numeric call answers CGMR_E_NO_DEVICE
        with pytest.raises(CgmrError) as e:
            g.optimize_gnc()
        assert e.value.code == E_NO_DEVICE
        assert g.lib.cgmr_graph_optimize_gnc(g.h, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)) == E_NO_DEVICE
    finally:
        g.close()


def test_null_graph_is_refused():
    lib = _lib.load_library()
    null = C.c_void_p(0)
    assert lib.cgmr_graph_set_edge_gnc(null, 0, 0, null, null) == E_INVALID
    assert lib.cgmr_graph_set_received_gnc(null, C.c_double(0.0), 0) == E_INVALID
    assert lib.cgmr_graph_optimize_gnc(null, null, null, null, null, null) == E_INVALID
    assert lib.cgmr_graph_gnc_weights(null, 0, null) == E_INVALID
    assert lib.cgmr_graph_keep_gnc_weights(null, 1) == E_INVALID
    assert lib.cgmr_graph_set_condensed_gnc(null, 1, C.c_double(0.0)) == E_INVALID


def test_new_symbols_resolve():
    lib = _lib.load_library()
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SYMBOLS and hasattr(lib, name), name
    assert lib.cgmr_version() == 105                                             # additions are found by symbol


def test_python_methods_check_their_arguments():
    g = RobotGraph(None, 0, 2)
    try:
        with pytest.raises(ValueError):
            g.optimize_gnc(loss="huber")
        with pytest.raises(TypeError):
            g.optimize_gnc(kind="cauchy")
    finally:
        g.close()
