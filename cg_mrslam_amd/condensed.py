"""Multi-robot path: one robot's pose graph resident in HBM, its condensed graphs and the inter-robot exchange.

Thin host-side mirror of the reference's
  * ``CondensedGraphBuffer``  (src/mrslam/condensed_graph/condensed_graph_buffer.{h,cpp}): in-/out-closures,
    ``computeCondensedGraph``, ``insertEdgesFromRobot`` (replace-on-receive), ``getMyEdges``, ``selectGaugeCentroid``;
  * ``MRGraphSLAM::addInterRobotData``  (src/mrslam/mr_graph_slam.cpp:331-395);
  * the wire structs of ``msg_factory.h`` (44 bytes per edge, float32 on the wire, src/mrslam/msg_factory.h:78-112,200-218);
  * ``GraphComm``'s pairwise UDP send / receive (src/mrslam/graph_comm.cpp:103-208), replaced by ONE all-gather per round
    of a fixed-capacity buffer per rank over RCCL / xGMI
over the C ABI (include/cgmr.h "robot graph" and "exchange"; csrc/robot_graph.cpp, condensed_host.cpp, exchange_host.cpp, mrslam_kernels.hip, rccl_comm.cpp).
Everything here is a ctypes call; there is no numeric or bookkeeping logic in Python and no CPU fallback for the numeric
entry points (a graph created without a context only keeps the books, for CPU tests of the protocol).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CGMR_E_CHOLESKY_BASE, CgmrError, Context, load_library

WIRE_EDGE_DTYPE = np.dtype([("from", "<i4"), ("to", "<i4"), ("est", "<f4", (3,)), ("info", "<f4", (6,))])
assert WIRE_EDGE_DTYPE.itemsize == 44            # EdgeArrayMessage::ESE2Data on the wire


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else C.c_void_p(0)


class RobotGraph:
    """``cgmr_graph``: the g2o optimiser of one robot plus its ``CondensedGraphBuffer``."""

    #: edges per peer a reference message can hold: MAX_LENGTH_MSG = 100000 bytes of 44-byte edges (msg_factory.h:115).  It is
    #: the capacity of a slice (of edges, and of closure ids), not a promise that a full slice of both fits one message:
    #: 2270 edges leave room for 24 closure ids.  ``message_for`` applies the byte limit itself.
    REFERENCE_CAP_EDGES = 2270

    def __init__(self, ctx: Context | None, robot: int, n_robots: int, base_id: int = 10000, cap_edges: int = 128,
                 async_condense: bool = False):
        self.lib = ctx.lib if ctx is not None else load_library()
        self.lib.cgmr_graph_last_error.restype = C.c_char_p
        self.lib.cgmr_graph_wire_bytes.restype = C.c_int64
        self.lib.cgmr_graph_skipped_messages.restype = C.c_int64
        self.lib.cgmr_graph_failed_batches.restype = C.c_int64
        self.lib.cgmr_graph_send_buffer.restype = C.c_void_p
        self.lib.cgmr_graph_recv_buffer.restype = C.c_void_p
        self.lib.cgmr_graph_destroy.restype = None
        self.ctx, self.robot, self.n_robots, self.base_id, self.cap = ctx, robot, n_robots, base_id, cap_edges
        h = C.c_void_p()
        rc = self.lib.cgmr_graph_create(ctx.h if ctx is not None else C.c_void_p(0), C.c_int(robot), C.c_int(n_robots),
                                        C.c_int(base_id), C.c_int(cap_edges), C.byref(h))
        if rc != 0:
            raise CgmrError(rc, "cgmr_graph_create failed")
        self.h = h
        # computeCondensedGraph queues its passes on the context's side stream and returns (cgmr_graph_compute_condensed_async):
        # they run beside the next round's grow / analysis / solve; pack, the all-gather and deliver() follow them on the device
        self.async_condense = bool(async_condense) and ctx is not None
        if self.async_condense:
            self._check(self.lib.cgmr_graph_set_async(self.h, C.c_int(1)))

    def close(self):
        if getattr(self, "h", None):
            if self.ctx is not None and not getattr(self.ctx, "h", None):
                # the context was destroyed first (both in one garbage cycle, collected in any order -- after an exception, at
                # interpreter exit): cgmr_graph_destroy would use it.  The graph's device memory is left to the process's exit
                self.h = None
                return
            self.lib.cgmr_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, allow_cholesky=False):
        if rc >= 0 or (allow_cholesky and rc <= CGMR_E_CHOLESKY_BASE):
            return rc
        raise CgmrError(rc, self.lib.cgmr_graph_last_error(self.h).decode() or
                        (self.ctx.lib.cgmr_last_error(self.ctx.h).decode() if self.ctx is not None else ""))

    # ------------------------------------------------------------------ graph
    def add_vertices(self, ids, poses, fixed=None):
        ids, poses = _i32(ids), _f64(poses).reshape(-1, 3)
        fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.uint8)
        self._check(self.lib.cgmr_graph_add_vertices(self.h, C.c_int(len(ids)), _p(ids), _p(poses), _p(fx) if fx is not None else C.c_void_p(0)))

    def add_edges(self, from_ids, to_ids, meas, info):
        f, t = _i32(from_ids), _i32(to_ids)
        self._check(self.lib.cgmr_graph_add_edges(self.h, C.c_int(len(f)), _p(f), _p(t), _p(_f64(meas)), _p(_f64(info))))

    def counts(self):
        out = np.zeros(4, dtype=np.int32)
        self._check(self.lib.cgmr_graph_counts(self.h, _p(out)))
        return dict(zip(["vertices", "own_edges", "received_edges", "peers_with_requests"], out.tolist()))

    def optimize(self, iters: int):
        """``GraphSLAM::optimize(iters)``: returns (status, chi2[iters+1]); a Cholesky failure is a status, not an exception."""
        chi = np.zeros(iters + 1)
        rc = self.lib.cgmr_graph_optimize(self.h, C.c_int(iters), _p(chi))
        self._check(rc, allow_cholesky=True)
        return rc, chi

    def poses(self, first=0, n=None):
        n = self.counts()["vertices"] - first if n is None else n
        out = np.zeros((n, 3))
        self._check(self.lib.cgmr_graph_get_poses(self.h, C.c_int(first), C.c_int(n), _p(out)))
        return out

    def set_poses(self, first, poses):
        poses = _f64(poses).reshape(-1, 3)
        self._check(self.lib.cgmr_graph_set_poses(self.h, C.c_int(first), C.c_int(len(poses)), _p(poses)))

    # ------------------------------------------------------------------ closures / condensed graphs
    def insertInClosure(self, peer, ids):   # noqa: N802
        ids = _i32(ids)
        self._check(self.lib.cgmr_graph_insert_in_closure(self.h, C.c_int(peer), C.c_int(len(ids)), _p(ids)))

    def insertOutClosure(self, peer, ids):   # noqa: N802
        ids = _i32(ids)
        self._check(self.lib.cgmr_graph_insert_out_closure(self.h, C.c_int(peer), C.c_int(len(ids)), _p(ids)))

    def closures(self, peer, which="out"):
        out = np.zeros(4096, dtype=np.int32)
        n = self._check(self.lib.cgmr_graph_closures(self.h, C.c_int(peer), C.c_int(0 if which == "out" else 1), C.c_int(len(out)), _p(out)))
        return out[:n].copy()

    def set_algorithm(self, algorithm: str = "gn", **params):
        """The optimiser of ``optimize``: "gn" (default, the reference's Gauss-Newton), "levenberg" with g2o's
        Levenberg-Marquardt parameters (tau, initial_lambda, max_trials, good_step_lower, good_step_upper) or "dl" (g2o's
        dogleg) with its parameters (initial_delta, max_trials, initial_lambda, lambda_factor; checked here, ValueError)."""
        from ._lib import dl_params_checked, lm_params
        if algorithm not in ("gn", "levenberg", "dl"):
            raise ValueError(f"algorithm must be 'gn', 'levenberg' or 'dl', not {algorithm!r}")
        if algorithm == "gn":
            self._check(self.lib.cgmr_graph_set_algorithm(self.h, C.c_int(0), C.c_void_p(0)))
        elif algorithm == "dl":
            prm = dl_params_checked(params)
            self._check(self.lib.cgmr_graph_set_dogleg_params(self.h, C.byref(prm)))
            self._check(self.lib.cgmr_graph_set_algorithm(self.h, C.c_int(2), C.c_void_p(0)))
        else:
            prm = lm_params(**params)
            self._check(self.lib.cgmr_graph_set_algorithm(self.h, C.c_int(1), C.byref(prm)))

    def set_edge_robust(self, kind, delta=1.0, first: int = 0, n: int | None = None):
        """Robust kernels of own edges [first, first + n) by insertion index (n None: to the last one): ``kind`` a name or
        code, or an array of either, one per edge; ``delta`` a scalar or array.  Edges added later take none.  Names and
        deltas are checked here (ValueError) before the library sees them."""
        from ._lib import robust_arrays
        if n is None:
            n = self.counts()["own_edges"] - first if np.ndim(kind) == 0 else len(kind)
        codes, deltas, code0, delta0 = robust_arrays(kind, delta, n)
        codes = np.full(n, code0, dtype=np.uint8) if codes is None else codes
        deltas = np.full(n, delta0) if deltas is None else deltas
        deltas = np.where(codes == 0, 1.0, deltas)
        self._check(self.lib.cgmr_graph_set_edge_robust(self.h, C.c_int(first), C.c_int(n), _p(codes), _p(deltas)))

    def set_received_robust(self, kind, delta: float = 1.0):
        """One robust kernel for every edge received from the peers (default: none)."""
        from ._lib import robust_arrays
        _, _, code, d = robust_arrays(kind, delta, 1)
        self._check(self.lib.cgmr_graph_set_received_robust(self.h, C.c_int(code), C.c_double(d if code else 1.0)))

    def set_condensed_robust(self, on: bool):
        """Build every condensed graph with the own edges' robust kernels (set_edge_robust), rho1 taken at each graph's
        spanning-tree guess (cgmr_graph_set_condensed_robust; default off: the plain condensed graphs, byte for byte)."""
        self._check(self.lib.cgmr_graph_set_condensed_robust(self.h, C.c_int(1 if on else 0)))

    def edge_stats(self):
        """(e2, weights) of every level-0 edge at the estimate of the last optimize, own edges first, then the received ones
        (debug_edges order); None when that solve ran with no kernel set."""
        n = self._check(self.lib.cgmr_graph_edge_stats(self.h, C.c_int(0), C.c_void_p(0), C.c_void_p(0)))
        if n == 0:
            return None
        e2, w = np.zeros(n), np.zeros(n)
        self._check(self.lib.cgmr_graph_edge_stats(self.h, C.c_int(n), _p(e2), _p(w)))
        return e2, w

    # ------------------------------------------------------------------ graduated non-convexity
    def set_edge_gnc(self, barc_sq=None, known_inliers=None, first: int = 0, n: int | None = None):
        """GNC parameters of own edges [first, first + n) by insertion index (n None: to the last one, or the length of an
        array given): ``barc_sq`` a scalar, an array or None (the default: the chi2 0.99 quantile, or the call's
        ``default_barc_sq``); ``known_inliers`` a mask of length n, a list of indices into the range, or None (all free).
        Edges added later are default and free."""
        from ._lib import gnc_known_mask
        if n is None:
            if barc_sq is not None and np.ndim(barc_sq) == 1:
                n = len(barc_sq)
            elif known_inliers is not None and np.asarray(known_inliers).dtype in (np.bool_, np.uint8):
                n = len(known_inliers)
            else:
                n = self.counts()["own_edges"] - first
        c = None if barc_sq is None else np.ascontiguousarray(np.broadcast_to(np.asarray(barc_sq, dtype=np.float64), (n,)))
        k = None if known_inliers is None else gnc_known_mask(known_inliers, n)
        self._check(self.lib.cgmr_graph_set_edge_gnc(self.h, C.c_int(first), C.c_int(n), _p(c) if c is not None else C.c_void_p(0),
                                                     _p(k) if k is not None else C.c_void_p(0)))

    def set_received_gnc(self, barc_sq: float = 0.0, known_inlier: bool = False):
        """One GNC class for every edge received from the peers: ``barc_sq`` (0: the default), known inlier or free."""
        self._check(self.lib.cgmr_graph_set_received_gnc(self.h, C.c_double(float(barc_sq)), C.c_int(1 if known_inlier else 0)))

    def optimize_gnc(self, loss="tls", max_outer: int = 100, default_barc_sq: float = 0.0, raise_on_cholesky: bool = True, **params):
        """Graduated non-convexity on the system ``optimize`` would solve now (cgmr_graph_optimize_gnc): ``loss`` "tls" or "gm";
        ``params``: mu_factor, inner_iters, outer_per_wait.  Returns a dict shaped like ``Context.gnc_optimize``'s: status, mu
        [max_outer], cost [max_outer + 1], partial [max_outer], outer_done, weights and edge_chi2 of every edge (own edges, then
        the received ones).  The own edges' weights stay with the graph (``gnc_weights``)."""
        from ._lib import GNC_DEFAULTS, GncParams, gnc_loss_code
        bad = set(params) - set(GNC_DEFAULTS)
        if bad:
            raise TypeError(f"unknown GNC parameter(s): {sorted(bad)}")
        v = dict(GNC_DEFAULTS, **params)
        mo = max(int(max_outer), 1)
        mu, cost, partial, done = np.zeros(mo), np.zeros(mo + 1), np.zeros(mo, dtype=np.int32), C.c_int32(0)
        prm = GncParams(gnc_loss_code(loss), float(v["mu_factor"]), int(max_outer), int(v["inner_iters"]), int(v["outer_per_wait"]),
                        None, float(default_barc_sq), None, None, None)
        rc = self.lib.cgmr_graph_optimize_gnc(self.h, C.byref(prm), _p(mu), _p(cost), _p(partial), C.byref(done))
        self._check(rc, allow_cholesky=not raise_on_cholesky)
        st = self.edge_stats()
        e2, w = st if st is not None else (np.zeros(0), np.zeros(0))
        return dict(status=rc, mu=mu, cost=cost, partial=partial, outer_done=int(done.value), weights=w, edge_chi2=e2)

    def gnc_weights(self):
        """The stored GNC weight of every own edge: 1 before any ``optimize_gnc`` and for edges added since the last one."""
        n = self._check(self.lib.cgmr_graph_gnc_weights(self.h, C.c_int(0), C.c_void_p(0)))
        w = np.zeros(n)
        if n:
            self._check(self.lib.cgmr_graph_gnc_weights(self.h, C.c_int(n), _p(w)))
        return w

    def keep_gnc_weights(self, on: bool):
        """``optimize`` (Gauss-Newton) scales every own edge by its stored GNC weight (cgmr_graph_keep_gnc_weights; default off)."""
        self._check(self.lib.cgmr_graph_keep_gnc_weights(self.h, C.c_int(1 if on else 0)))

    def set_condensed_gnc(self, on: bool, drop_below: float = 0.0):
        """Build every condensed graph without the own edges of stored weight 0 or below ``drop_below``, the others scaled by
        their weight (cgmr_graph_set_condensed_gnc; default off: the plain condensed graphs, byte for byte)."""
        self._check(self.lib.cgmr_graph_set_condensed_gnc(self.h, C.c_int(1 if on else 0), C.c_double(float(drop_below))))

    def lm_last(self):
        """Records of the last Levenberg-Marquardt solve: (lambdas, trials), one entry per iteration run."""
        n = self._check(self.lib.cgmr_graph_lm_last(self.h, C.c_int(0), C.c_void_p(0), C.c_void_p(0)))
        lam = np.zeros(n)
        tri = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.lib.cgmr_graph_lm_last(self.h, C.c_int(n), _p(lam), _p(tri)))
        return lam, tri

    def dl_last(self):
        """Records of the last dogleg solve: (deltas, trials, steps), one entry per iteration run."""
        n = self._check(self.lib.cgmr_graph_dl_last(self.h, C.c_int(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)))
        dlt = np.zeros(n)
        tri = np.zeros(n, dtype=np.int32)
        stp = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.lib.cgmr_graph_dl_last(self.h, C.c_int(n), _p(dlt), _p(tri), _p(stp)))
        return dlt, tri, stp

    def set_optimal_gauge(self, optimal: bool):
        """``computeCondensedGraph(robot, optimal)``: selectOptimalGauge instead of selectGaugeCentroid (reference default: off)."""
        self._check(self.lib.cgmr_graph_set_optimal_gauge(self.h, C.c_int(1 if optimal else 0)))

    def computeCondensedGraph(self, peer: int = -1):   # noqa: N802
        """``computeCondensedGraph`` for one peer or (``peer < 0``) for every peer that has asked; returns the number built."""
        if self.async_condense:
            return self._check(self.lib.cgmr_graph_compute_condensed_async(self.h, C.c_int(peer)))
        return self._check(self.lib.cgmr_graph_compute_condensed(self.h, C.c_int(peer)))

    def condensed_wait(self):
        """Wait for the passes ``computeCondensedGraph`` queued (``async_condense``); raises if one of them failed."""
        self._check(self.lib.cgmr_graph_condensed_wait(self.h))

    def deliver(self, dst: "RobotGraph"):
        """My packed message (``pack()`` first) into ``dst``'s receive buffer, on the device (robots sharing a GPU)."""
        self._check(self.lib.cgmr_graph_deliver(self.h, dst.h))

    def condensed(self, peer):
        """(gauge id, to ids[n], est[n,3], info_upper[n,6]) of the condensed graph built for ``peer``, double precision."""
        cap = self.cap
        gid = C.c_int32(-1)
        to, est, iu = np.zeros(cap, dtype=np.int32), np.zeros((cap, 3)), np.zeros((cap, 6))
        n = self._check(self.lib.cgmr_graph_get_condensed(self.h, C.c_int(peer), C.c_int(cap), C.byref(gid), _p(to), _p(est), _p(iu)))
        return (int(gid.value) if n else None), to[:n].astype(np.int64), est[:n].copy(), iu[:n].copy()

    def set_condensed(self, peer, from_id, to_ids, est, info):
        to = _i32(to_ids)
        e = np.ascontiguousarray(est, dtype=np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(info, dtype=np.float32).reshape(-1, 6)
        self._check(self.lib.cgmr_graph_set_condensed(self.h, C.c_int(peer), C.c_int(len(to)), C.c_int32(int(from_id)), _p(to), _p(e), _p(i)))

    # ------------------------------------------------------------------ wire
    def skipped_messages(self) -> int:
        """Messages left out, not built or dropped because they exceed ``cap_edges`` (the reference skips a send whose
        ``toCharArray`` does not fit ``MAX_LENGTH_MSG``, graph_comm.cpp:112-122)."""
        return int(self.lib.cgmr_graph_skipped_messages(self.h))

    def failed_batches(self) -> int:
        """Asynchronous batches of condensed graphs that failed (Cholesky / a bounded device-side wait): their peers got no edges
        in that round's message; the later rounds are built regardless."""
        return int(self.lib.cgmr_graph_failed_batches(self.h))

    def wire_bytes(self) -> int:
        return int(self.lib.cgmr_graph_wire_bytes(self.h))

    def send_buffer(self) -> int:
        return int(self.lib.cgmr_graph_send_buffer(self.h) or 0)

    def recv_buffer(self) -> int:
        return int(self.lib.cgmr_graph_recv_buffer(self.h) or 0)

    def pack(self, d_send: int = 0):
        self._check(self.lib.cgmr_graph_pack(self.h, C.c_void_p(d_send)))

    def ingest(self, d_recv: int = 0):
        n = np.zeros(self.n_robots, dtype=np.int32)
        self._check(self.lib.cgmr_graph_ingest(self.h, C.c_void_p(d_recv), _p(n)))
        return n

    def ingest_delivered(self):
        """The ingest that goes with ``deliver``: the k-th call digests the k-th message of every peer."""
        n = np.zeros(self.n_robots, dtype=np.int32)
        self._check(self.lib.cgmr_graph_ingest_delivered(self.h, _p(n)))
        return n

    def pack_host(self) -> np.ndarray:
        buf = np.zeros(self.wire_bytes(), dtype=np.uint8)
        self._check(self.lib.cgmr_graph_pack_host(self.h, _p(buf)))
        return buf

    def ingest_host(self, recv) -> np.ndarray:
        recv = np.ascontiguousarray(recv, dtype=np.uint8).reshape(-1)
        if recv.size != self.n_robots * self.wire_bytes():
            raise ValueError("receive buffer must hold n_robots wire buffers")
        n = np.zeros(self.n_robots, dtype=np.int32)
        self._check(self.lib.cgmr_graph_ingest_host(self.h, _p(recv), _p(n)))
        return n

    def message_for(self, peer):
        """``constructCondensedGraphMessage(peer)``: a ``messages.CondensedGraphMessage`` or None (nothing to send).  A message
        beyond the slice capacity or beyond ``MAX_LENGTH_MSG`` bytes is not sent: None, and one more ``skipped_messages()`` --
        what comes back always has a ``to_bytes()``."""
        from .messages import EDGE_DTYPE, CondensedGraphMessage
        cap = self.cap
        edges, clos = np.empty(cap, dtype=EDGE_DTYPE), np.empty(cap, dtype=np.int32)
        ne, nc = C.c_int32(0), C.c_int32(0)
        rc = self._check(self.lib.cgmr_graph_message_for(self.h, C.c_int(peer), C.c_int(cap), _p(edges), C.byref(ne), C.c_int(cap),
                                                         _p(clos), C.byref(nc)))
        return CondensedGraphMessage(self.robot, edges[:ne.value].copy(), clos[:nc.value].copy()) if rc == 1 else None

    def message_from(self, msg) -> int:
        """``addInterRobotData(CondensedGraphMessage*)``: returns the number of edges now held from the sender because of
        this message (0 = the previous set stays)."""
        e = np.ascontiguousarray(msg.edges)
        c = _i32(msg.closures)
        n = C.c_int32(0)
        self._check(self.lib.cgmr_graph_message_from(self.h, C.c_int(msg.robotId), C.c_int(len(e)), _p(e), C.c_int(len(c)), _p(c), C.byref(n)))
        return int(n.value)

    def received_edges(self, peer):
        n = self.counts_received(peer)
        if n == 0:
            return (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros((0, 6)))
        f, t, m, i = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty((n, 3)), np.empty((n, 6))
        n = self._check(self.lib.cgmr_graph_received_edges(self.h, C.c_int(peer), C.c_int(n), _p(f), _p(t), _p(m), _p(i)))
        return f[:n].astype(np.int64), t[:n].astype(np.int64), m[:n], i[:n]

    def debug_received_segment(self):
        """Test support: (meas[n,3], info[n,6]) of the received edges as the solver reads them (the compact second edge segment),
        peer order; ``received_edges`` reads the staging."""
        n = self._check(self.lib.cgmr_graph_debug_received_segment(self.h, C.c_int(0), None, None))
        m, i = np.zeros((n, 3)), np.zeros((n, 6))
        self._check(self.lib.cgmr_graph_debug_received_segment(self.h, C.c_int(n), _p(m), _p(i)))
        return m, i

    def counts_received(self, peer):
        """Edges currently held from ``peer`` (no data moved)."""
        return int(self._check(self.lib.cgmr_graph_received_edges(self.h, C.c_int(peer), C.c_int(0), None, None, None, None)))

    def last_seconds(self):
        out = np.zeros(2)
        self._check(self.lib.cgmr_graph_last_seconds(self.h, _p(out)))
        return {"optimize": float(out[0]), "condense": float(out[1])}


def wire_narrow_edges(ctx: Context, from_id, to_vertex, vertex_ids, est, info):
    """Test support (``cgmr_wire_narrow_edges``): the device's double -> float32 wire records of host data, [n] WIRE_EDGE_DTYPE."""
    to, ids, e, i = _i32(to_vertex), _i32(vertex_ids), _f64(est).reshape(-1, 3), _f64(info).reshape(-1, 6)
    out = np.zeros(len(to), dtype=WIRE_EDGE_DTYPE)
    ctx._check(ctx.lib.cgmr_wire_narrow_edges(ctx.h, C.c_int(len(to)), C.c_int32(int(from_id)), _p(to), C.c_int(len(ids)), _p(ids), _p(e),
                                              _p(i), _p(out)))
    return out


def wire_narrow_edges_batched(ctx: Context, nq, gauge_id, out_slot, strides, to_vertex, vertex_ids, est, info, wire):
    """Test support (``cgmr_wire_narrow_edges_batched``): one batched launch.  ``strides`` = (marg, est, info, wire) in bytes;
    ``to_vertex`` / ``est`` / ``info`` / ``wire`` are uint8 buffers laid out by those strides (include/cgmr.h); returns the wire
    buffer as the device left it."""
    nq, gid, slot, ids = _i32(nq), _i32(gauge_id), _i32(out_slot), _i32(vertex_ids)
    bufs = [np.ascontiguousarray(b, dtype=np.uint8).reshape(-1) for b in (to_vertex, est, info, wire)]
    n_slots = len(bufs[3]) // int(strides[3])
    if len(bufs[0]) != len(nq) * strides[0] or any(len(b) != n_slots * s for b, s in zip(bufs[1:], strides[1:])):
        raise ValueError("buffers must hold njobs * marg_stride and n_slots * stride bytes")
    out = bufs[3].copy()
    ctx._check(ctx.lib.cgmr_wire_narrow_edges_batched(ctx.h, C.c_int(len(nq)), _p(nq), _p(gid), _p(slot), C.c_int(n_slots),
                                                      *(C.c_longlong(int(s)) for s in strides), _p(bufs[0]), C.c_int(len(ids)), _p(ids),
                                                      _p(bufs[1]), _p(bufs[2]), _p(out)))
    return out


def unpack_wire(buf: np.ndarray, n_robots: int, cap: int):
    """Decode one rank's wire buffer (tests, debugging): (robot, n_edges[R], n_closures[R], edges[R][cap], closures[R][cap])."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    hdr = buf[:4 * (2 + 2 * n_robots)].view(np.int32)
    o = 4 * (2 + 2 * n_robots)
    edges = buf[o:o + n_robots * cap * 44].view(WIRE_EDGE_DTYPE).reshape(n_robots, cap)
    o += n_robots * cap * 44
    clos = buf[o:o + n_robots * cap * 4].view(np.int32).reshape(n_robots, cap)
    return int(hdr[0]), hdr[2:2 + n_robots].copy(), hdr[2 + n_robots:2 + 2 * n_robots].copy(), edges, clos


class Exchange:
    """One all-gather per round of every rank's wire buffer.

    transport "rccl":  ``cgmr_allgather_condensed`` on device buffers, a native RCCL communicator on a side stream (the
                       unique id travels through ``torch.distributed``); overlaps with whatever the context's stream does next
    transport "torch": ``torch.distributed.all_gather_into_tensor`` on the same device buffers (backend nccl = RCCL)
    transport "host":  host staging (backend gloo: CPU tests, single-GPU dry runs)
    ``start()`` issues the collective, ``finish()`` ingests what arrived; in between the caller runs the next solve."""

    def __init__(self, graph: RobotGraph, transport: str = "auto", group=None):
        import torch
        import torch.distributed as dist
        self.g, self.group, self.torch, self.dist = graph, group, torch, dist
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        if self.world != graph.n_robots:
            raise ValueError("one rank per robot: world size must equal n_robots")
        self.wb = graph.wire_bytes()
        backend = dist.get_backend(group) if dist.is_initialized() else "none"
        if transport == "auto":
            transport = "rccl" if (backend == "nccl" and graph.ctx is not None) else ("host" if backend in ("gloo", "none") else "torch")
        self.comm = None
        self.pending = None
        self.fallback_reason = None
        if transport == "rccl":
            try:
                self._init_rccl()
            except Exception as e:          # noqa: BLE001 -- any failure: fall back to torch's own RCCL communicator
                self.fallback_reason = f"{type(e).__name__}: {e}"
                transport = "torch"
            # all ranks must agree on the transport
            flag = torch.tensor([1 if transport == "rccl" else 0], device=torch.device("cuda", graph.ctx.device))
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
            if int(flag.item()) == 0 and transport == "rccl":
                self._destroy_comm()
                transport = "torch"
                self.fallback_reason = "a peer could not create the RCCL communicator"
        self.transport = transport
        if transport == "torch":
            dev = torch.device("cuda", graph.ctx.device)
            graph.lib.cgmr_ctx_stream.restype = C.c_void_p
            # the context's stream as a torch stream: the two are ordered with events, the host never waits
            self.ctx_stream = torch.cuda.ExternalStream(int(graph.lib.cgmr_ctx_stream(graph.ctx.h) or 0), device=dev)
            self.t_send = torch.zeros(self.wb, dtype=torch.uint8, device=dev)
            self.t_recv = torch.zeros(self.world * self.wb, dtype=torch.uint8, device=dev)

    def _init_rccl(self):
        """Native RCCL communicator next to torch's.  Two guards against a hang (a rank that fails BEFORE the collective
        ``ncclCommInitRank`` would leave the others inside it): every rank first probes librccl locally and the ranks agree
        (MIN all-reduce) that all of them can go on; the collective initialisation itself runs under a timeout
        (``CGMR_RCCL_INIT_TIMEOUT`` seconds, default 60) and a rank that runs out of time falls back to the torch
        transport -- its peers, stuck in the same collective, time out the same way and the agreement in ``__init__``
        settles on "torch" for everybody."""
        import os
        import threading
        torch, dist, g = self.torch, self.dist, self.g
        lib = g.lib
        dev = torch.device("cuda", g.ctx.device)
        h = np.zeros(128, dtype=np.uint8)
        # rank 0 asks librccl for the id; the others only check that the library resolves (ncclGetUniqueId starts a bootstrap
        # listener: one per rank that nothing ever uses otherwise)
        ok_local = lib.cgmr_comm_unique_id(_p(h)) if dist.get_rank(self.group) == 0 else lib.cgmr_comm_probe()
        flag = torch.tensor([1 if ok_local == 0 else 0], device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
        if int(flag.item()) == 0:
            raise CgmrError(ok_local or -1, "librccl is not loadable on every rank")
        uid = torch.from_numpy(h).to(dev)
        dist.broadcast(uid, src=0, group=self.group)
        h = np.ascontiguousarray(uid.cpu().numpy())
        comm = C.c_void_p()
        res = {}

        def create():
            res["rc"] = lib.cgmr_comm_create(g.ctx.h, C.c_int(self.world), C.c_int(dist.get_rank(self.group)), _p(h), C.byref(comm))

        t = threading.Thread(target=create, daemon=True)
        t.start()
        t.join(float(os.environ.get("CGMR_RCCL_INIT_TIMEOUT", "60")))
        if t.is_alive():
            # the thread may still come back with a communicator: close() then takes care of it; until it has, the context is
            # shared with a thread inside ncclCommInitRank, which touches the device but none of the context's buffers
            self._late_init = (t, comm, res)
            raise TimeoutError("ncclCommInitRank did not return (native RCCL communicator); using torch.distributed instead")
        if res.get("rc", -1) != 0:
            raise CgmrError(res.get("rc", -1), g.ctx.lib.cgmr_last_error(g.ctx.h).decode())
        self.comm = comm

    def diagnostics(self) -> dict:
        """What this rank's exchange runs on, for a multi-GPU run's own report: the transport, why it is not the native one (if so),
        and how many ranks the native communicator itself reports (``ncclCommCount``)."""
        d = {"transport": self.transport, "transport_fallback_reason": self.fallback_reason, "world": self.world,
             "native_comm_ranks": None, "native_comm_rank": None}
        if self.transport == "rccl" and self.comm is not None:
            out = np.zeros(3, dtype=np.int32)
            if self.g.lib.cgmr_comm_info(self.comm, _p(out)) == 0:
                d["native_comm_ranks"], d["native_comm_rank"] = int(out[0]), int(out[1])
                d["native_comm_answered_by_librccl"] = bool(out[2])
        return d

    def _destroy_comm(self):
        if self.comm is not None:
            self.g.lib.cgmr_comm_destroy.restype = None
            self.g.lib.cgmr_comm_destroy(self.comm)
            self.comm = None

    def close(self):
        late = getattr(self, "_late_init", None)
        if late is not None:                                  # a collective initialisation that outlived its time-out
            t, comm, res = late
            t.join(5.0)
            if not t.is_alive() and res.get("rc", -1) == 0 and comm:
                self.g.lib.cgmr_comm_destroy.restype = None
                self.g.lib.cgmr_comm_destroy(comm)
            self._late_init = None
        self._destroy_comm()

    def start(self):
        """Serialise my message and issue the all-gather; returns immediately for the device transports."""
        g = self.g
        if self.world == 1:
            self.pending = None
            return
        if self.transport == "rccl":
            g.pack(0)
            g.ctx._check(g.lib.cgmr_allgather_condensed(g.ctx.h, self.comm, C.c_void_p(g.send_buffer()), C.c_size_t(self.wb),
                                                        C.c_void_p(g.recv_buffer())))
            self.pending = "rccl"
        elif self.transport == "torch":
            g.pack(self.t_send.data_ptr())
            g.ctx._check(g.lib.cgmr_ctx_join_side(g.ctx.h))     # (a batch queued on the context's side stream: the packed message sits behind it)
            # the context's stream is not torch's: torch's stream waits (on the device) for the packed message, the
            # collective then overlaps with whatever the context's stream does next -- as on the native transport
            self.torch.cuda.current_stream(self.t_send.device).wait_stream(self.ctx_stream)
            self.pending = self.dist.all_gather_into_tensor(self.t_recv, self.t_send, group=self.group, async_op=True)
        else:
            send = self.torch.from_numpy(g.pack_host())
            recv = self.torch.empty(self.world * self.wb, dtype=self.torch.uint8)
            self.pending = (self.dist.all_gather_into_tensor(recv, send, group=self.group, async_op=True), recv, send)

    def finish(self):
        """Wait for the all-gather issued by ``start()`` and ingest it.  Returns accepted edges per sender (or None)."""
        g = self.g
        if self.pending is None:
            return None
        if self.transport == "rccl":
            g.ctx._check(g.lib.cgmr_comm_wait(g.ctx.h, self.comm))
            n = g.ingest(0)
        elif self.transport == "torch":
            self.pending.wait()                                                   # torch's stream waits for the collective ...
            self.ctx_stream.wait_stream(self.torch.cuda.current_stream(self.t_recv.device))   # ... and the context's stream for torch's
            n = g.ingest(self.t_recv.data_ptr())
        else:
            work, recv, _send = self.pending
            work.wait()
            n = g.ingest_host(recv.numpy())
        self.pending = None
        return n

    def last_collective_seconds(self):
        if self.transport != "rccl" or self.comm is None:
            return None
        s = C.c_double()
        if self.g.lib.cgmr_comm_last_seconds(self.comm, C.byref(s)) != 0:
            return None
        return s.value
