"""The bad calls of tests/test_error_texts_gpu.py and tools/make_error_texts_golden.py: every solver entry-point family of the
C ABI, in each of its variants, on a 4-vertex, 4-edge square with one listed input made bad -- where that input applies to the
entry point.  Every call goes to the library through ctypes as a C caller would make it (the binding's own checks would stop
most of them first) and must be refused by a host-side check before anything is launched.

Left out, because on the recorded library the input is not refused before it is used:
  * an edge index equal to nV with cgmr_covariance_estimate* / cgmr_condense*: their spanning-tree guess walks the edge list on
    the host before the structure check looks at it;
and cgmr_max_clique_greedy takes none of the listed inputs (no measurement, kernel, kind, edge, query or iteration count).

run_all(lib, ctx_handle) -> {case id: [return code, cgmr_last_error text]}
"""
import ctypes as C
import math

import numpy as np

from cg_mrslam_amd._lib import DlParams, FactorTypes, GncParams, LmParams, Mixture, Robust

NV, NE = 4, 4
BAD_INPUTS = ("meas_null", "robust_kind_9", "vertex_kind_2", "edge_index_nV", "query_index_nV", "gauge_index_nV", "iters_minus_1")


def _p(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


class _Square:
    """The arrays of one call; ``bad`` names the input spoiled.  With ``dev`` poses / meas / info live in device memory."""

    def __init__(self, bad, dev):
        self.keep = []
        self.poses = np.array([[0, 0, 0], [1, 0, 0], [1, 1, math.pi / 2], [0, 1, math.pi]], dtype=np.float64)
        self.fixed = np.array([1, 0, 0, 0], dtype=np.uint8)
        self.ef = np.array([0, 1, 2, 3], dtype=np.int32)
        self.et = np.array([1, 2, 3, 0], dtype=np.int32)
        if bad == "edge_index_nV":
            self.et[2] = NV
        self.meas = np.tile(np.array([1.0, 0.0, math.pi / 2]), (NE, 1))
        self.info = np.tile(np.array([10.0, 0, 0, 10.0, 0, 20.0]), (NE, 1))
        if dev:
            import torch
            t = [torch.from_numpy(a).to("cuda:0") for a in (self.poses, self.meas, self.info)]
            torch.cuda.synchronize()
            self.keep += t
            ptrs = [C.c_void_p(x.data_ptr()) for x in t]
        else:
            ptrs = [_p(self.poses), _p(self.meas), _p(self.info)]
        if bad == "meas_null":
            ptrs[1] = C.c_void_p(0)
        self.p_poses, self.p_meas, self.p_info = ptrs
        # the optional descriptions: valid unless they are what is spoiled
        self.vk = np.zeros(NV, dtype=np.uint8)
        self.ek = np.zeros(NE, dtype=np.uint8)
        if bad == "vertex_kind_2":
            self.vk[1] = 2
        self.ft = FactorTypes(self.vk.ctypes.data, self.ek.ctypes.data)
        self.rk = Robust(0, 0, 9 if bad == "robust_kind_9" else 3, 1.0, 0, 0)
        self.cptr = np.arange(NE + 1, dtype=np.int32)                 # one component per edge
        self.cw = np.ones(NE)
        self.mix = Mixture(self.cptr.ctypes.data, self.meas.ctypes.data, self.info.ctypes.data, self.cw.ctypes.data, 0)
        self.iters = -1 if bad == "iters_minus_1" else 2
        q = NV if bad == "query_index_nV" else 2
        self.query = np.array([1, q], dtype=np.int32)
        self.pair_b = np.array([3, 1], dtype=np.int32)
        self.gauge = NV if bad == "gauge_index_nV" else 0
        self.obs_kind = np.zeros(2, dtype=np.uint8)
        self.cl_meas = np.tile(np.array([0.0, 1.0, 0.0]), (2, 1))
        self.cl_info = np.tile(np.array([10.0, 0, 0, 10.0, 0, 20.0]), (2, 1))
        self.out = np.zeros(256)                                       # any output: no call gets as far as writing one
        self.outi = np.zeros(64, dtype=np.int32)

    def problem(self, with_fixed=True):
        head = [C.c_int(NV), self.p_poses] + ([_p(self.fixed)] if with_fixed else [])
        return head + [C.c_int(NE), _p(self.ef), _p(self.et), self.p_meas, self.p_info]


def _entries():
    """(entry point [#variant], dev, the inputs that apply beside meas_null, arguments behind the problem's) for every variant."""
    E = []
    o, oi = (lambda s: _p(s.out)), (lambda s: _p(s.outi))
    rk, ft, mix = (lambda s: C.byref(s.rk)), (lambda s: C.byref(s.ft)), (lambda s: C.byref(s.mix))
    gnc = GncParams(0, 1.4, 20, 1, 8, 0, 0.0, 0, 0, 0)
    variants = (("", (), ()), ("_robust", ("robust_kind_9",), (rk,)), ("_typed", ("robust_kind_9", "vertex_kind_2"), (ft, rk)),
                ("_mixture", ("vertex_kind_2",), (ft, mix)))
    for alg, mid in (("gn", lambda s: [C.c_int(s.iters), o(s)]),
                     ("lm", lambda s: [C.c_int(s.iters), C.byref(LmParams(1e-5, -1.0, 10, 1 / 3, 2 / 3)), o(s), o(s), oi(s), oi(s)]),
                     ("dl", lambda s: [C.c_int(s.iters), C.byref(DlParams(1e4, 100, 1e-7, 10.0)), o(s), o(s), oi(s), oi(s), oi(s)])):
        for sfx, applies, tail in variants:
            if alg == "dl" and sfx == "_robust":
                continue                                               # (dogleg's plain entry points take the kernel themselves)
            if alg == "dl" and sfx == "":
                applies, tail = ("robust_kind_9",), (rk,)
            for dev in (False, True):
                E.append((f"cgmr_{alg}_optimize{sfx}{'_dev' if dev else ''}", dev, applies + ("edge_index_nV", "iters_minus_1"),
                          lambda s, mid=mid, tail=tail: mid(s) + [t(s) for t in tail]))
    for dev in (False, True):
        d = "_dev" if dev else ""
        E.append((f"cgmr_gnc_optimize{d}", dev, ("vertex_kind_2", "edge_index_nV"),
                  lambda s: [ft(s), C.byref(gnc), o(s), o(s), oi(s), oi(s)]))
        E.append((f"cgmr_gnc_optimize{d}#no_types", dev, ("edge_index_nV",),         # (the plain form: a null cgmr_factor_types)
                  lambda s: [C.c_void_p(0), C.byref(gnc), o(s), o(s), oi(s), oi(s)]))
        E.append((f"cgmr_chordal_initialize{d}", dev, ("edge_index_nV",), lambda s: [C.c_int(3), o(s), oi(s)]))
        E.append((f"cgmr_chordal_initialize_typed{d}", dev, ("vertex_kind_2", "edge_index_nV"), lambda s: [C.c_int(3), o(s), oi(s), ft(s)]))
    E.append(("cgmr_mixture_select", False, ("vertex_kind_2", "edge_index_nV"), lambda s: [ft(s), mix(s), o(s)]))
    marg = (("", (), ()), ("_robust", ("robust_kind_9",), (rk,)), ("_typed", ("robust_kind_9", "vertex_kind_2"), (ft, rk)))
    for sfx, applies, tail in marg:
        E.append((f"cgmr_marginals{sfx}", False, applies + ("edge_index_nV", "query_index_nV"),
                  lambda s, tail=tail: [C.c_int(2), _p(s.query), o(s)] + [t(s) for t in tail]))
        E.append((f"cgmr_marginals_all{sfx}", False, applies + ("edge_index_nV",), lambda s, tail=tail: [o(s), o(s)] + [t(s) for t in tail]))
    for sfx, applies, tail in marg[:2]:
        E.append((f"cgmr_covariance_estimate{sfx}", False, applies + ("query_index_nV", "gauge_index_nV"),
                  lambda s, tail=tail: [C.c_int(s.gauge), C.c_int(2), _p(s.query), o(s)] + [t(s) for t in tail]))
        E.append((f"cgmr_condense{sfx}", False, applies + ("query_index_nV", "gauge_index_nV"),
                  lambda s, tail=tail: [C.c_int(s.gauge), C.c_int(2), _p(s.query), oi(s), o(s), o(s), o(s)] + [t(s) for t in tail]))
    for sfx, applies, tail in (("", ("robust_kind_9",), (rk,)), ("_typed", ("robust_kind_9", "vertex_kind_2"), (ft, rk))):
        E.append((f"cgmr_marginals_joint{sfx}", False, applies + ("edge_index_nV", "query_index_nV"),
                  lambda s, tail=tail: [C.c_int(2), _p(s.query), o(s)] + [t(s) for t in tail]))
        E.append((f"cgmr_marginals_pairs{sfx}", False, applies + ("edge_index_nV", "query_index_nV"),
                  lambda s, tail=tail: [C.c_int(2), _p(s.query), _p(s.pair_b), o(s), o(s), o(s)] + [t(s) for t in tail]))
    E.append(("cgmr_relative_covariance", False, ("robust_kind_9", "edge_index_nV", "query_index_nV"),
              lambda s: [C.c_int(2), _p(s.query), _p(s.pair_b), o(s), o(s), _p(s.cl_meas), _p(s.cl_info), o(s), rk(s)]))
    E.append(("cgmr_observation_covariance", False, ("robust_kind_9", "vertex_kind_2", "edge_index_nV", "query_index_nV"),
              lambda s: [C.c_int(2), _p(s.query), _p(s.pair_b), _p(s.obs_kind), o(s), o(s), _p(s.cl_meas), _p(s.cl_info), o(s), ft(s), rk(s)]))
    E.append(("cgmr_closure_consistency", False, ("robust_kind_9", "edge_index_nV", "query_index_nV"),
              lambda s: [C.c_int(2), _p(s.query), _p(s.pair_b), _p(s.cl_meas), _p(s.cl_info), C.c_double(9.0), o(s), _p(s.outi.view(np.uint64)),
                         oi(s), oi(s), oi(s), rk(s)]))
    return E


def case_ids():
    return [f"{name}:{bad}" for name, _dev, applies, _tail in _entries() for bad in ("meas_null",) + tuple(applies)]


def run_all(lib, ctx_handle):
    out = {}
    for name, dev, applies, tail in _entries():
        no_fixed = name.startswith("cgmr_covariance_estimate") or name.startswith("cgmr_condense")
        for bad in ("meas_null",) + tuple(applies):
            s = _Square(bad, dev)
            rc = getattr(lib, name.split("#")[0])(ctx_handle, *s.problem(with_fixed=not no_fixed), *tail(s))
            out[f"{name}:{bad}"] = [int(rc), lib.cgmr_last_error(ctx_handle).decode()]
    return out
