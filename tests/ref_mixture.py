"""Float64 numpy reference of the max-mixture edges (include/cgmr.h: cgmr_mixture), over ref_typed.  TEST INFRASTRUCTURE ONLY.

The objective is the contract, restated from the header [the method is recalled from Olson and Agarwal's max-mixtures paper,
not read from it]: an edge with the components (z_k, Omega_k, w_k), k = 1..K, contributes

    min_k (r_k + c_k),   r_k = e(z_k)^T Omega_k e(z_k),   c_k = max_j a_j - a_k,   a_k = 2 ln w_k + ln det Omega_k

with r and det formed in the factor's own dimension (3 for kinds 0 and 3, 2 for kinds 1 and 4).  The selected component is
the first argmin.  A linearisation is the typed linearisation of the selected (z, Omega) at the point it is taken at;
Levenberg-Marquardt and dogleg are the policies of ref_lm.py / ref_dogleg.py run on this cost and this system, the way
ref_typed borrows them.

A mixture is (comp_ptr [nE + 1], comp_meas [nC, 3], comp_info [nC, 6], comp_weight [nC]).  Every function that visits a point
can record it in a ``Visits`` object: the selection there and, per multi-component edge, the relative gap between its best
and its second-best cost -- the reach predicate of tests/mixture_cases.py is a bound on the smallest of them."""
from __future__ import annotations

import contextlib
import types

import numpy as np

import ref_numpy as R
import ref_typed as T


def _owner(cptr):
    cptr = np.asarray(cptr, dtype=np.int64)
    return np.repeat(np.arange(len(cptr) - 1), np.diff(cptr))


def own_dim_det(info, ek):
    """det Omega over the factor's own dimension, per component (``ek``: the kind of the component's edge)."""
    u = np.asarray(info, dtype=np.float64).reshape(-1, 6)
    ek = np.asarray(ek)
    O = R.info_full(u)
    det3 = np.linalg.det(O) if len(u) else np.zeros(0)
    det2 = u[:, 0] * u[:, 3] - u[:, 1] * u[:, 1]
    two = (ek == T.SE2_XY) | (ek == T.PRIOR_XY)
    return np.where(two, det2, np.where(ek == 2, u[:, 0], det3))


def offsets(mix, ek=None):
    """c [nC]: max_j a_j - a_k over the components of the same edge; exactly 0 on an edge of one component (whose weight and
    Omega are not looked at)."""
    cptr, _, cinfo, cw = mix
    own = _owner(cptr)
    ek = np.zeros(len(cptr) - 1, np.uint8) if ek is None else np.asarray(ek, dtype=np.uint8)
    single = np.diff(np.asarray(cptr, dtype=np.int64))[own] == 1
    with np.errstate(divide="ignore", invalid="ignore"):
        a = 2 * np.log(np.asarray(cw, dtype=np.float64)) + np.log(own_dim_det(cinfo, ek[own]))
    a[single] = 0.0
    amax = np.full(len(cptr) - 1, -np.inf)
    np.maximum.at(amax, own, a)
    return np.where(single, 0.0, amax[own] - a)


def component_costs(poses, ef, et, mix, ek=None, coff=None):
    """r_k + c_k of every component at ``poses`` [nC]."""
    cptr, cmeas, cinfo, _ = mix
    own = _owner(cptr)
    ek = np.zeros(len(cptr) - 1, np.uint8) if ek is None else np.asarray(ek, dtype=np.uint8)
    coff = offsets(mix, ek) if coff is None else coff
    r = T.edge_chi2(poses, np.asarray(ef)[own], np.asarray(et)[own], cmeas, cinfo, ek[own])
    return r + coff


def select(poses, ef, et, mix, ek=None, coff=None):
    """(selected component per edge [nE], its cost r + c [nE], gap [nE]): gap = (second best - best) / max(second best, tiny)
    of an edge with several components, inf of an edge with one.  Ties go to the lowest index."""
    cptr = np.asarray(mix[0], dtype=np.int64)
    cost = component_costs(poses, ef, et, mix, ek, coff)
    nE = len(cptr) - 1
    sel, best, gap = np.zeros(nE, np.int32), np.zeros(nE), np.full(nE, np.inf)
    for k in range(nE):
        c = cost[cptr[k]:cptr[k + 1]]
        q = int(np.argmin(c))                                   # (numpy: the first of equal minima)
        sel[k], best[k] = q, c[q]
        if len(c) > 1:
            second = float(np.min(np.delete(c, q)))
            gap[k] = (second - c[q]) / max(second, 1e-300)
    return sel, best, gap


class Visits:
    """The linearisation and trial points a reference run went through: per point the selection and the smallest gap of an
    edge whose components are not all identical (``exempt``: edges left out of the gap, the tie cases)."""

    def __init__(self, exempt=()):
        self.sel, self.gap = [], []
        self.exempt = np.asarray(list(exempt), dtype=np.int64)

    def add(self, sel, gap):
        g = np.array(gap, copy=True)
        g[self.exempt] = np.inf
        self.sel.append(sel.copy())
        self.gap.append(float(g.min()) if len(g) else np.inf)

    @property
    def min_gap(self):
        return min(self.gap) if self.gap else np.inf


def selected_graph(mix, sel):
    """(meas [nE, 3], info [nE, 6]) of the selected components."""
    cptr = np.asarray(mix[0], dtype=np.int64)
    p = cptr[:-1] + np.asarray(sel, dtype=np.int64)
    return np.asarray(mix[1], dtype=np.float64).reshape(-1, 3)[p], np.asarray(mix[2], dtype=np.float64).reshape(-1, 6)[p]


def chi2(poses, ef, et, mix, ek=None, coff=None, visits=None):
    """The mixture cost: the sum over the edges of min_k (r_k + c_k)."""
    sel, best, gap = select(poses, ef, et, mix, ek, coff)
    if visits is not None:
        visits.add(sel, gap)
    return float(np.sum(best))


def build_system(poses, fixed, ef, et, mix, vk=None, ek=None, coff=None, visits=None):
    """ref_typed.build_system of the graph selected at ``poses``: (H, b, Layout)."""
    sel, _, gap = select(poses, ef, et, mix, ek, coff)
    if visits is not None:
        visits.add(sel, gap)
    meas, info = selected_graph(mix, sel)
    return T.build_system(poses, fixed, ef, et, meas, info, vk, ek)


def gn_optimize(poses, fixed, ef, et, mix, iters, vk=None, ek=None, visits=None):
    """(poses, chi2 [iters + 1], selection at the returned poses, the selection every iteration linearised with [iters])."""
    x = np.array(poses, dtype=np.float64, copy=True)
    vk, ek = T._kinds(x, ef, vk, ek)
    coff = offsets(mix, ek)
    fx = T.active_fixed(len(x), fixed, ef, et)
    chis, sels = [], []
    for _ in range(iters):
        sel, best, gap = select(x, ef, et, mix, ek, coff)
        if visits is not None:
            visits.add(sel, gap)
        chis.append(float(np.sum(best)))
        sels.append(sel)
        meas, info = selected_graph(mix, sel)
        H, b, lay = T.build_system(x, fx, ef, et, meas, info, vk, ek)
        x = T.apply_step(x, lay, T.splu_solve(H, b))
    sel, best, gap = select(x, ef, et, mix, ek, coff)
    if visits is not None:
        visits.add(sel, gap)
    chis.append(float(np.sum(best)))
    return x, np.array(chis), sel, sels


@contextlib.contextmanager
def _mixture_modules(mix, vk, ek, visits):
    """ref_lm / ref_dogleg see the mixture cost and the selected system while the block runs (ref_typed._typed_modules' way);
    the meas / info they pass through are ignored."""
    import ref_dogleg
    import ref_lm
    coff = offsets(mix, ek)

    def _chi2(p, ef, et, meas, info):
        return chi2(p, ef, et, mix, ek, coff, visits)

    def _build(p, fx, ef, et, meas, info):
        return build_system(p, fx, ef, et, mix, vk, ek, coff, visits)

    shim = types.SimpleNamespace(active_fixed=T.active_fixed, chi2=_chi2, build_system=_build, normalize_theta=R.normalize_theta)
    saved = (ref_lm.R, ref_lm.apply_step, ref_dogleg.R)
    ref_lm.R, ref_lm.apply_step, ref_dogleg.R = shim, T.apply_step, shim
    try:
        yield ref_lm, ref_dogleg
    finally:
        ref_lm.R, ref_lm.apply_step, ref_dogleg.R = saved


def lm_optimize(poses, fixed, ef, et, mix, iters, vk=None, ek=None, visits=None, **params):
    """ref_lm.lm_optimize's result on the mixture cost, with ``selected`` (at the returned poses) added."""
    vk, ek = T._kinds(np.asarray(poses), ef, vk, ek)
    cm, ci = selected_graph(mix, np.zeros(len(ef), np.int64))
    with _mixture_modules(mix, vk, ek, visits) as (ref_lm, _):
        out = ref_lm.lm_optimize(poses, fixed, ef, et, cm, ci, iters, **params)
    out["selected"] = select(out["poses"], ef, et, mix, ek)[0]
    return out


def dl_optimize(poses, fixed, ef, et, mix, iters, vk=None, ek=None, visits=None, **params):
    """ref_dogleg.dl_optimize's result on the mixture cost, with ``selected`` (at the returned poses) added."""
    vk, ek = T._kinds(np.asarray(poses), ef, vk, ek)
    cm, ci = selected_graph(mix, np.zeros(len(ef), np.int64))
    with _mixture_modules(mix, vk, ek, visits) as (_, ref_dogleg):
        out = ref_dogleg.dl_optimize(poses, fixed, ef, et, cm, ci, iters, **params)
    out["selected"] = select(out["poses"], ef, et, mix, ek)[0]
    return out
