"""Host-side mirror of the reference's ``ScanMatcher`` for the hot path (src/matcher/scan_matcher.h:41-85).

``ScanMatcher.closeScanMatching`` keeps the reference's meaning -- match the current scan against the
reference scan inside the window around the odometry guess, return ``(found, trel)`` -- but takes flat
arrays (ranges + guess) instead of g2o vertices, and a batch of independent pairs at once; the work
runs on the MI355X through ``cgmr_match_close_batch`` (include/cgmr.h).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CgmrError, Context


class MatcherConfig(C.Structure):
    """``cgmr_matcher_config`` (include/cgmr.h)."""
    _fields_ = [("grid_ll_x", C.c_float), ("grid_ll_y", C.c_float), ("grid_ur_x", C.c_float), ("grid_ur_y", C.c_float),
                ("resolution", C.c_double), ("kernel_range", C.c_double), ("kscale", C.c_int),
                ("win_x", C.c_double), ("win_y", C.c_double), ("win_theta", C.c_double), ("theta_res", C.c_double),
                ("bin_x", C.c_double), ("bin_y", C.c_double), ("bin_theta", C.c_double), ("subsample_res", C.c_double),
                ("n_beams", C.c_int), ("angle_min", C.c_double), ("angle_inc", C.c_double), ("max_range", C.c_double),
                ("min_range", C.c_double), ("laser_pose", C.c_double * 3)]


class MatchResult(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("theta", C.c_double), ("score", C.c_double)]


class MatchResponse(C.Structure):
    """``struct cgmr_match_response`` (include/cgmr.h): the response surface of a search, cov / info 3x3 row-major."""
    _fields_ = [("mean", C.c_double * 3), ("cov", C.c_double * 9), ("info", C.c_double * 9), ("mass", C.c_double),
                ("border_mass", C.c_double), ("n_candidates", C.c_int64), ("status", C.c_int32), ("reserved", C.c_int32)]


class ResponseJob(C.Structure):
    """``cgmr_response_job`` (include/cgmr.h)."""
    _fields_ = [("n_ref", C.c_int), ("ref_pts_xy", C.c_void_p), ("n_qry", C.c_int), ("qry_pts_xy", C.c_void_p),
                ("n_regions", C.c_int), ("regions", C.c_void_p), ("winner", C.c_double * 4), ("found", C.c_int)]


def _response_dict(r):
    """A MatchResponse as plain numpy values."""
    return {"mean": np.array(r.mean[:]), "cov": np.array(r.cov[:]).reshape(3, 3), "info": np.array(r.info[:]).reshape(3, 3),
            "mass": float(r.mass), "border_mass": float(r.border_mass), "n_candidates": int(r.n_candidates),
            "status": int(r.status)}


class RefineParams(C.Structure):
    """``cgmr_refine_params`` (include/cgmr.h): the numerical settings of a refinement.  ``RefineParams()`` holds the
    defaults of ``cgmr_refine_params_default`` -- 10, 4, 1e-6, 1e-6, 1.0; keyword arguments replace single ones."""
    _fields_ = [("max_iters", C.c_int32), ("max_halvings", C.c_int32), ("ridge", C.c_double), ("step_tol", C.c_double),
                ("bound_steps", C.c_double)]

    def __init__(self, **kw):
        from ._lib import load_library
        fn = load_library().cgmr_refine_params_default
        fn.restype = _RefineParamsPod
        d = fn()
        super().__init__(d.max_iters, d.max_halvings, d.ridge, d.step_tol, d.bound_steps)
        for k, v in kw.items():
            if k not in ("max_iters", "max_halvings", "ridge", "step_tol", "bound_steps"):
                raise TypeError(f"RefineParams has no field {k!r}")
            setattr(self, k, v)


class _RefineParamsPod(C.Structure):
    """(the return type of ``cgmr_refine_params_default``: the fields without the constructor above)"""
    _fields_ = RefineParams._fields_


class MatchRefined(C.Structure):
    """``struct cgmr_match_refined`` (include/cgmr.h): a match moved below the grid's resolution, hessian 3x3 row-major."""
    _fields_ = [("pose", C.c_double * 3), ("cost0", C.c_double), ("cost", C.c_double), ("score0", C.c_double),
                ("score", C.c_double), ("hessian", C.c_double * 9), ("n_active", C.c_int32), ("n_iters", C.c_int32),
                ("n_halvings", C.c_int32), ("stop", C.c_int32), ("at_bound", C.c_int32), ("status", C.c_int32)]


class RefineJob(C.Structure):
    """``cgmr_refine_job`` (include/cgmr.h)."""
    _fields_ = [("n_ref", C.c_int), ("ref_pts_xy", C.c_void_p), ("n_qry", C.c_int), ("qry_pts_xy", C.c_void_p),
                ("winner", C.c_double * 4), ("found", C.c_int)]


def _refined_dict(r):
    """A MatchRefined as plain numpy values."""
    return {"pose": np.array(r.pose[:]), "cost0": float(r.cost0), "cost": float(r.cost), "score0": float(r.score0),
            "score": float(r.score), "hessian": np.array(r.hessian[:]).reshape(3, 3), "n_active": int(r.n_active),
            "n_iters": int(r.n_iters), "n_halvings": int(r.n_halvings), "stop": int(r.stop), "at_bound": int(r.at_bound),
            "status": int(r.status)}


POLISH_MAX_WINNERS = 4        # CGMR_POLISH_MAX_WINNERS (include/cgmr.h)


class _PolishParamsPod(C.Structure):
    """``cgmr_polish_params`` (include/cgmr.h)."""
    _fields_ = [("T", C.c_double), ("window", C.c_double * 3), ("refine", C.c_int32), ("reserved", C.c_int32),
                ("refine_params", _RefineParamsPod)]


class PolishParams:
    """What the polished searches take behind a result (include/cgmr.h, "Polishing a search's results").  ``T``: the
    temperature of the response (see ``matchResponse``; no default -- None: no response).  ``window``: the half-widths
    (x, y, theta) of the response's window around a winner; the default is the searches' own results discretisation
    (dx, dy, dth), the distance below which the search itself counts two results as one match.  ``refine``: a
    ``RefineParams`` (see ``matchRefine``), None: no refinement."""

    def __init__(self, T=None, window=(0.5, 0.5, 0.2), refine=None):   # noqa: N803
        if refine is not None and not isinstance(refine, RefineParams):
            raise ValueError("PolishParams: refine must be a RefineParams or None")
        self.T = None if T is None else float(T)
        self.window = tuple(float(w) for w in window)
        if len(self.window) != 3:
            raise ValueError("PolishParams: window holds three half-widths (x, y, theta)")
        self.refine = refine

    def pod(self):
        p = _PolishParamsPod()
        p.T = 0.0 if self.T is None else self.T
        for q in range(3):
            p.window[q] = self.window[q]
        p.refine = 0 if self.refine is None else 1
        r = RefineParams() if self.refine is None else self.refine
        for k, _ in RefineParams._fields_:
            setattr(p.refine_params, k, getattr(r, k))
        return p


class MatchPolished(C.Structure):
    """``struct cgmr_match_polished`` (include/cgmr.h): the response and the refinement of one winner."""
    _fields_ = [("response", MatchResponse), ("refined", MatchRefined)]


class PolishJob(C.Structure):
    """``cgmr_polish_job`` (include/cgmr.h)."""
    _fields_ = [("n_ref", C.c_int), ("ref_pts_xy", C.c_void_p), ("n_qry", C.c_int), ("qry_pts_xy", C.c_void_p),
                ("n_winners", C.c_int), ("winners", (C.c_double * 4) * POLISH_MAX_WINNERS)]


def _polished_dict(e):
    return {"response": _response_dict(e.response), "refined": _refined_dict(e.refined)}


def _se2_mul(a, b):
    """g2o SE2 product: translation a.t + R(a.theta) b.t, angle normalised [g2o-recalled]."""
    import math
    c, s = math.cos(a[2]), math.sin(a[2])
    t = a[2] + b[2]
    if not (-math.pi <= t < math.pi):
        t = t - 2 * math.pi * math.floor((t + math.pi) / (2 * math.pi))
    return np.array([a[0] + (c * b[0] - s * b[1]), a[1] + (s * b[0] + c * b[1]), t])


def _se2_inv(a):
    import math
    c, s = math.cos(a[2]), math.sin(a[2])
    return np.array([-(c * a[0] + s * a[1]), -(-s * a[0] + c * a[1]), -a[2]])


def normalize_theta(t):
    import math
    if -math.pi <= t < math.pi:
        return t
    return t - 2 * math.pi * math.floor((t + math.pi) / (2 * math.pi))


class ScanSet(C.Structure):
    """``cgmr_scan_set`` (include/cgmr.h): the flat form of a g2o VertexSet with RobotLaser data + its reference vertex."""
    _fields_ = [("n_scans", C.c_int), ("ranges", C.c_void_p), ("poses_xyt", C.c_void_p), ("ref_index", C.c_int)]


_STACKED = {}                 # tuple of id(ranges array) -> (the arrays themselves, their stack): a key-frame driver passes the same
_STACKED_MAX = 512            # scans of the same vertices again and again (up to 21 x 1081 floats per set)


def _scan_set(scans, ref_index):
    """scans: list of (ranges, pose).  Returns (ScanSet, keep-alive arrays)."""
    key = tuple(id(r) for r, _ in scans)
    hit = _STACKED.get(key)
    if hit is not None and all(a is r for a, (r, _) in zip(hit[0], scans)):
        ranges = hit[1]
    else:
        ranges = np.ascontiguousarray(np.stack([np.asarray(r, dtype=np.float32) for r, _ in scans]), dtype=np.float32)
        if all(isinstance(r, np.ndarray) and not r.flags.writeable for r, _ in scans):   # (only scans nobody can change behind the cache)
            if len(_STACKED) >= _STACKED_MAX:
                _STACKED.clear()
            _STACKED[key] = ([r for r, _ in scans], ranges)
    poses = np.array([p for _, p in scans], dtype=np.float64).reshape(len(scans), 3)
    s = ScanSet(len(scans), C.c_void_p(ranges.ctypes.data), C.c_void_p(poses.ctypes.data), int(ref_index))
    return s, (ranges, poses)


class _GenericSearch:
    """The ScanMatcher member functions every matcher can run (grid / kernel / laser taken from ``self.cfg``), thin
    callers of the C ABI (csrc/matcher_api.cpp does the region / transform bookkeeping, the GPU the searches).  Scans
    are passed as ``(ranges, vertex_pose)`` pairs, the flat-array form of a g2o VertexSet with RobotLaser user data."""

    # ---- host helpers with the reference's arithmetic (libcgmr.so, no GPU) -----------------------------------
    def cartesian(self, ranges):
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        out = np.zeros((len(r), 2))
        n = self.ctx.lib.cgmr_scan_cartesian(C.c_int(len(r)), C.c_void_p(r.ctypes.data), C.c_double(self.cfg.angle_min),
                                             C.c_double(self.cfg.angle_inc), C.c_double(self.cfg.max_range),
                                             C.c_double(self.cfg.min_range), C.c_void_p(out.ctypes.data))
        return out[:n].copy()

    def subsample(self, pts, res=0.1):
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
        out = np.zeros_like(pts)
        n = self.ctx.lib.cgmr_subsample(C.c_int(len(pts)), C.c_void_p(pts.ctypes.data), C.c_double(res),
                                        C.c_void_p(out.ctypes.data))
        return out[:n].copy()

    @staticmethod
    def applyTransfToScan(transf, pts):   # noqa: N802  (scan_matcher.cpp:78-87)
        import math
        c, s = math.cos(transf[2]), math.sin(transf[2])
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
        return np.stack([(c * pts[:, 0] - s * pts[:, 1]) + transf[0], (s * pts[:, 0] + c * pts[:, 1]) + transf[1]], axis=1)

    def transformPointsFromVSet(self, scans, ref_index):   # noqa: N802  (scan_matcher.cpp:89-110)
        """scans: list of (ranges, pose) in the caller's (id-ordered) iteration order; ref_index: the reference vertex."""
        s, keep = _scan_set(scans, ref_index)
        cap = len(scans) * int(self.cfg.n_beams)
        out = np.zeros((max(cap, 1), 2))
        n = self.ctx.lib.cgmr_transform_points_from_vset(C.byref(self.cfg), C.byref(s), C.c_void_p(out.ctypes.data), C.c_int(cap))
        if n < 0:
            raise CgmrError(n, "cgmr_transform_points_from_vset: bad scan set")
        return out[:n].copy()

    # ---- CharGrid::greedySearch / hierarchicalSearch on the GPU ---------------------------------------------
    def greedySearch(self, ref_pts, qry_pts, regions, thetaRes, maxScore, dx, dy, dth, step=None, cap=65536):   # noqa: N802,N803
        ref = np.ascontiguousarray(ref_pts, dtype=np.float64).reshape(-1, 2)
        qry = np.ascontiguousarray(qry_pts, dtype=np.float64).reshape(-1, 2)
        reg = np.ascontiguousarray(regions, dtype=np.float32).reshape(-1, 6)
        step = float(np.float32(self.cfg.resolution)) if step is None else float(step)
        buf = (MatchResult * cap)()
        n = C.c_int(0)
        rc = self.ctx.lib.cgmr_match_greedy(self.ctx.h, C.byref(self.cfg), C.c_int(len(ref)), C.c_void_p(ref.ctypes.data),
                                            C.c_int(len(qry)), C.c_void_p(qry.ctypes.data), C.c_int(len(reg)),
                                            C.c_void_p(reg.ctypes.data), C.c_double(step), C.c_double(step),
                                            C.c_double(thetaRes), C.c_double(maxScore), C.c_double(dx), C.c_double(dy),
                                            C.c_double(dth), buf, C.c_int(cap), C.byref(n))
        self.ctx._check(rc)
        m = min(n.value, cap)
        return np.array([[buf[k].x, buf[k].y, buf[k].theta, buf[k].score] for k in range(m)]).reshape(-1, 4)

    def hierarchicalSearch(self, ref_pts, qry_pts, regions, thetaRes, maxScore, dx, dy, dth, nLevels, cap=65536):   # noqa: N802,N803
        """CharGrid::hierarchicalSearch (chargrid.cpp:310-344, 376-400) through ``cgmr_match_hierarchical``."""
        ref = np.ascontiguousarray(ref_pts, dtype=np.float64).reshape(-1, 2)
        qry = np.ascontiguousarray(qry_pts, dtype=np.float64).reshape(-1, 2)
        reg = np.ascontiguousarray(regions, dtype=np.float32).reshape(-1, 6)
        buf = (MatchResult * cap)()
        n = C.c_int(0)
        rc = self.ctx.lib.cgmr_match_hierarchical(self.ctx.h, C.byref(self.cfg), C.c_int(len(ref)), C.c_void_p(ref.ctypes.data),
                                                  C.c_int(len(qry)), C.c_void_p(qry.ctypes.data), C.c_int(len(reg)),
                                                  C.c_void_p(reg.ctypes.data), C.c_double(thetaRes), C.c_double(maxScore),
                                                  C.c_double(dx), C.c_double(dy), C.c_double(dth), C.c_int(nLevels), buf,
                                                  C.c_int(cap), C.byref(n))
        self.ctx._check(rc)
        m = min(n.value, cap)
        return np.array([[buf[k].x, buf[k].y, buf[k].theta, buf[k].score] for k in range(m)]).reshape(-1, 4)

    # ---- the response surface of a search: the information matrix of the match itself (include/cgmr.h) -------
    def matchResponse(self, ref_pts, qry_pts, region, thetaRes, T, winner, step=None):   # noqa: N802,N803
        """The weighted second moments of the candidates of ``greedySearch`` over ONE region around ``winner`` =
        (x*, y*, theta*, s*), at temperature ``T`` (metres of score; no default -- DESIGN.md).  Returns a dict: mean, cov,
        info (3x3, info in the frame g2o's EdgeSE2 error lives in), mass, border_mass, n_candidates, status."""
        ref = np.ascontiguousarray(ref_pts, dtype=np.float64).reshape(-1, 2)
        qry = np.ascontiguousarray(qry_pts, dtype=np.float64).reshape(-1, 2)
        reg = np.ascontiguousarray(region, dtype=np.float32).reshape(-1, 6)
        if len(reg) != 1:
            raise ValueError("a response has exactly one region")
        win = np.ascontiguousarray(winner, dtype=np.float64).reshape(4)
        step = float(np.float32(self.cfg.resolution)) if step is None else float(step)
        out = MatchResponse()
        rc = self.ctx.lib.cgmr_match_response(self.ctx.h, C.byref(self.cfg), C.c_int(len(ref)), C.c_void_p(ref.ctypes.data),
                                              C.c_int(len(qry)), C.c_void_p(qry.ctypes.data), C.c_void_p(reg.ctypes.data),
                                              C.c_double(step), C.c_double(step), C.c_double(thetaRes), C.c_double(T),
                                              C.c_void_p(win.ctypes.data), C.byref(out))
        self.ctx._check(rc)
        return _response_dict(out)

    def matchResponseBatch(self, jobs, thetaRes, T, step=None, raw=False):   # noqa: N802,N803
        """``matchResponse`` for many searches in one launch.  ``jobs``: list of (ref_pts, qry_pts, region, winner) with
        ``winner`` None for a search that found nothing (status 2).  ``raw``: the result structs' bytes instead of dicts."""
        step = float(np.float32(self.cfg.resolution)) if step is None else float(step)
        arr = (ResponseJob * max(len(jobs), 1))()
        keep = []
        for k, (ref_pts, qry_pts, region, winner) in enumerate(jobs):
            ref = np.ascontiguousarray(ref_pts, dtype=np.float64).reshape(-1, 2)
            qry = np.ascontiguousarray(qry_pts, dtype=np.float64).reshape(-1, 2)
            reg = np.ascontiguousarray(region, dtype=np.float32).reshape(-1, 6)
            keep.append((ref, qry, reg))
            arr[k].n_ref, arr[k].ref_pts_xy = len(ref), ref.ctypes.data
            arr[k].n_qry, arr[k].qry_pts_xy = len(qry), qry.ctypes.data
            arr[k].n_regions, arr[k].regions = len(reg), reg.ctypes.data
            arr[k].found = 0 if winner is None else 1
            for q in range(4):
                arr[k].winner[q] = 0.0 if winner is None else float(winner[q])
        out = (MatchResponse * max(len(jobs), 1))()
        rc = self.ctx.lib.cgmr_match_response_batch(self.ctx.h, C.byref(self.cfg), C.c_int(len(jobs)), arr, C.c_double(step),
                                                    C.c_double(step), C.c_double(thetaRes), C.c_double(T), out)
        self.ctx._check(rc)
        if raw:
            return bytes(out)[:C.sizeof(MatchResponse) * len(jobs)]
        return [_response_dict(out[k]) for k in range(len(jobs))]

    # ---- refining a match below the grid's resolution (include/cgmr.h, "Refining a match") -------------------
    def matchRefine(self, ref_pts, qry_pts, thetaRes, winner, params=None, step=None, raw=False):   # noqa: N802,N803
        """Damped Gauss-Newton on the bilinear distance field of ``ref_pts``, started at ``winner`` = (x*, y*, theta*, s*)
        of the search before and kept within ``params.bound_steps`` search steps of it; ``winner`` None = the search
        found nothing (status 2).  Returns a dict: pose, cost0, cost, score0, score, hessian (3x3), n_active, n_iters,
        n_halvings, stop, at_bound, status (``raw``: the result struct's bytes instead).  The pose's cost is not higher
        than the winner's; nothing more is promised."""
        ref = np.ascontiguousarray(ref_pts, dtype=np.float64).reshape(-1, 2)
        qry = np.ascontiguousarray(qry_pts, dtype=np.float64).reshape(-1, 2)
        win = np.zeros(4) if winner is None else np.ascontiguousarray(winner, dtype=np.float64).reshape(4)
        par = RefineParams() if params is None else params
        step = float(np.float32(self.cfg.resolution)) if step is None else float(step)
        out = MatchRefined()
        rc = self.ctx.lib.cgmr_match_refine(self.ctx.h, C.byref(self.cfg), C.c_int(len(ref)), C.c_void_p(ref.ctypes.data),
                                            C.c_int(len(qry)), C.c_void_p(qry.ctypes.data), C.c_double(step), C.c_double(step),
                                            C.c_double(thetaRes), C.c_void_p(win.ctypes.data), C.c_int(0 if winner is None else 1),
                                            C.byref(par), C.byref(out))
        self.ctx._check(rc)
        return bytes(out) if raw else _refined_dict(out)

    def matchRefineBatch(self, jobs, thetaRes, params=None, step=None, raw=False):   # noqa: N802,N803
        """``matchRefine`` for many matches in one launch, one workgroup each.  ``jobs``: list of (ref_pts, qry_pts, winner)
        with ``winner`` None for a search that found nothing.  ``raw``: the result structs' bytes instead of dicts."""
        par = RefineParams() if params is None else params
        step = float(np.float32(self.cfg.resolution)) if step is None else float(step)
        arr = (RefineJob * max(len(jobs), 1))()
        keep = []
        for k, (ref_pts, qry_pts, winner) in enumerate(jobs):
            ref = np.ascontiguousarray(ref_pts, dtype=np.float64).reshape(-1, 2)
            qry = np.ascontiguousarray(qry_pts, dtype=np.float64).reshape(-1, 2)
            keep.append((ref, qry))
            arr[k].n_ref, arr[k].ref_pts_xy = len(ref), ref.ctypes.data
            arr[k].n_qry, arr[k].qry_pts_xy = len(qry), qry.ctypes.data
            arr[k].found = 0 if winner is None else 1
            for q in range(4):
                arr[k].winner[q] = 0.0 if winner is None else float(winner[q])
        out = (MatchRefined * max(len(jobs), 1))()
        rc = self.ctx.lib.cgmr_match_refine_batch(self.ctx.h, C.byref(self.cfg), C.c_int(len(jobs)), arr, C.c_double(step),
                                                  C.c_double(step), C.c_double(thetaRes), C.byref(par), out)
        self.ctx._check(rc)
        if raw:
            return bytes(out)[:C.sizeof(MatchRefined) * len(jobs)]
        return [_refined_dict(out[k]) for k in range(len(jobs))]

    # ---- refinement and response of a search's results behind one rasterisation (include/cgmr.h) -------------
    def matchPolishBatch(self, jobs, thetaRes, params, step=None, raw=False):   # noqa: N802,N803
        """``matchRefine`` and ``matchResponse`` for up to four winners per job, one workgroup and ONE rasterisation of the
        job's grid each, all jobs in one launch.  ``jobs``: list of (ref_pts, qry_pts, winners) with ``winners`` a list of
        (x*, y*, theta*, s*); ``params``: a ``PolishParams``.  Returns per job a list of {"response", "refined"} dicts, one
        per winner; a part that was not asked for has status 3.  ``raw``: the bytes of all 4 result structs of every job."""
        step = float(np.float32(self.cfg.resolution)) if step is None else float(step)
        arr = (PolishJob * max(len(jobs), 1))()
        keep = []
        for k, (ref_pts, qry_pts, winners) in enumerate(jobs):
            ref = np.ascontiguousarray(ref_pts, dtype=np.float64).reshape(-1, 2)
            qry = np.ascontiguousarray(qry_pts, dtype=np.float64).reshape(-1, 2)
            keep.append((ref, qry))
            arr[k].n_ref, arr[k].ref_pts_xy = len(ref), ref.ctypes.data
            arr[k].n_qry, arr[k].qry_pts_xy = len(qry), qry.ctypes.data
            arr[k].n_winners = len(winners)                       # (more than four: the call refuses it by name)
            for w, win in enumerate(winners[:POLISH_MAX_WINNERS]):
                for q in range(4):
                    arr[k].winners[w][q] = float(win[q])
        out = (MatchPolished * max(POLISH_MAX_WINNERS * len(jobs), 1))()
        par = params.pod()
        rc = self.ctx.lib.cgmr_match_polish_batch(self.ctx.h, C.byref(self.cfg), C.c_int(len(jobs)), arr, C.c_double(step),
                                                  C.c_double(step), C.c_double(thetaRes), C.byref(par), out)
        self.ctx._check(rc)
        if raw:
            return bytes(out)[:C.sizeof(MatchPolished) * POLISH_MAX_WINNERS * len(jobs)]
        return [[_polished_dict(out[POLISH_MAX_WINNERS * k + w]) for w in range(len(jobs[k][2]))] for k in range(len(jobs))]

    # ---- ScanMatcher::scanMatchingLC (scan_matcher.cpp:201-294) ---------------------------------------------
    def scanMatchingLC(self, ref_scans, ref_index, cur_scans, cur_index, maxScore, polish=None):   # noqa: N802,N803
        """Returns the list of SE2 (x, y, theta) the reference pushes into ``trel`` (0-2 entries).  With ``polish`` (a
        ``PolishParams``) every result is polished behind the search: returns (that list, a list of {"response", "refined"}
        dicts, one per result)."""
        a, ka = _scan_set(ref_scans, ref_index)
        b, kb = _scan_set(cur_scans, cur_index)
        out = np.zeros((2, 3))
        n = C.c_int(0)
        if polish is not None:
            par, pol = polish.pod(), (MatchPolished * 2)()
            rc = self.ctx.lib.cgmr_scan_matching_lc_polished(self.ctx.h, C.byref(self.cfg), C.byref(a), C.byref(b), C.c_double(maxScore),
                                                             C.byref(par), C.c_void_p(out.ctypes.data), C.byref(n), pol)
            self.ctx._check(rc)
            return [out[k].copy() for k in range(n.value)], [_polished_dict(pol[k]) for k in range(n.value)]
        rc = self.ctx.lib.cgmr_scan_matching_lc(self.ctx.h, C.byref(self.cfg), C.byref(a), C.byref(b), C.c_double(maxScore),
                                                C.c_void_p(out.ctypes.data), C.byref(n))
        self.ctx._check(rc)
        return [out[k].copy() for k in range(n.value)]

    # ---- ScanMatcher::globalMatching (scan_matcher.cpp:366-428) ---------------------------------------------
    def globalMatching(self, ref_scans, ref_index, cur_scans, cur_index, maxScore, polish=None):   # noqa: N802,N803
        """Returns (found, trel).  With ``polish`` (a ``PolishParams``): ((found, trel), a list of one {"response", "refined"}
        dict when something was found, else an empty one)."""
        a, ka = _scan_set(ref_scans, ref_index)
        b, kb = _scan_set(cur_scans, cur_index)
        out = np.zeros(3)
        found = C.c_int(0)
        if polish is not None:
            par, pol = polish.pod(), MatchPolished()
            rc = self.ctx.lib.cgmr_global_matching_polished(self.ctx.h, C.byref(self.cfg), C.byref(a), C.byref(b), C.c_double(maxScore),
                                                            C.byref(par), C.c_void_p(out.ctypes.data), C.byref(found), C.byref(pol))
            self.ctx._check(rc)
            return ((True, out.copy()), [_polished_dict(pol)]) if found.value else ((False, None), [])
        rc = self.ctx.lib.cgmr_global_matching(self.ctx.h, C.byref(self.cfg), C.byref(a), C.byref(b), C.c_double(maxScore),
                                               C.c_void_p(out.ctypes.data), C.byref(found))
        self.ctx._check(rc)
        return (True, out.copy()) if found.value else (False, None)

    def scanMatchingLChierarchical(self, ref_scans, ref_index, cur_scans, cur_index, maxScore):   # noqa: N802,N803
        """``ScanMatcher::scanMatchingLChierarchical`` (scan_matcher.cpp:296-356): one region of +-(2, 2, 1) around
        reference^-1 * current, three hierarchy levels; returns (found, [trel]) like the reference's vector of at most one."""
        a, ka = _scan_set(ref_scans, ref_index)
        b, kb = _scan_set(cur_scans, cur_index)
        out = np.zeros(3)
        found = C.c_int(0)
        rc = self.ctx.lib.cgmr_scan_matching_lc_hierarchical(self.ctx.h, C.byref(self.cfg), C.byref(a), C.byref(b), C.c_double(maxScore),
                                                             C.c_void_p(out.ctypes.data), C.byref(found))
        self.ctx._check(rc)
        return (True, [out.copy()]) if found.value else (False, [])

    # ---- ScanMatcher::closeScanMatching with a multi-scan reference set (scan_matcher.cpp:112-189) ---------------
    def closeScanMatchingVSet(self, ref_scans, origin_index, cur_ranges, cur_pose, maxScore=0.15, covariance_T=None, refine=None):   # noqa: N802,N803
        """The reference's call shape: up to 6 reference scans (graph_slam.cpp:230-241) rasterised in the frame of the
        origin vertex, the current scan subsampled, window around origin^-1 * current.  Returns (found, trel).
        With ``covariance_T`` (a temperature, see ``matchResponse``) the response surface of the same window is taken
        behind the search: returns (found, trel, info, response) -- info 3x3, zeros unless response["status"] == 0.
        With ``refine`` (a ``RefineParams``, see ``matchRefine``) the winner is refined on the same points: ``trel`` is the
        refined pose and the refinement's result dict comes last -- (found, trel, refined), or with ``covariance_T`` as
        well (found, trel, info, response, refined), the response still taken around the search's winner.  The dict
        carries the search's own winner as ``search``."""
        a, ka = _scan_set(ref_scans, origin_index)
        cur = np.ascontiguousarray(cur_ranges, dtype=np.float32)
        pose = np.ascontiguousarray(cur_pose, dtype=np.float64)
        out = np.zeros(3)
        found = C.c_int(0)
        if refine is not None:
            ref, search = MatchRefined(), np.zeros(3)
            rc = self.ctx.lib.cgmr_close_scan_matching_refined(self.ctx.h, C.byref(self.cfg), C.byref(a), C.c_void_p(cur.ctypes.data),
                                                               C.c_void_p(pose.ctypes.data), C.c_double(maxScore), C.byref(refine),
                                                               C.c_void_p(out.ctypes.data), C.c_void_p(search.ctypes.data),
                                                               C.byref(found), C.byref(ref))
            self.ctx._check(rc)
            refined = dict(_refined_dict(ref), search=search.copy() if found.value else None)
            trel = out.copy() if found.value else None
            if covariance_T is None:
                return (bool(found.value), trel, refined)
            _, _, info, resp = self.closeScanMatchingVSet(ref_scans, origin_index, cur_ranges, cur_pose, maxScore, covariance_T=covariance_T)
            return (bool(found.value), trel, info, resp, refined)
        if covariance_T is not None:
            info, resp = np.zeros(9), MatchResponse()
            rc = self.ctx.lib.cgmr_close_scan_matching_cov(self.ctx.h, C.byref(self.cfg), C.byref(a), C.c_void_p(cur.ctypes.data),
                                                           C.c_void_p(pose.ctypes.data), C.c_double(maxScore),
                                                           C.c_double(covariance_T), C.c_void_p(out.ctypes.data), C.byref(found),
                                                           C.c_void_p(info.ctypes.data), C.byref(resp))
            self.ctx._check(rc)
            return (bool(found.value), out.copy() if found.value else None, info.reshape(3, 3), _response_dict(resp))
        rc = self.ctx.lib.cgmr_close_scan_matching(self.ctx.h, C.byref(self.cfg), C.byref(a), C.c_void_p(cur.ctypes.data),
                                                   C.c_void_p(pose.ctypes.data), C.c_double(maxScore),
                                                   C.c_void_p(out.ctypes.data), C.byref(found))
        self.ctx._check(rc)
        return (True, out.copy()) if found.value else (False, None)

    # ---- ScanMatcher::verifyMatching (scan_matcher.cpp:430-505) --------------------------------------------------
    def verifyMatching(self, scans1, ref1_index, scans2, ref2_index, trel12):   # noqa: N802
        """Returns (accepted, score).  ``trel12``: pose of reference vertex 2 in the frame of reference vertex 1."""
        a, ka = _scan_set(scans1, ref1_index)
        b, kb = _scan_set(scans2, ref2_index)
        t = np.ascontiguousarray(trel12, dtype=np.float64)
        score = C.c_double()
        acc = C.c_int()
        rc = self.ctx.lib.cgmr_verify_matching(self.ctx.h, C.byref(self.cfg), C.byref(a), C.byref(b), C.c_void_p(t.ctypes.data),
                                               C.byref(score), C.byref(acc))
        self.ctx._check(rc)
        return bool(acc.value), score.value


def _scan_set_array(sets):
    """list of (scans, ref_index) -> (ctypes array of ScanSet, keep-alive list)."""
    arr = (ScanSet * len(sets))()
    keep = []
    for k, (scans, ri) in enumerate(sets):
        s, ka = _scan_set(scans, ri)
        arr[k] = s
        keep.append(ka)
    return arr, keep


class _BatchedSearch:
    """Batched forms of the ScanMatcher member functions: many independent calls, one kernel launch
    per search level.  ``jobs``: list of (ref_scans, ref_index, cur_scans, cur_index)."""

    def scanMatchingLCBatch(self, jobs, maxScore, polish=None):   # noqa: N802,N803
        """Returns per job the list of ``scanMatchingLC``.  With ``polish`` (a ``PolishParams``): (those lists, per job a
        list of {"response", "refined"} dicts, one per result), every result of the batch polished in one launch."""
        a, ka = _scan_set_array([(j[0], j[1]) for j in jobs])
        b, kb = _scan_set_array([(j[2], j[3]) for j in jobs])
        out, n = np.zeros((len(jobs), 2, 3)), np.zeros(len(jobs), dtype=np.int32)
        if polish is not None:
            par, pol = polish.pod(), (MatchPolished * max(2 * len(jobs), 1))()
            self.ctx._check(self.ctx.lib.cgmr_scan_matching_lc_polished_batch(self.ctx.h, C.byref(self.cfg), C.c_int(len(jobs)), a, b,
                                                                              C.c_double(maxScore), C.byref(par),
                                                                              C.c_void_p(out.ctypes.data), C.c_void_p(n.ctypes.data), pol))
            return ([[out[j, k].copy() for k in range(n[j])] for j in range(len(jobs))],
                    [[_polished_dict(pol[2 * j + k]) for k in range(n[j])] for j in range(len(jobs))])
        self.ctx._check(self.ctx.lib.cgmr_scan_matching_lc_batch(self.ctx.h, C.byref(self.cfg), C.c_int(len(jobs)), a, b,
                                                                 C.c_double(maxScore), C.c_void_p(out.ctypes.data),
                                                                 C.c_void_p(n.ctypes.data)))
        return [[out[j, k].copy() for k in range(n[j])] for j in range(len(jobs))]

    def globalMatchingBatch(self, jobs, maxScore, polish=None):   # noqa: N802,N803
        """Returns per job (found, trel).  With ``polish`` (a ``PolishParams``): (that list, per job a list of one
        {"response", "refined"} dict when something was found, else an empty one)."""
        a, ka = _scan_set_array([(j[0], j[1]) for j in jobs])
        b, kb = _scan_set_array([(j[2], j[3]) for j in jobs])
        out, f = np.zeros((len(jobs), 3)), np.zeros(len(jobs), dtype=np.int32)
        if polish is not None:
            par, pol = polish.pod(), (MatchPolished * max(len(jobs), 1))()
            self.ctx._check(self.ctx.lib.cgmr_global_matching_polished_batch(self.ctx.h, C.byref(self.cfg), C.c_int(len(jobs)), a, b,
                                                                             C.c_double(maxScore), C.byref(par),
                                                                             C.c_void_p(out.ctypes.data), C.c_void_p(f.ctypes.data), pol))
            return ([(True, out[j].copy()) if f[j] else (False, None) for j in range(len(jobs))],
                    [[_polished_dict(pol[j])] if f[j] else [] for j in range(len(jobs))])
        self.ctx._check(self.ctx.lib.cgmr_global_matching_batch(self.ctx.h, C.byref(self.cfg), C.c_int(len(jobs)), a, b,
                                                                C.c_double(maxScore), C.c_void_p(out.ctypes.data),
                                                                C.c_void_p(f.ctypes.data)))
        return [(True, out[j].copy()) if f[j] else (False, None) for j in range(len(jobs))]

    def scanMatchingLChierarchicalBatch(self, jobs, maxScore):   # noqa: N802,N803
        """jobs: list of (ref_scans, ref_index, cur_scans, cur_index).  Returns [(found, [trel])] like the single calls."""
        a, ka = _scan_set_array([(j[0], j[1]) for j in jobs])
        b, kb = _scan_set_array([(j[2], j[3]) for j in jobs])
        out, f = np.zeros((len(jobs), 3)), np.zeros(len(jobs), dtype=np.int32)
        self.ctx._check(self.ctx.lib.cgmr_scan_matching_lc_hierarchical_batch(self.ctx.h, C.byref(self.cfg), C.c_int(len(jobs)), a, b,
                                                                              C.c_double(maxScore), C.c_void_p(out.ctypes.data),
                                                                              C.c_void_p(f.ctypes.data)))
        return [(True, [out[j].copy()]) if f[j] else (False, []) for j in range(len(jobs))]

    def verifyMatchingBatch(self, jobs, trel12):   # noqa: N802
        """jobs: list of (scans1, ref1_index, scans2, ref2_index); trel12 (n, 3).  Returns [(accepted, score)]."""
        a, ka = _scan_set_array([(j[0], j[1]) for j in jobs])
        b, kb = _scan_set_array([(j[2], j[3]) for j in jobs])
        t = np.ascontiguousarray(trel12, dtype=np.float64).reshape(len(jobs), 3)
        sc, acc = np.zeros(len(jobs)), np.zeros(len(jobs), dtype=np.int32)
        self.ctx._check(self.ctx.lib.cgmr_verify_matching_batch(self.ctx.h, C.byref(self.cfg), C.c_int(len(jobs)), a, b,
                                                                C.c_void_p(t.ctypes.data), C.c_void_p(sc.ctypes.data),
                                                                C.c_void_p(acc.ctypes.data)))
        return [(bool(acc[j]), float(sc[j])) for j in range(len(jobs))]


class ScanMatcher(_GenericSearch, _BatchedSearch):
    """The close-range matcher the reference builds in GraphSLAM::init (src/slam/graph_slam.cpp:58-59):
    ``initializeKernel(resolution, kernelRadius)`` + ``initializeGrid((-15,-15),(15,15), resolution)``."""

    def __init__(self, ctx: Context, n_beams: int, angle_min: float, angle_inc: float, max_range: float,
                 laser_pose=(0.0, 0.0, 0.0), resolution: float = 0.025, kernel_range: float = 0.2):
        self.ctx = ctx
        self.cfg = MatcherConfig()
        ctx.lib.cgmr_matcher_config_close(C.byref(self.cfg), C.c_int(n_beams), C.c_double(angle_min),
                                          C.c_double(angle_inc), C.c_double(max_range))
        self.initializeKernel(resolution, kernel_range)
        for k in range(3):
            self.cfg.laser_pose[k] = float(laser_pose[k])

    # reference spellings ----------------------------------------------------------------------
    def initializeKernel(self, resolution, kernelRange):   # noqa: N802,N803
        self.cfg.resolution = float(resolution)
        self.cfg.kernel_range = float(kernelRange)

    def initializeGrid(self, lowerLeft, upperRight, resolution):   # noqa: N802,N803
        self.cfg.grid_ll_x, self.cfg.grid_ll_y = float(lowerLeft[0]), float(lowerLeft[1])
        self.cfg.grid_ur_x, self.cfg.grid_ur_y = float(upperRight[0]), float(upperRight[1])
        self.cfg.resolution = float(resolution)

    def closeScanMatching(self, ranges_ref, ranges_cur, guess, maxScore=0.15, want_nresults=False):   # noqa: N802,N803
        """Batched ``closeScanMatching``.  ``ranges_*``: (P, n_beams) float32; ``guess``: (P, 3)
        = origin^-1 * current.  Returns (found[P] bool, trel[P,3], score[P])."""
        rr = np.ascontiguousarray(ranges_ref, dtype=np.float32)
        rq = np.ascontiguousarray(ranges_cur, dtype=np.float32)
        single = rr.ndim == 1
        if single:
            rr, rq = rr[None], rq[None]
        P, B = rr.shape
        if B != self.cfg.n_beams or rq.shape != rr.shape:
            raise ValueError("ranges must be (n_pairs, n_beams)")
        g = np.ascontiguousarray(guess, dtype=np.float64).reshape(P, 3)
        xyt = np.zeros((P, 3))
        score = np.zeros(P)
        found = np.zeros(P, dtype=np.uint8)
        nres = np.zeros(P, dtype=np.int32)
        rc = self.ctx.lib.cgmr_match_close_batch(self.ctx.h, C.byref(self.cfg), C.c_int(P), C.c_void_p(rr.ctypes.data),
                                                 C.c_void_p(rq.ctypes.data), C.c_void_p(g.ctypes.data),
                                                 C.c_double(maxScore), C.c_void_p(xyt.ctypes.data),
                                                 C.c_void_p(score.ctypes.data), C.c_void_p(found.ctypes.data),
                                                 C.c_void_p(nres.ctypes.data if want_nresults else 0))
        self.ctx._check(rc)
        if want_nresults:
            return found.astype(bool), xyt, score, nres
        return found.astype(bool), xyt, score

    def closeScanMatchingVSetBatch(self, ranges_ref, ref_rel, ranges_cur, guess, maxScore=0.15):   # noqa: N802,N803
        """Batched ``closeScanMatching`` with the reference's call shape: ``ranges_ref`` (P, S, n_beams) -- S <= 6 scans per
        reference set (last vertex + predecessors, graph_slam.cpp:230-244), ``ref_rel`` (P, S, 3) = origin^-1 * v_k (zeros
        for the origin), ``ranges_cur`` (P, n_beams), ``guess`` (P, 3).  Returns (found[P], trel[P,3], score[P])."""
        rr = np.ascontiguousarray(ranges_ref, dtype=np.float32)
        P, S, B = rr.shape
        rq = np.ascontiguousarray(ranges_cur, dtype=np.float32).reshape(P, B)
        rel = np.ascontiguousarray(ref_rel, dtype=np.float64).reshape(P, S, 3)
        g = np.ascontiguousarray(guess, dtype=np.float64).reshape(P, 3)
        xyt, score, found = np.zeros((P, 3)), np.zeros(P), np.zeros(P, dtype=np.uint8)
        rc = self.ctx.lib.cgmr_match_close_vset_batch(self.ctx.h, C.byref(self.cfg), C.c_int(P), C.c_int(S), C.c_void_p(rr.ctypes.data),
                                                      C.c_void_p(rel.ctypes.data), C.c_void_p(rq.ctypes.data),
                                                      C.c_void_p(g.ctypes.data), C.c_double(maxScore), C.c_void_p(xyt.ctypes.data),
                                                      C.c_void_p(score.ctypes.data), C.c_void_p(found.ctypes.data), C.c_void_p(0))
        self.ctx._check(rc)
        return found.astype(bool), xyt, score

    def last_stats(self):
        out = np.zeros(2, dtype=np.int64)
        self.ctx._check(self.ctx.lib.cgmr_match_last_stats(self.ctx.h, C.c_void_p(out.ctypes.data)))
        pc = np.zeros(4, dtype=np.int64)
        self.ctx._check(self.ctx.lib.cgmr_match_last_path_counts(self.ctx.h, C.c_void_p(pc.ctypes.data)))
        rd = C.c_int64(0)
        self.ctx._check(self.ctx.lib.cgmr_match_last_redo_pairs(self.ctx.h, C.byref(rd)))
        sh = np.zeros(4, dtype=np.int64)
        self.ctx._check(self.ctx.lib.cgmr_match_last_launch_shape(self.ctx.h, C.c_void_p(sh.ctypes.data)))
        return {"pairs": int(out[0]), "slow_pairs": int(out[1]), "borrowed_pool_pairs": int(pc[0]),
                "redo_by_cause": {"grid": int(pc[1]), "window_or_points": int(pc[2]), "lists": int(pc[3])},
                "redo_pairs": int(rd.value),
                "launch": {"edt": int(sh[0]), "sort32": int(sh[1]), "lean": int(sh[2]), "split": int(sh[3])}}

    def closeScanMatching_dev(self, d_ranges_ref, d_ranges_cur, d_guess, n_pairs, d_xyt, d_score, d_found,   # noqa: N802
                              maxScore=0.15, d_nres=0):   # noqa: N803
        """Device-pointer variant (ints from ``tensor.data_ptr()``)."""
        rc = self.ctx.lib.cgmr_match_close_batch_dev(self.ctx.h, C.byref(self.cfg), C.c_int(n_pairs),
                                                     C.c_void_p(d_ranges_ref), C.c_void_p(d_ranges_cur),
                                                     C.c_void_p(d_guess), C.c_double(maxScore), C.c_void_p(d_xyt),
                                                     C.c_void_p(d_score), C.c_void_p(d_found), C.c_void_p(d_nres))
        self.ctx._check(rc)

    def scan_transforms(self, rel_xyt):
        """``cgmr_scan_transforms`` (host, libm, no GPU): ``rel_xyt`` (..., 3) = origin^-1 * v_k of reference scans ->
        (n, 4) = (cos, sin, tx, ty) of (origin^-1 * v_k) * laserPose, what ``closeScanMatchingVSet_dev`` takes."""
        rel = np.ascontiguousarray(rel_xyt, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((len(rel), 4))
        rc = self.ctx.lib.cgmr_scan_transforms(C.byref(self.cfg), C.c_int(len(rel)), C.c_void_p(rel.ctypes.data),
                                               C.c_void_p(out.ctypes.data))
        if rc != 0:
            raise CgmrError(rc, "cgmr_scan_transforms: bad argument")
        return out

    def closeScanMatchingVSet_dev(self, d_ranges_ref, d_ref_xform, d_ranges_cur, d_guess, n_pairs, n_ref_scans, d_xyt,   # noqa: N802
                                  d_score, d_found, maxScore=0.15, d_nres=0):   # noqa: N803
        """Device-pointer variant of ``closeScanMatchingVSetBatch`` (ints from ``tensor.data_ptr()``): ``d_ranges_ref``
        (P, S, n_beams) float32, ``d_ref_xform`` (P, S, 4) float64 from ``scan_transforms`` -- not the relative poses the
        host call takes --, ``d_ranges_cur`` (P, n_beams), ``d_guess`` (P, 3)."""
        rc = self.ctx.lib.cgmr_match_close_vset_batch_dev(self.ctx.h, C.byref(self.cfg), C.c_int(n_pairs), C.c_int(n_ref_scans),
                                                          C.c_void_p(d_ranges_ref), C.c_void_p(d_ref_xform),
                                                          C.c_void_p(d_ranges_cur), C.c_void_p(d_guess), C.c_double(maxScore),
                                                          C.c_void_p(d_xyt), C.c_void_p(d_score), C.c_void_p(d_found),
                                                          C.c_void_p(d_nres))
        self.ctx._check(rc)

    def last_kernel_seconds(self) -> float:
        s = C.c_double()
        self.ctx._check(self.ctx.lib.cgmr_match_last_kernel_seconds(self.ctx.h, C.byref(s)))
        return s.value


class LCScanMatcher(ScanMatcher):
    """The loop-closure matcher of GraphSLAM::init (src/slam/graph_slam.cpp:61-62): kernel (0.1, 0.5), grid
    [-35,35]^2 at 0.1 m -- plus the generic searches every ScanMatcher can run.  Scans are passed as
    ``(ranges, vertex_pose)`` pairs, the flat-array form of a g2o VertexSet with RobotLaser user data."""

    def __init__(self, ctx, n_beams, angle_min, angle_inc, max_range, laser_pose=(0.0, 0.0, 0.0)):
        super().__init__(ctx, n_beams, angle_min, angle_inc, max_range, laser_pose, resolution=0.1, kernel_range=0.5)
        self.initializeGrid((-35, -35), (35, 35), 0.1)


def smoke(ctx, oracle) -> None:
    """Tiny invocation checked against the oracle (used by __graft_entry__.smoke)."""
    from . import synth
    sp = synth.make_scan_pairs(6, seed=31)
    m = ScanMatcher(ctx, sp["n_beams"], sp["angle_min"], sp["angle_inc"], sp["max_range"])
    found, xyt, score = m.closeScanMatching(sp["ranges_ref"], sp["ranges_qry"], sp["guess"])
    xyt_o, score_o, found_o = oracle.close_scan_match_batch(sp["ranges_ref"], sp["ranges_qry"], sp["angle_min"],
                                                            sp["angle_inc"], sp["max_range"], [0, 0, 0], sp["guess"])
    if not (np.array_equal(found, found_o.astype(bool)) and np.array_equal(xyt, xyt_o) and np.array_equal(score, score_o)):
        raise CgmrError(-1, "matcher smoke: GPU result differs from the oracle")
    print(f"smoke ok: matcher {int(found.sum())}/{len(found)} pairs matched, bit-identical to the oracle")
