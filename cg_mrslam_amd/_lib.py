"""ctypes binding of libcgmr.so (include/cgmr.h).  Fails loudly when the HIP library is
missing -- there is deliberately no CPU path behind these calls."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

CGMR_E_CHOLESKY_BASE = -100
CGMR_E_TIMEOUT = -5


class CgmrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"cgmr error {code}: {msg}")
        self.code = code


def library_path() -> str:
    # CGMR_LIB: load another build of the same library (A/B runs of kernel variants); default = the in-tree build
    return os.environ.get("CGMR_LIB") or os.path.join(_HERE, "libcgmr.so")


def build_library(force: bool = False) -> str:
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "-s", "clean"])
    subprocess.check_call(["make", "-C", csrc, "-s", "-j8"])
    return library_path()


_SYMBOLS = [
    "cgmr_version", "cgmr_ctx_create", "cgmr_ctx_destroy", "cgmr_last_error", "cgmr_ctx_synchronize",
    "cgmr_gn_optimize", "cgmr_gn_optimize_dev", "cgmr_gn_symbolic_info", "cgmr_gn_last_timing",
    "cgmr_set_profiling", "cgmr_gn_kernel_times", "cgmr_gn_kernel_times_ex",
    "cgmr_match_response", "cgmr_match_response_batch", "cgmr_close_scan_matching_cov", "cgmr_match_response_information",
    "cgmr_refine_params_default", "cgmr_match_refine", "cgmr_match_refine_batch", "cgmr_close_scan_matching_refined",
    "cgmr_match_polish_batch", "cgmr_scan_matching_lc_polished_batch", "cgmr_scan_matching_lc_polished",
    "cgmr_global_matching_polished_batch", "cgmr_global_matching_polished",
    "cgmr_marginals_joint", "cgmr_marginals_pairs", "cgmr_relative_covariance",
    "cgmr_marginals_joint_typed", "cgmr_marginals_pairs_typed", "cgmr_observation_covariance",
    "cgmr_gnc_params_default", "cgmr_gnc_optimize", "cgmr_gnc_optimize_dev", "cgmr_gnc_last_stats",
    "cgmr_graph_set_edge_gnc", "cgmr_graph_set_received_gnc", "cgmr_graph_optimize_gnc", "cgmr_graph_gnc_weights",
    "cgmr_graph_keep_gnc_weights", "cgmr_graph_set_condensed_gnc",
    "cgmr_chordal_initialize", "cgmr_chordal_initialize_dev", "cgmr_chordal_initialize_typed",
    "cgmr_chordal_initialize_typed_dev", "cgmr_initial_guess",
    "cgmr_gn_optimize_mixture", "cgmr_gn_optimize_mixture_dev", "cgmr_lm_optimize_mixture", "cgmr_lm_optimize_mixture_dev",
    "cgmr_dl_optimize_mixture", "cgmr_dl_optimize_mixture_dev", "cgmr_mixture_select",
    "cgmr_closure_consistency", "cgmr_max_clique_greedy", "cgmr_switches",
    "cgmr_closure_consistency_exact", "cgmr_max_clique_exact",
    "cgmr_closure_consistency_inter", "cgmr_closure_consistency_inter_exact",
    "cgmr_match_close_vset_batch_dev", "cgmr_scan_transforms",
    "cgmr_jcbb_dense", "cgmr_joint_compatibility",
    "cgmr_condense_tree", "cgmr_min_spanning_tree",
    "cgmr_remove_nodes",
    "cgmr_scan_information", "cgmr_scan_prune", "cgmr_scan_info_last_stats",
]

JOINT_MAX_QUERIES = 2048      # include/cgmr.h: CGMR_JOINT_MAX_QUERIES (unique query vertices of a joint / pairs call)
REMOVE_MAX_DEGREE = 16        # include/cgmr.h: CGMR_REMOVE_MAX_DEGREE (distinct neighbours of a vertex remove_nodes takes out)
SCAN_INFO_DEFAULT_SCRATCH = 1 << 30   # include/cgmr.h: CGMR_SCAN_INFO_DEFAULT_SCRATCH (bytes of scan windows alive at one time)
TREE_MAX_NODES = 1025         # include/cgmr.h: CGMR_TREE_MAX_NODES (the gauge and the unique requested vertices of a condense_tree call)
PCM_MAX_CLOSURES = 1024       # include/cgmr.h: CGMR_PCM_MAX_CLOSURES (candidates of a consistency call, vertices of a clique call)
EXACT_DEFAULT_NODE_LIMIT = 512    # include/cgmr.h: CGMR_EXACT_DEFAULT_NODE_LIMIT (nodes per root and round of the exact clique search)
EXACT_ROUNDS = 2              # csrc/pcm_device.h: CGMR_EXACT_ROUNDS (a call expands at most n * EXACT_ROUNDS * node_limit nodes)
JC_MAX_OBS = 32               # include/cgmr.h: CGMR_JC_MAX_OBS (observations of a joint-compatibility call)
JC_MAX_LANDMARKS = 256        # include/cgmr.h: CGMR_JC_MAX_LANDMARKS (its candidate landmarks)
JC_ROUNDS = 2                 # csrc/jcbb_device.h: CGMR_JC_ROUNDS (a call makes at most roots * JC_ROUNDS * node_limit joint tests)
JC_DEFAULT_NODE_LIMIT = 2048  # include/cgmr.h: CGMR_JC_DEFAULT_NODE_LIMIT (joint tests per root and round)
# scipy.stats.chi2.ppf(0.99, k) for k = 1 .. 64 at index k (index 0 unused): the thresholds of a joint-compatibility call at the
# 0.99 level, by degrees of freedom; entry 3 is GraphSLAM.GAMMA_99
JC_GAMMA_99 = (
    0.0, 6.6348966010212145, 9.21034037197618, 11.344866730144373, 13.276704135987622,
    15.08627246938899, 16.811893829770927, 18.475306906582357, 20.090235029663233, 21.665994333461924,
    23.209251158954356, 24.724970311318277, 26.216967305535853, 27.68824961045705, 29.141237740672796,
    30.57791416689249, 31.999926908815176, 33.40866360500461, 34.805305734705065, 36.19086912927004,
    37.56623478662507, 38.93217268351607, 40.289360437593864, 41.638398118858476, 42.97982013935165,
    44.31410489621915, 45.64168266628317, 46.962942124751436, 48.27823577031548, 49.58788447289881,
    50.89218131151707, 52.19139483319193, 53.48577183623535, 54.77553976011035, 56.06090874778906,
    57.3420734338592, 58.61921450168706, 59.89250004508689, 61.1620867636897, 62.4281210161849,
    63.690739751564465, 64.9500713352112, 66.20623628399322, 67.45934792232582, 68.7095129693454,
    69.95683206583814, 71.20140024831149, 72.44330737654823, 73.68263852010573, 74.91947430847816,
    76.1538912490127, 77.38596201613736, 78.6157557150025, 79.84333812225145, 81.0687719062971,
    82.29211682919967, 83.51342993198946, 84.73276570506393, 85.95017624510335, 87.16571139978757,
    88.37941890144937, 89.59134449068712, 90.80153203083871, 92.01002361413214, 93.21685966023843,
)


def declared_symbols():
    """Every entry point include/cgmr.h declares (parsed from the header)."""
    import re
    hdr = os.path.join(os.path.dirname(_HERE), "include", "cgmr.h")
    txt = open(hdr).read()
    return sorted(set(re.findall(r"\b(cgmr_[a-z0-9_]+)\s*\(", txt)))


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise CgmrError(-2, f"{path} not found: build it with __graft_entry__.build() "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # PyTorch-ROCm bundles its own libamdhip64; two HIP runtimes in one process cannot both own the GPU
    # ("No HIP GPUs are available" from whichever initialises second).  Importing torch first makes the
    # dynamic loader resolve libcgmr.so's libamdhip64 dependency to the copy torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    lib.cgmr_last_error.restype = C.c_char_p
    lib.cgmr_ctx_destroy.restype = None
    lib.cgmr_matcher_config_close.restype = None
    _LIB = lib
    return lib


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


class LmParams(C.Structure):
    """cgmr_lm_params (include/cgmr.h): g2o's OptimizationAlgorithmLevenberg properties."""
    _fields_ = [("tau", C.c_double), ("initial_lambda", C.c_double), ("max_trials", C.c_int32),
                ("good_step_lower", C.c_double), ("good_step_upper", C.c_double)]


LM_DEFAULTS = dict(tau=1e-5, initial_lambda=-1.0, max_trials=10, good_step_lower=1.0 / 3, good_step_upper=2.0 / 3)


def lm_params(**kw) -> LmParams:
    """An LmParams with g2o's defaults for whatever ``kw`` does not name."""
    bad = set(kw) - set(LM_DEFAULTS)
    if bad:
        raise TypeError(f"unknown Levenberg-Marquardt parameter(s): {sorted(bad)}")
    v = dict(LM_DEFAULTS, **kw)
    return LmParams(float(v["tau"]), float(v["initial_lambda"]), int(v["max_trials"]), float(v["good_step_lower"]),
                    float(v["good_step_upper"]))


class DlParams(C.Structure):
    """cgmr_dl_params (include/cgmr.h): g2o's OptimizationAlgorithmDogleg properties."""
    _fields_ = [("initial_delta", C.c_double), ("max_trials", C.c_int32), ("initial_lambda", C.c_double),
                ("lambda_factor", C.c_double)]


DL_DEFAULTS = dict(initial_delta=1e4, max_trials=100, initial_lambda=1e-7, lambda_factor=10.0)
DL_STEP_SD, DL_STEP_GN, DL_STEP_DL = 1, 2, 3      # include/cgmr.h: CGMR_DL_STEP_*


def dl_params(**kw) -> DlParams:
    """A DlParams with g2o's defaults for whatever ``kw`` does not name."""
    bad = set(kw) - set(DL_DEFAULTS)
    if bad:
        raise TypeError(f"unknown dogleg parameter(s): {sorted(bad)}")
    v = dict(DL_DEFAULTS, **kw)
    return DlParams(float(v["initial_delta"]), int(v["max_trials"]), float(v["initial_lambda"]), float(v["lambda_factor"]))


def dl_params_checked(kw) -> DlParams:
    """dl_params(**kw), with the values the library accepts (ValueError otherwise): max_trials >= 1; initial_delta,
    initial_lambda finite and > 0; lambda_factor finite and > 1."""
    p = dl_params(**kw)
    fin = all(math.isfinite(v) for v in (p.initial_delta, p.initial_lambda, p.lambda_factor))
    if not (fin and p.max_trials >= 1 and p.initial_delta > 0 and p.initial_lambda > 0 and p.lambda_factor > 1):
        raise ValueError("dogleg parameters: max_trials >= 1, initial_delta / initial_lambda > 0, lambda_factor > 1, all finite")
    return p


class GncParams(C.Structure):
    """cgmr_gnc_params (include/cgmr.h): graduated non-convexity."""
    _fields_ = [("loss", C.c_int32), ("mu_factor", C.c_double), ("max_outer", C.c_int32), ("inner_iters", C.c_int32),
                ("outer_per_wait", C.c_int32), ("barc_sq", C.c_void_p), ("default_barc_sq", C.c_double),
                ("known_inlier", C.c_void_p), ("weight_out", C.c_void_p), ("edge_chi2_out", C.c_void_p)]


GNC_TLS, GNC_GM = 0, 1                            # include/cgmr.h: CGMR_GNC_*
GNC_LOSSES = {"tls": GNC_TLS, "gm": GNC_GM}
GNC_DEFAULTS = dict(mu_factor=1.4, inner_iters=1, outer_per_wait=8)


def gnc_loss_code(loss) -> int:
    """CGMR_GNC_* of a loss given by name ("tls", "gm", any case) or by code; an unknown code passes (the library refuses it)."""
    if isinstance(loss, str):
        if loss.lower() not in GNC_LOSSES:
            raise ValueError(f"unknown GNC loss {loss!r}; one of {sorted(GNC_LOSSES)}")
        return GNC_LOSSES[loss.lower()]
    return int(loss)


def gnc_known_mask(known_inliers, n):
    """uint8 [n] from an index list or a mask of length n (None: no known inlier)."""
    mask = np.zeros(n, dtype=np.uint8)
    if known_inliers is None:
        return mask
    k = np.asarray(known_inliers)
    if k.dtype == np.bool_ or (k.dtype == np.uint8 and k.shape == (n,)):
        if k.shape != (n,):
            raise ValueError(f"known-inlier mask: {k.shape} given for {n} edges")
        mask[:] = k != 0
    elif k.size:
        k = k.astype(np.int64).reshape(-1)
        if k.min() < 0 or k.max() >= n:
            raise ValueError("known-inlier index out of range")
        mask[k] = 1
    return mask


class Robust(C.Structure):
    """cgmr_robust (include/cgmr.h): the robust kernels of one call."""
    _fields_ = [("kind", C.c_void_p), ("delta", C.c_void_p), ("default_kind", C.c_int32), ("default_delta", C.c_double),
                ("edge_chi2_out", C.c_void_p), ("weight_out", C.c_void_p)]


class FactorTypes(C.Structure):
    """cgmr_factor_types (include/cgmr.h): the vertex and edge kinds of one typed call."""
    _fields_ = [("vertex_kind", C.c_void_p), ("edge_kind", C.c_void_p)]


class Mixture(C.Structure):
    """cgmr_mixture (include/cgmr.h): the components of the edges of one mixture call."""
    _fields_ = [("comp_ptr", C.c_void_p), ("comp_meas", C.c_void_p), ("comp_info", C.c_void_p), ("comp_weight", C.c_void_p),
                ("selected_out", C.c_void_p)]


def mixture_arrays(mixture, nE):
    """(Mixture or None, selected int32 [nE], the arrays it points into) from ``mixture`` = (comp_ptr [nE + 1], comp_meas [nC, 3],
    comp_info [nC, 6], comp_weight [nC]) or None.  Shapes are checked here; the values by the library."""
    sel = np.zeros(nE, dtype=np.int32)
    if mixture is None:
        return None, sel, None
    cp, cm, ci, cw = mixture
    cp = np.ascontiguousarray(cp, dtype=np.int32).reshape(-1)
    if cp.shape != (nE + 1,):
        raise ValueError(f"mixture: comp_ptr has {cp.shape[0]} entries for {nE} edges (nE + 1 expected)")
    nC = max(int(cp.max()), 0) if cp.size else 0
    cm = np.ascontiguousarray(cm, dtype=np.float64).reshape(-1, 3)
    ci = np.ascontiguousarray(ci, dtype=np.float64).reshape(-1, 6)
    cw = np.ascontiguousarray(cw, dtype=np.float64).reshape(-1)
    if cm.shape[0] < nC or ci.shape[0] < nC or cw.shape[0] < nC:
        raise ValueError(f"mixture: comp_ptr names {nC} components, comp_meas / comp_info / comp_weight hold "
                         f"{cm.shape[0]} / {ci.shape[0]} / {cw.shape[0]}")
    keep = (cp, cm, ci, cw, sel)
    return Mixture(*(a.ctypes.data if a.size else None for a in keep)), sel, keep


# include/cgmr.h: CGMR_VERTEX_* / CGMR_EDGE_*
VERTEX_SE2, VERTEX_XY = 0, 1
EDGE_SE2, EDGE_SE2_XY, EDGE_BEARING_SE2_XY, EDGE_PRIOR_SE2, EDGE_PRIOR_SE2_XY = 0, 1, 2, 3, 4


def factor_types(vertex_kind, edge_kind, nV, nE):
    """(FactorTypes, the arrays it points into) for per-vertex / per-edge kinds (None: all zero)."""
    vk = None if vertex_kind is None else np.ascontiguousarray(vertex_kind, dtype=np.uint8).reshape(-1)
    ek = None if edge_kind is None else np.ascontiguousarray(edge_kind, dtype=np.uint8).reshape(-1)
    if vk is not None and vk.shape != (nV,):
        raise ValueError(f"vertex kinds: {vk.shape[0]} given for {nV} vertices")
    if ek is not None and ek.shape != (nE,):
        raise ValueError(f"edge kinds: {ek.shape[0]} given for {nE} edges")
    ft = FactorTypes(vk.ctypes.data if vk is not None and nV else None, ek.ctypes.data if ek is not None and nE else None)
    return ft, (vk, ek)


def chordal_stages(stages) -> int:
    """The ``stages`` argument of cgmr_chordal_initialize from 1 / 2 / 3 or "r" / "t" / "rt" (include/cgmr.h: CGMR_CHORDAL_*)."""
    if isinstance(stages, str):
        if not stages or set(stages) - set("rt"):
            raise ValueError(f"chordal stages {stages!r}: some of 'r' (rotation) and 't' (translation)")
        return (1 if "r" in stages else 0) | (2 if "t" in stages else 0)
    if isinstance(stages, (bool, np.bool_)) or not isinstance(stages, (int, np.integer)) or not 1 <= int(stages) <= 3:
        raise ValueError(f"chordal stages must be 1, 2 or 3, got {stages!r}")
    return int(stages)


# g2o's robust kernels by their C codes (include/cgmr.h: CGMR_RK_*)
ROBUST_KINDS = {"none": 0, "huber": 1, "pseudohuber": 2, "cauchy": 3, "welsch": 4, "tukey": 5, "saturated": 6, "dcs": 7}


def robust_code(kind) -> int:
    """The C code of a robust kernel given by name (g2o's, any case: "Huber", "PseudoHuber", "DCS", ...) or by code."""
    if isinstance(kind, str):
        key = kind.lower().replace("_", "").replace("-", "")
        if key.startswith("robustkernel"):
            key = key[len("robustkernel"):]
        if key not in ROBUST_KINDS:
            raise ValueError(f"unknown robust kernel {kind!r}; one of {sorted(ROBUST_KINDS)}")
        return ROBUST_KINDS[key]
    if isinstance(kind, (bool, np.bool_)) or not isinstance(kind, (int, np.integer)) or not 0 <= int(kind) <= 7:
        raise ValueError(f"robust kernel code must be 0..7, got {kind!r}")
    return int(kind)


def robust_arrays(kind, delta, n):
    """(codes uint8 [n] or None, deltas float64 [n] or None, uniform code, uniform delta), checked as the library checks them:
    a known kind, and a finite delta > 0 for every kind but "none".  Raises ValueError."""
    if isinstance(kind, (str, int, np.integer)):
        codes, code0 = None, robust_code(kind)
    else:
        arr = np.asarray(kind)
        if arr.dtype.kind in "iu":                                 # codes: checked in one go
            if arr.size and (arr.min() < 0 or arr.max() > 7):
                raise ValueError("robust kernel codes must be 0..7")
            codes = arr.astype(np.uint8).reshape(-1)
        else:
            codes = np.array([robust_code(k) for k in arr.tolist()], dtype=np.uint8)
        code0 = 0
        if codes.shape != (n,):
            raise ValueError(f"per-edge robust kinds: {codes.shape[0]} given for {n} edges")
    if np.ndim(delta) == 0:
        deltas, delta0 = None, float(delta)
    else:
        deltas, delta0 = np.ascontiguousarray(delta, dtype=np.float64), 1.0
        if deltas.shape != (n,):
            raise ValueError(f"per-edge robust deltas: {deltas.shape} given for {n} edges")
    k = codes if codes is not None else np.full(n if deltas is not None else 1, code0, dtype=np.uint8)
    d = deltas if deltas is not None else np.full(k.shape, delta0)
    bad = (k != 0) & ~(np.isfinite(d) & (d > 0))
    if bad.any():
        raise ValueError(f"robust kernel delta must be finite and > 0 (edge {int(np.flatnonzero(bad)[0])})")
    return codes, deltas, code0, delta0


class Context:
    """One cgmr context = one HIP device + one stream (include/cgmr.h)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.cgmr_ctx_create(C.c_int(device), C.c_void_p(stream or 0), C.byref(h))
        if rc != 0:
            raise CgmrError(rc, "cgmr_ctx_create failed (no usable gfx950 device?)")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.cgmr_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, allow_cholesky=False):
        if rc == 0:
            return rc
        if allow_cholesky and rc <= CGMR_E_CHOLESKY_BASE:
            return rc
        raise CgmrError(rc, self.lib.cgmr_last_error(self.h).decode())

    def synchronize(self):
        self._check(self.lib.cgmr_ctx_synchronize(self.h))

    # ------------------------------------------------------------------ GN / Levenberg-Marquardt / dogleg
    @staticmethod
    def _problem(poses, fixed, ef, et, meas, info):
        """The six arrays of a problem as the library reads them.  ``poses`` a host array: everything is host memory, and the
        call writes to a copy of the poses; ``poses`` a (device pointer, nV) pair: meas / info are device pointers too.
        Returns (nV, the poses' copy or None, the six ctypes arguments, the arrays they point into)."""
        keep = [np.ascontiguousarray(fixed, dtype=np.uint8), np.ascontiguousarray(ef, dtype=np.int32),
                np.ascontiguousarray(et, dtype=np.int32)]
        if isinstance(poses, tuple):
            (d_poses, nV), p = poses, None
            dev = [C.c_void_p(d_poses), C.c_void_p(meas), C.c_void_p(info)]
        else:
            p = np.ascontiguousarray(poses, dtype=np.float64).copy()
            keep += [p, np.ascontiguousarray(meas, dtype=np.float64), np.ascontiguousarray(info, dtype=np.float64)]
            nV, dev = p.shape[0], [_ptr(a) for a in keep[3:]]
        fx, f, t = (_ptr(a) for a in keep[:3])
        return nV, p, (dev[0], fx, C.c_int(len(keep[1])), f, t, dev[1], dev[2]), keep

    @staticmethod
    def _records(iters, n_int):
        """The outputs of a call: chi2 [iters + 1]; for a trust-region algorithm (``n_int`` not None) one float64 record
        [iters] (lambdas / deltas) and ``n_int`` int32 ones (trials, steps)."""
        if n_int is None:
            return [np.zeros(iters + 1)]
        return [np.zeros(iters + 1), np.zeros(iters)] + [np.zeros(iters, dtype=np.int32) for _ in range(n_int)]

    def _optimize(self, entry, problem, iters, prm=None, n_int=None, rk=False, allow_fail=False, ft=None):
        """One cgmr_*_optimize* call on ``problem`` (the arguments of _problem).  ``prm``: the parameters of a trust-region
        algorithm, which also returns its iterations done; ``rk``: a cgmr_robust, None for a null one, False for an entry
        point that takes none.  Returns (status, [the poses,] chi2, [records, iterations done])."""
        nV, p, (poses, fixed, nE, ef, et, meas, info), _keep = self._problem(*problem)
        rec, done = self._records(iters, n_int), C.c_int32(0)
        args = [self.h, C.c_int(nV), poses, fixed, nE, ef, et, meas, info, C.c_int(iters)]
        if prm is not None:
            args.append(C.byref(prm))
        args += [_ptr(a) for a in rec]
        if prm is not None:
            args.append(C.byref(done))
        if ft is not None:                                        # (the typed entry points: cgmr_factor_types in front of rk)
            args.append(C.byref(ft))
        if rk is not False:
            args.append(C.byref(rk) if rk is not None else C.c_void_p(0))
        rc = getattr(self.lib, entry)(*args)
        self._check(rc, allow_cholesky=allow_fail)
        return (rc,) + (() if p is None else (p,)) + tuple(rec) + (() if prm is None else (int(done.value),))

    def gn_optimize(self, poses, fixed, ef, et, meas, info, iters, raise_on_cholesky=True):
        """Host arrays in, host arrays out.  Returns (status, poses, chi2[iters+1])."""
        return self._optimize("cgmr_gn_optimize", (poses, fixed, ef, et, meas, info), iters, allow_fail=not raise_on_cholesky)

    def gn_optimize_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters,
                        raise_on_cholesky=True):
        """Device pointers (ints) for poses/meas/info, host numpy for the structure."""
        return self._optimize("cgmr_gn_optimize_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                              allow_fail=not raise_on_cholesky)

    def lm_optimize(self, poses, fixed, ef, et, meas, info, iters, **params):
        """Levenberg-Marquardt (cgmr_lm_optimize, g2o's OptimizationAlgorithmLevenberg); ``params``: tau, initial_lambda,
        max_trials, good_step_lower, good_step_upper (g2o's defaults otherwise).  Host arrays in and out.  Returns
        (status, poses, chi2[iters+1], lambdas[iters], trials[iters], iters_done); termination is status 0 with
        iters_done < iters, never a Cholesky status."""
        return self._optimize("cgmr_lm_optimize", (poses, fixed, ef, et, meas, info), iters, lm_params(**params), 1)

    def lm_optimize_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, **params):
        """Device pointers (ints) for poses/meas/info, host numpy for the structure.  Returns
        (status, chi2[iters+1], lambdas[iters], trials[iters], iters_done)."""
        return self._optimize("cgmr_lm_optimize_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                              lm_params(**params), 1)

    # ------------------------------------------------------------------ robust kernels
    @staticmethod
    def _robust(kind, delta, n, d_kind_ptr=None, d_delta_ptr=None):
        """cgmr_robust for host (kind / delta: name or code / scalar, or per-edge arrays) or device (d_*_ptr) inputs, with the
        statistics arrays it fills.  Returns (struct, e2 [n], weights [n], the arrays the struct points into)."""
        codes, deltas, code0, delta0 = robust_arrays(kind, delta, n)
        e2, w = np.zeros(n), np.zeros(n)
        rk = Robust(None, None, code0, delta0, e2.ctypes.data if n else None, w.ctypes.data if n else None)
        rk.kind = d_kind_ptr if d_kind_ptr is not None else (codes.ctypes.data if codes is not None and n else None)
        rk.delta = d_delta_ptr if d_delta_ptr is not None else (deltas.ctypes.data if deltas is not None and n else None)
        return rk, e2, w, (codes, deltas)

    def gn_optimize_robust(self, poses, fixed, ef, et, meas, info, iters, kind="none", delta=1.0, raise_on_cholesky=True):
        """gn_optimize with robust kernels (cgmr_gn_optimize_robust): ``kind`` a name, a code or per-edge array of either,
        ``delta`` a scalar or per-edge array.  Returns (status, poses, robust chi2[iters+1], e2 [nE], weights [nE]), the last
        two at the returned estimate."""
        rk, e2, w, _keep = self._robust(kind, delta, len(ef))
        return self._optimize("cgmr_gn_optimize_robust", (poses, fixed, ef, et, meas, info), iters, rk=rk,
                              allow_fail=not raise_on_cholesky) + (e2, w)

    def gn_optimize_robust_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, kind="none", delta=1.0,
                               d_kind_ptr=None, d_delta_ptr=None, raise_on_cholesky=True):
        """gn_optimize_dev with robust kernels: per-edge kinds (uint8) / deltas (float64) as device pointers, or a uniform
        ``kind`` / ``delta``.  Returns (status, robust chi2[iters+1], e2 [nE], weights [nE])."""
        rk, e2, w, _keep = self._robust(kind, delta, len(ef), d_kind_ptr, d_delta_ptr)
        return self._optimize("cgmr_gn_optimize_robust_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                              rk=rk, allow_fail=not raise_on_cholesky) + (e2, w)

    def lm_optimize_robust(self, poses, fixed, ef, et, meas, info, iters, kind="none", delta=1.0, **params):
        """lm_optimize with robust kernels (``kind`` / ``delta`` as gn_optimize_robust).  Returns (status, poses, robust
        chi2[iters+1], lambdas[iters], trials[iters], iters_done, e2 [nE], weights [nE])."""
        rk, e2, w, _keep = self._robust(kind, delta, len(ef))
        return self._optimize("cgmr_lm_optimize_robust", (poses, fixed, ef, et, meas, info), iters, lm_params(**params), 1,
                              rk=rk) + (e2, w)

    def lm_optimize_robust_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, kind="none", delta=1.0,
                               d_kind_ptr=None, d_delta_ptr=None, **params):
        """lm_optimize_dev with robust kernels (as gn_optimize_robust_dev).  Returns (status, robust chi2[iters+1],
        lambdas[iters], trials[iters], iters_done, e2 [nE], weights [nE])."""
        rk, e2, w, _keep = self._robust(kind, delta, len(ef), d_kind_ptr, d_delta_ptr)
        return self._optimize("cgmr_lm_optimize_robust_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                              lm_params(**params), 1, rk=rk) + (e2, w)

    def lm_last_stats(self):
        """The last lm_optimize* call: dict(host_waits, trials)."""
        out = np.zeros(2, dtype=np.int64)
        self._check(self.lib.cgmr_lm_last_stats(self.h, _ptr(out)))
        return dict(host_waits=int(out[0]), trials=int(out[1]))

    # ------------------------------------------------------------------ dogleg
    def dl_optimize(self, poses, fixed, ef, et, meas, info, iters, kind=None, delta=1.0, raise_on_fail=True, **params):
        """Dogleg (cgmr_dl_optimize, g2o's OptimizationAlgorithmDogleg); ``params``: initial_delta, max_trials,
        initial_lambda, lambda_factor (g2o's defaults otherwise); ``kind`` / ``delta``: robust kernels as gn_optimize_robust
        takes them (None: the plain call).  Host arrays in and out.  Returns (status, poses, chi2[iters+1], deltas[iters],
        trials[iters], steps[iters], iters_done), with e2 [nE] and weights [nE] appended when ``kind`` is given.
        Termination is status 0 with iters_done < iters; g2o's Fail in iteration i is CGMR_E_CHOLESKY_BASE - i (raised
        unless ``raise_on_fail`` is False)."""
        prm = dl_params(**params)
        rk, e2, w, _keep = self._robust(kind, delta, len(ef)) if kind is not None else (None, None, None, None)
        out = self._optimize("cgmr_dl_optimize", (poses, fixed, ef, et, meas, info), iters, prm, 2, rk=rk,
                             allow_fail=not raise_on_fail)
        return out + (e2, w) if kind is not None else out

    def dl_optimize_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, kind=None, delta=1.0,
                        d_kind_ptr=None, d_delta_ptr=None, raise_on_fail=True, **params):
        """Device pointers (ints) for poses/meas/info, host numpy for the structure; robust kernels as
        gn_optimize_robust_dev takes them (``kind`` None and no device arrays: the plain call).  Returns (status,
        chi2[iters+1], deltas[iters], trials[iters], steps[iters], iters_done), with e2 and weights appended when robust."""
        prm = dl_params(**params)
        robust = kind is not None or d_kind_ptr is not None or d_delta_ptr is not None
        rk, e2, w, _keep = self._robust("none" if kind is None else kind, delta, len(ef), d_kind_ptr, d_delta_ptr) if robust \
            else (None, None, None, None)
        out = self._optimize("cgmr_dl_optimize_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters, prm, 2,
                             rk=rk, allow_fail=not raise_on_fail)
        return out + (e2, w) if robust else out

    # ------------------------------------------------------------------ graduated non-convexity
    def _gnc(self, entry, problem, max_outer, loss, barc_sq, known_inliers, vertex_kind, edge_kind, raise_on_cholesky, params):
        bad = set(params) - set(GNC_DEFAULTS)
        if bad:
            raise TypeError(f"unknown GNC parameter(s): {sorted(bad)}")
        v = dict(GNC_DEFAULTS, **params)
        nV, p, (poses, fixed, nE, ef, et, meas, info), _keep = self._problem(*problem)
        n = nE.value
        typed = vertex_kind is not None or edge_kind is not None
        ft, _keep_ft = factor_types(vertex_kind, edge_kind, nV, n) if typed else (None, None)
        c_arr, c0 = None, 0.0
        if barc_sq is not None and np.ndim(barc_sq) == 0:
            c0 = float(barc_sq)
            if not c0 > 0 or not math.isfinite(c0):            # (<= 0 would select the default in the C struct)
                raise CgmrError(-1, "gnc_optimize: barc_sq must be finite and > 0")
        elif barc_sq is not None:
            c_arr = np.ascontiguousarray(barc_sq, dtype=np.float64).reshape(-1)
            if c_arr.shape != (n,):
                raise ValueError(f"barc_sq: {c_arr.shape[0]} given for {n} edges")
        known = gnc_known_mask(known_inliers, n) if known_inliers is not None else None
        w, e2 = np.zeros(n), np.zeros(n)
        mo = max(int(max_outer), 1)
        mu, cost, partial, done = np.zeros(mo), np.zeros(mo + 1), np.zeros(mo, dtype=np.int32), C.c_int32(0)
        prm = GncParams(gnc_loss_code(loss), float(v["mu_factor"]), int(max_outer), int(v["inner_iters"]), int(v["outer_per_wait"]),
                        c_arr.ctypes.data if c_arr is not None and n else None, c0,
                        known.ctypes.data if known is not None and n else None, w.ctypes.data if n else None,
                        e2.ctypes.data if n else None)
        rc = getattr(self.lib, entry)(self.h, C.c_int(nV), poses, fixed, nE, ef, et, meas, info,
                                      C.byref(ft) if ft is not None else C.c_void_p(0), C.byref(prm), _ptr(mu), _ptr(cost),
                                      _ptr(partial), C.byref(done))
        self._check(rc, allow_cholesky=not raise_on_cholesky)
        out = dict(status=rc, mu=mu, cost=cost, partial=partial, outer_done=int(done.value), weights=w, edge_chi2=e2)
        if p is not None:
            out["poses"] = p
        return out

    def gnc_optimize(self, poses, fixed, ef, et, meas, info, max_outer=100, loss="tls", barc_sq=None, known_inliers=None,
                     vertex_kind=None, edge_kind=None, raise_on_cholesky=True, **params):
        """Graduated non-convexity (cgmr_gnc_optimize): ``loss`` "tls" or "gm"; ``barc_sq`` a scalar, a per-edge array or None
        (the chi2 0.99 quantile of each factor's dimension); ``known_inliers`` an index list or mask; ``vertex_kind`` /
        ``edge_kind`` as the typed calls; ``params``: mu_factor, inner_iters, outer_per_wait.  Host arrays in and out.  Returns a
        dict: status, poses, mu [max_outer], cost [max_outer + 1], partial [max_outer], outer_done, weights [nE], edge_chi2 [nE]."""
        return self._gnc("cgmr_gnc_optimize", (poses, fixed, ef, et, meas, info), max_outer, loss, barc_sq, known_inliers,
                         vertex_kind, edge_kind, raise_on_cholesky, params)

    def gnc_optimize_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, max_outer=100, loss="tls", barc_sq=None,
                         known_inliers=None, vertex_kind=None, edge_kind=None, raise_on_cholesky=True, **params):
        """gnc_optimize on device pointers for poses / meas / info (everything per edge stays host memory): the same dict
        without the poses."""
        return self._gnc("cgmr_gnc_optimize_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), max_outer, loss,
                         barc_sq, known_inliers, vertex_kind, edge_kind, raise_on_cholesky, params)

    def gnc_last_stats(self):
        """The last gnc_optimize* call: dict(host_waits, inner_iterations)."""
        out = np.zeros(2, dtype=np.int64)
        self._check(self.lib.cgmr_gnc_last_stats(self.h, _ptr(out)))
        return dict(host_waits=int(out[0]), inner_iterations=int(out[1]))

    # ------------------------------------------------------------------ starting points
    def _chordal(self, problem, stages, vertex_kind, edge_kind, raise_on_cholesky):
        nV, p, (poses, fixed, nE, ef, et, meas, info), _keep = self._problem(*problem)
        typed = vertex_kind is not None or edge_kind is not None
        ft, _keep_ft = factor_types(vertex_kind, edge_kind, nV, nE.value) if typed else (None, None)
        entry = "cgmr_chordal_initialize" + ("_typed" if typed else "") + ("_dev" if p is None else "")
        chi2, counts = np.zeros(2), np.zeros(3, dtype=np.int32)
        args = [self.h, C.c_int(nV), poses, fixed, nE, ef, et, meas, info, C.c_int(chordal_stages(stages)), _ptr(chi2), _ptr(counts)]
        if typed:
            args.append(C.byref(ft))
        rc = getattr(self.lib, entry)(*args)
        self._check(rc, allow_cholesky=not raise_on_cholesky)
        out = dict(status=rc, chi2=chi2, counts=counts)
        if p is not None:
            out["poses"] = p
        return out

    def chordal_initialize(self, poses, fixed, ef, et, meas, info, stages=3, vertex_kind=None, edge_kind=None,
                           raise_on_cholesky=True):
        """Chordal initialisation (cgmr_chordal_initialize[_typed]): a starting point from two linear problems, whatever the
        estimates passed in.  ``stages``: 1 / "r" the headings, 2 / "t" the positions with the headings held, 3 / "rt" both;
        ``vertex_kind`` / ``edge_kind`` as the typed calls.  Host arrays in and out.  Returns a dict: status, poses, chi2 [2] (the
        SE(2) chi2 at the start and at the result), counts [3] (vertices solved in the rotation stage, in the translation
        stage, degenerate headings)."""
        return self._chordal((poses, fixed, ef, et, meas, info), stages, vertex_kind, edge_kind, raise_on_cholesky)

    def chordal_initialize_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, stages=3, vertex_kind=None,
                               edge_kind=None, raise_on_cholesky=True):
        """chordal_initialize on device pointers for poses / meas / info: the same dict without the poses."""
        return self._chordal(((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), stages, vertex_kind, edge_kind,
                             raise_on_cholesky)

    def initial_guess(self, poses, fixed, ef, et, meas):
        """g2o's spanning-tree guess (cgmr_initial_guess): breadth-first from the fixed vertices over the edges.  Host arrays
        in, the new poses out; a vertex that is not reached keeps its estimate.  No device work."""
        p = np.ascontiguousarray(poses, dtype=np.float64).copy()
        fx, f, t = (np.ascontiguousarray(a, dtype=d) for a, d in ((fixed, np.uint8), (ef, np.int32), (et, np.int32)))
        m = np.ascontiguousarray(meas, dtype=np.float64)
        rc = self.lib.cgmr_initial_guess(C.c_int(p.shape[0]), _ptr(p), _ptr(fx), C.c_int(len(f)), _ptr(f), _ptr(t), _ptr(m))
        if rc != 0:
            raise CgmrError(rc, "cgmr_initial_guess: a null or negative argument, or an edge index out of range")
        return p

    def dl_last_stats(self):
        """The last dl_optimize* call: dict(host_waits, trials, factorisations)."""
        out = np.zeros(3, dtype=np.int64)
        self._check(self.lib.cgmr_dl_last_stats(self.h, _ptr(out)))
        return dict(host_waits=int(out[0]), trials=int(out[1]), factorisations=int(out[2]))

    # ------------------------------------------------------------------ typed factors (landmarks, priors)
    # include/cgmr.h: cgmr_factor_types.  ``vertex_kind`` [nV] (0 pose, 1 point) and ``edge_kind`` [nE] (0 EDGE_SE2, 1 EDGE_SE2_XY,
    # 2 EDGE_BEARING_SE2_XY, 3 EDGE_PRIOR_SE2, 4 EDGE_PRIOR_SE2_XY; a prior has from == to), None = all zero; ``kind`` / ``delta``: robust kernels as
    # gn_optimize_robust takes them, None = the plain call.  Each returns what its untyped call does, with (e2, weights) appended
    # when ``kind`` is given.
    def _typed(self, entry, problem, iters, vertex_kind, edge_kind, kind, delta, prm=None, n_int=None, allow_fail=False):
        nE = len(problem[2])
        nV = problem[0][1] if isinstance(problem[0], tuple) else len(problem[0])
        ft, _keep_ft = factor_types(vertex_kind, edge_kind, nV, nE)
        rk, e2, w, _keep = self._robust(kind, delta, nE) if kind is not None else (None, None, None, None)
        out = self._optimize(entry, problem, iters, prm, n_int, rk=rk, allow_fail=allow_fail, ft=ft)
        return out + (e2, w) if kind is not None else out

    def gn_optimize_typed(self, poses, fixed, ef, et, meas, info, iters, vertex_kind=None, edge_kind=None, kind=None, delta=1.0,
                          raise_on_cholesky=True):
        """Gauss-Newton with typed factors: (status, poses, chi2[iters+1])."""
        return self._typed("cgmr_gn_optimize_typed", (poses, fixed, ef, et, meas, info), iters, vertex_kind, edge_kind, kind, delta,
                           allow_fail=not raise_on_cholesky)

    def gn_optimize_typed_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, vertex_kind=None, edge_kind=None,
                              kind=None, delta=1.0, raise_on_cholesky=True):
        """gn_optimize_typed on device pointers (the kinds stay host arrays): (status, chi2[iters+1])."""
        return self._typed("cgmr_gn_optimize_typed_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                           vertex_kind, edge_kind, kind, delta, allow_fail=not raise_on_cholesky)

    def lm_optimize_typed(self, poses, fixed, ef, et, meas, info, iters, vertex_kind=None, edge_kind=None, kind=None, delta=1.0,
                          **params):
        """Levenberg-Marquardt with typed factors: (status, poses, chi2, lambdas, trials, iters_done)."""
        return self._typed("cgmr_lm_optimize_typed", (poses, fixed, ef, et, meas, info), iters, vertex_kind, edge_kind, kind, delta,
                           lm_params(**params), 1)

    def lm_optimize_typed_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, vertex_kind=None, edge_kind=None,
                              kind=None, delta=1.0, **params):
        """lm_optimize_typed on device pointers: (status, chi2, lambdas, trials, iters_done)."""
        return self._typed("cgmr_lm_optimize_typed_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                           vertex_kind, edge_kind, kind, delta, lm_params(**params), 1)

    def dl_optimize_typed(self, poses, fixed, ef, et, meas, info, iters, vertex_kind=None, edge_kind=None, kind=None, delta=1.0,
                          raise_on_fail=True, **params):
        """Dogleg with typed factors: (status, poses, chi2, deltas, trials, steps, iters_done)."""
        return self._typed("cgmr_dl_optimize_typed", (poses, fixed, ef, et, meas, info), iters, vertex_kind, edge_kind, kind, delta,
                           dl_params(**params), 2, allow_fail=not raise_on_fail)

    def dl_optimize_typed_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, vertex_kind=None, edge_kind=None,
                              kind=None, delta=1.0, raise_on_fail=True, **params):
        """dl_optimize_typed on device pointers: (status, chi2, deltas, trials, steps, iters_done)."""
        return self._typed("cgmr_dl_optimize_typed_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                           vertex_kind, edge_kind, kind, delta, dl_params(**params), 2, allow_fail=not raise_on_fail)

    # ------------------------------------------------------------------ max-mixture edges
    # include/cgmr.h: cgmr_mixture.  ``mixture`` = (comp_ptr [nE + 1], comp_meas [nC, 3], comp_info [nC, 6], comp_weight [nC]), host
    # arrays in the _dev variants too, None = the typed / plain call; ``meas`` / ``info`` hold every edge's first component.
    # ``vertex_kind`` / ``edge_kind`` as the typed calls.  Each returns what its typed call does with ``selected`` int32 [nE]
    # appended: every edge's selected component at the returned poses.
    def _mixture(self, entry, problem, iters, mixture, vertex_kind, edge_kind, prm=None, n_int=None, allow_fail=False):
        nE = len(problem[2])
        nV = problem[0][1] if isinstance(problem[0], tuple) else len(problem[0])
        ft, _keep_ft = factor_types(vertex_kind, edge_kind, nV, nE)
        mix, sel, _keep = mixture_arrays(mixture, nE)
        out = self._optimize(entry, problem, iters, prm, n_int, rk=mix, allow_fail=allow_fail, ft=ft)
        return out + (sel,)

    def gn_optimize_mixture(self, poses, fixed, ef, et, meas, info, iters, mixture=None, vertex_kind=None, edge_kind=None,
                            raise_on_cholesky=True):
        """Gauss-Newton on max-mixture edges: (status, poses, chi2[iters+1], selected)."""
        return self._mixture("cgmr_gn_optimize_mixture", (poses, fixed, ef, et, meas, info), iters, mixture, vertex_kind, edge_kind,
                             allow_fail=not raise_on_cholesky)

    def gn_optimize_mixture_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, mixture=None, vertex_kind=None,
                                edge_kind=None, raise_on_cholesky=True):
        """gn_optimize_mixture on device pointers (the mixture stays host arrays): (status, chi2[iters+1], selected)."""
        return self._mixture("cgmr_gn_optimize_mixture_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                             mixture, vertex_kind, edge_kind, allow_fail=not raise_on_cholesky)

    def lm_optimize_mixture(self, poses, fixed, ef, et, meas, info, iters, mixture=None, vertex_kind=None, edge_kind=None, **params):
        """Levenberg-Marquardt on max-mixture edges: (status, poses, chi2, lambdas, trials, iters_done, selected)."""
        return self._mixture("cgmr_lm_optimize_mixture", (poses, fixed, ef, et, meas, info), iters, mixture, vertex_kind, edge_kind,
                             lm_params(**params), 1)

    def lm_optimize_mixture_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, mixture=None, vertex_kind=None,
                                edge_kind=None, **params):
        """lm_optimize_mixture on device pointers: (status, chi2, lambdas, trials, iters_done, selected)."""
        return self._mixture("cgmr_lm_optimize_mixture_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                             mixture, vertex_kind, edge_kind, lm_params(**params), 1)

    def dl_optimize_mixture(self, poses, fixed, ef, et, meas, info, iters, mixture=None, vertex_kind=None, edge_kind=None,
                            raise_on_fail=True, **params):
        """Dogleg on max-mixture edges: (status, poses, chi2, deltas, trials, steps, iters_done, selected)."""
        return self._mixture("cgmr_dl_optimize_mixture", (poses, fixed, ef, et, meas, info), iters, mixture, vertex_kind, edge_kind,
                             dl_params(**params), 2, allow_fail=not raise_on_fail)

    def dl_optimize_mixture_dev(self, d_poses_ptr, nV, fixed, ef, et, d_meas_ptr, d_info_ptr, iters, mixture=None, vertex_kind=None,
                                edge_kind=None, raise_on_fail=True, **params):
        """dl_optimize_mixture on device pointers: (status, chi2, deltas, trials, steps, iters_done, selected)."""
        return self._mixture("cgmr_dl_optimize_mixture_dev", ((d_poses_ptr, nV), fixed, ef, et, d_meas_ptr, d_info_ptr), iters,
                             mixture, vertex_kind, edge_kind, dl_params(**params), 2, allow_fail=not raise_on_fail)

    def mixture_select(self, poses, fixed, ef, et, meas, info, mixture=None, vertex_kind=None, edge_kind=None):
        """The mixture cost and the selection at ``poses`` (cgmr_mixture_select, one chi-only pass): (chi2, selected)."""
        nV, p, (pp, fx, nE, f, t, m, i), _keep = self._problem(poses, fixed, ef, et, meas, info)
        ft, _keep_ft = factor_types(vertex_kind, edge_kind, nV, nE.value)
        mix, sel, _keep_mix = mixture_arrays(mixture, nE.value)
        chi = np.zeros(1)
        rc = self.lib.cgmr_mixture_select(self.h, C.c_int(nV), pp, fx, nE, f, t, m, i, C.byref(ft),
                                          C.byref(mix) if mix is not None else C.c_void_p(0), _ptr(chi))
        self._check(rc)
        return float(chi[0]), sel

    def marginals_typed(self, poses, fixed, ef, et, meas, info, query, vertex_kind=None, edge_kind=None, kind=None, delta=1.0):
        """marginals on the typed H: cov [nK, 3, 3] (a point's third row and column are zero); (cov, e2, weights) with ``kind``."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        query = np.ascontiguousarray(query, dtype=np.int32)
        ft, _keep_ft = factor_types(vertex_kind, edge_kind, poses.shape[0], len(ef))
        rk, e2, w, _keep = self._robust(kind, delta, len(ef)) if kind is not None else (None, None, None, None)
        cov = np.zeros((len(query), 3, 3))
        rc = self.lib.cgmr_marginals_typed(self.h, C.c_int(poses.shape[0]), _ptr(poses), _ptr(fixed), C.c_int(len(ef)), _ptr(ef),
                                           _ptr(et), _ptr(meas), _ptr(info), C.c_int(len(query)), _ptr(query), _ptr(cov),
                                           C.byref(ft), C.byref(rk) if rk is not None else C.c_void_p(0))
        self._check(rc)
        return (cov, e2, w) if kind is not None else cov

    def marginals_all_typed(self, poses, fixed, ef, et, meas, info, cross=False, vertex_kind=None, edge_kind=None, kind=None,
                            delta=1.0):
        """marginals_all on the typed H: cov [nV, 3, 3], with ``cross=True`` (cov, cross [nE, 3, 3]); (e2, weights) appended
        with ``kind``."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        ft, _keep_ft = factor_types(vertex_kind, edge_kind, poses.shape[0], len(ef))
        rk, e2, w, _keep = self._robust(kind, delta, len(ef)) if kind is not None else (None, None, None, None)
        cov = np.zeros((poses.shape[0], 3, 3))
        cr = np.zeros((len(ef), 3, 3)) if cross else None
        rc = self.lib.cgmr_marginals_all_typed(self.h, C.c_int(poses.shape[0]), _ptr(poses), _ptr(fixed), C.c_int(len(ef)),
                                               _ptr(ef), _ptr(et), _ptr(meas), _ptr(info), _ptr(cov), _ptr(cr), C.byref(ft),
                                               C.byref(rk) if rk is not None else C.c_void_p(0))
        self._check(rc)
        out = (cov, cr) if cross else (cov,)
        if kind is not None:
            out += (e2, w)
        return out if len(out) > 1 else out[0]

    # ------------------------------------------------------------------ marginals / condensed graph
    @staticmethod
    def _graph_args(poses, ef, et, meas, info):
        return (np.ascontiguousarray(poses, dtype=np.float64), np.ascontiguousarray(ef, dtype=np.int32),
                np.ascontiguousarray(et, dtype=np.int32), np.ascontiguousarray(meas, dtype=np.float64),
                np.ascontiguousarray(info, dtype=np.float64))

    def marginals(self, poses, fixed, ef, et, meas, info, query):
        """3x3 blocks of H^-1 (H linearised at ``poses``) for the query vertex indices."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        query = np.ascontiguousarray(query, dtype=np.int32)
        cov = np.zeros((len(query), 3, 3))
        rc = self.lib.cgmr_marginals(self.h, C.c_int(poses.shape[0]), _ptr(poses), _ptr(fixed), C.c_int(len(ef)),
                                     _ptr(ef), _ptr(et), _ptr(meas), _ptr(info), C.c_int(len(query)), _ptr(query),
                                     _ptr(cov))
        self._check(rc)
        return cov

    def marginals_all(self, poses, fixed, ef, et, meas, info, cross=False):
        """3x3 blocks of H^-1 (H linearised at ``poses``) of every vertex: ``cov[nV, 3, 3]``; with ``cross=True``
        ``(cov, cross[nE, 3, 3])``, cross[e] = the block (from[e], to[e]).  Selected inversion (cgmr_marginals_all)."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        cov = np.zeros((poses.shape[0], 3, 3))
        cr = np.zeros((len(ef), 3, 3)) if cross else None
        rc = self.lib.cgmr_marginals_all(self.h, C.c_int(poses.shape[0]), _ptr(poses), _ptr(fixed), C.c_int(len(ef)),
                                         _ptr(ef), _ptr(et), _ptr(meas), _ptr(info), _ptr(cov),
                                         _ptr(cr))
        self._check(rc)
        return (cov, cr) if cross else cov

    def covariance_estimate(self, poses, ef, et, meas, info, gauge, query):
        """CovarianceEstimator::compute + getCovariance (src/slam/graph_manipulator.cpp:128-157)."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        query = np.ascontiguousarray(query, dtype=np.int32)
        cov = np.zeros((len(query), 3, 3))
        rc = self.lib.cgmr_covariance_estimate(self.h, C.c_int(poses.shape[0]), _ptr(poses), C.c_int(len(ef)), _ptr(ef),
                                               _ptr(et), _ptr(meas), _ptr(info), C.c_int(int(gauge)),
                                               C.c_int(len(query)), _ptr(query), _ptr(cov))
        self._check(rc)
        return cov

    def condense(self, poses, ef, et, meas, info, gauge, query):
        """CondensedGraphCreator::compute: returns (to[n], est[n,3], info_upper[n,6], cov[n,3,3])."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        query = np.ascontiguousarray(query, dtype=np.int32)
        n = max(len(query), 1)
        to = np.zeros(n, dtype=np.int32)
        est = np.zeros((n, 3))
        iu = np.zeros((n, 6))
        cov = np.zeros((n, 3, 3))
        rc = self.lib.cgmr_condense(self.h, C.c_int(poses.shape[0]), _ptr(poses), C.c_int(len(ef)), _ptr(ef), _ptr(et),
                                    _ptr(meas), _ptr(info), C.c_int(int(gauge)), C.c_int(len(query)), _ptr(query),
                                    _ptr(to), _ptr(est), _ptr(iu), _ptr(cov))
        if rc < 0:
            self._check(rc)
        return to[:rc].copy(), est[:rc].copy(), iu[:rc].copy(), cov[:rc].copy()

    # robust kernels in the marginals and the condensed graph (include/cgmr.h: cgmr_marginals_robust ...): ``kind`` / ``delta`` as
    # for gn_optimize_robust; rho1 at the linearisation point of the H that is inverted (the poses given for the marginals, the
    # spanning-tree guess for covariance_estimate / condense).  Each returns what the plain call does, then (e2 [nE], weights
    # [nE]) at that point.
    def marginals_robust(self, poses, fixed, ef, et, meas, info, query, kind="none", delta=1.0):
        """marginals with robust kernels: (cov, e2, weights)."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        query = np.ascontiguousarray(query, dtype=np.int32)
        rk, e2, w, _keep = self._robust(kind, delta, len(ef))
        cov = np.zeros((len(query), 3, 3))
        rc = self.lib.cgmr_marginals_robust(self.h, C.c_int(poses.shape[0]), _ptr(poses), _ptr(fixed), C.c_int(len(ef)),
                                            _ptr(ef), _ptr(et), _ptr(meas), _ptr(info), C.c_int(len(query)), _ptr(query),
                                            _ptr(cov), C.byref(rk))
        self._check(rc)
        return cov, e2, w

    def marginals_all_robust(self, poses, fixed, ef, et, meas, info, cross=False, kind="none", delta=1.0):
        """marginals_all with robust kernels: (cov, e2, weights), or (cov, cross, e2, weights) with ``cross=True``."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        rk, e2, w, _keep = self._robust(kind, delta, len(ef))
        cov = np.zeros((poses.shape[0], 3, 3))
        cr = np.zeros((len(ef), 3, 3)) if cross else None
        rc = self.lib.cgmr_marginals_all_robust(self.h, C.c_int(poses.shape[0]), _ptr(poses), _ptr(fixed), C.c_int(len(ef)),
                                                _ptr(ef), _ptr(et), _ptr(meas), _ptr(info), _ptr(cov), _ptr(cr), C.byref(rk))
        self._check(rc)
        return (cov, cr, e2, w) if cross else (cov, e2, w)

    def covariance_estimate_robust(self, poses, ef, et, meas, info, gauge, query, kind="none", delta=1.0):
        """covariance_estimate with robust kernels: (cov, e2, weights)."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        query = np.ascontiguousarray(query, dtype=np.int32)
        rk, e2, w, _keep = self._robust(kind, delta, len(ef))
        cov = np.zeros((len(query), 3, 3))
        rc = self.lib.cgmr_covariance_estimate_robust(self.h, C.c_int(poses.shape[0]), _ptr(poses), C.c_int(len(ef)), _ptr(ef),
                                                      _ptr(et), _ptr(meas), _ptr(info), C.c_int(int(gauge)),
                                                      C.c_int(len(query)), _ptr(query), _ptr(cov), C.byref(rk))
        self._check(rc)
        return cov, e2, w

    def condense_robust(self, poses, ef, et, meas, info, gauge, query, kind="none", delta=1.0):
        """condense with robust kernels: (to, est, info_upper, cov, e2, weights)."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        query = np.ascontiguousarray(query, dtype=np.int32)
        rk, e2, w, _keep = self._robust(kind, delta, len(ef))
        n = max(len(query), 1)
        to = np.zeros(n, dtype=np.int32)
        est = np.zeros((n, 3))
        iu = np.zeros((n, 6))
        cov = np.zeros((n, 3, 3))
        rc = self.lib.cgmr_condense_robust(self.h, C.c_int(poses.shape[0]), _ptr(poses), C.c_int(len(ef)), _ptr(ef), _ptr(et),
                                           _ptr(meas), _ptr(info), C.c_int(int(gauge)), C.c_int(len(query)), _ptr(query),
                                           _ptr(to), _ptr(est), _ptr(iu), _ptr(cov), C.byref(rk))
        if rc < 0:
            self._check(rc)
        return to[:rc].copy(), est[:rc].copy(), iu[:rc].copy(), cov[:rc].copy(), e2, w

    # the condensed graph as a spanning tree of relative poses (include/cgmr.h: cgmr_condense_tree, cgmr_min_spanning_tree)
    def condense_tree(self, poses, ef, et, meas, info, gauge, query, kind=None, delta=1.0):
        """The condensed graph over ``query`` as the minimum spanning tree of log det Sigma_z over the gauge and the unique
        requested vertices, rooted at the gauge: ``(from [n], to [n], est [n, 3], info_upper [n, 6], weight [n], flags [n])``,
        one edge per requested vertex other than the gauge in order of first appearance, from = its parent in the tree.
        flags: 0, 1 (unlabelled: identity information), 2 (no finite weight: hung on the gauge).  At most TREE_MAX_NODES nodes.
        ``kind`` / ``delta``: robust kernels as condense_robust takes them, (e2, weights) appended."""
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        query = np.ascontiguousarray(query, dtype=np.int32).reshape(-1)
        rk, e2, w, _keep = self._robust(kind, delta, len(ef)) if kind is not None else (None, None, None, None)
        n = max(len(query), 1)
        fr, to, fl = (np.zeros(n, dtype=np.int32) for _ in range(3))
        est, iu, wt = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros(n)
        rc = self.lib.cgmr_condense_tree(self.h, C.c_int(poses.shape[0]), _ptr(poses), C.c_int(len(ef)), _ptr(ef), _ptr(et),
                                         _ptr(meas), _ptr(info), C.c_int(int(gauge)), C.c_int(len(query)), _ptr(query), _ptr(fr),
                                         _ptr(to), _ptr(est), _ptr(iu), _ptr(wt), _ptr(fl),
                                         C.byref(rk) if rk is not None else C.c_void_p(0))
        if rc < 0:
            self._check(rc)
        out = tuple(a[:rc].copy() for a in (fr, to, est, iu, wt, fl))
        return out if kind is None else out + (e2, w)

    def min_spanning_tree(self, weights, root=0):
        """``parent [n]`` (int32, parent[root] = -1) of the minimum spanning tree of the dense symmetric ``weights`` [n, n] under
        the total order (w, max(a, b), min(a, b)), rooted at ``root``: the combinatorial half of condense_tree.  Only the lower
        triangle is read; a NaN counts as +inf.  1 <= n <= TREE_MAX_NODES.  Deterministic."""
        W = np.ascontiguousarray(weights, dtype=np.float64)
        n = W.shape[0]
        if W.shape != (n, n):
            raise ValueError(f"weights: a square matrix, not {W.shape}")
        parent = np.full(n, -1, dtype=np.int32)
        self._check(self.lib.cgmr_min_spanning_tree(self.h, C.c_int(n), _ptr(W), C.c_int(int(root)), _ptr(parent)))
        return parent

    # vertex removal (include/cgmr.h: cgmr_remove_nodes)
    def remove_nodes(self, ef, et, meas, info, remove, num_vertices=None):
        """What replaces the edges of each vertex of ``remove`` (an independent set of a pose-only graph) once it is gone: the
        vertex marginalised out of the star of its incident edges, and a minimum spanning tree of log det Sigma_z over its
        neighbours, rooted at the lowest, with first-order labels.  Estimates are not an input.  Returns ``(off [nR + 1],
        from [n], to [n], meas [n, 3], info_upper [n, 6], weight [n], flags [nR])``: the edges of ``remove[r]`` are
        off[r] .. off[r + 1] - 1; flags 0 removed, 1 no Cholesky factor, 2 more than REMOVE_MAX_DEGREE neighbours, 3 a tree
        edge without a finite weight -- a vertex flagged 1, 2 or 3 stays and gets no edges.  ``num_vertices``: default, the
        largest index used + 1.  Deterministic."""
        ef, et = np.ascontiguousarray(ef, dtype=np.int32).reshape(-1), np.ascontiguousarray(et, dtype=np.int32).reshape(-1)
        meas, info = np.ascontiguousarray(meas, dtype=np.float64), np.ascontiguousarray(info, dtype=np.float64)
        remove = np.ascontiguousarray(remove, dtype=np.int32).reshape(-1)
        nE, nR = len(ef), len(remove)
        if len(et) != nE or meas.size != 3 * nE or info.size != 6 * nE:
            raise ValueError("remove_nodes: ef, et [nE], meas [nE, 3], info [nE, 6]")
        if num_vertices is None:
            num_vertices = 1 + max([0] + [int(a.max()) for a in (ef, et, remove) if len(a)])
        # every removed vertex' degree is at most its count of incident edges
        cnt = np.bincount(np.concatenate([ef, et]).clip(0), minlength=1)
        ok = remove[(remove >= 0) & (remove < len(cnt))]
        cap = int(np.maximum(np.minimum(cnt[ok], REMOVE_MAX_DEGREE) - 1, 0).sum())
        n = max(cap, 1)
        off, fl = np.zeros(nR + 1, dtype=np.int32), np.zeros(max(nR, 1), dtype=np.int32)
        fr, to = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        z, iu, wt = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros(n)
        rc = self.lib.cgmr_remove_nodes(self.h, C.c_int(int(num_vertices)), C.c_int(nE), _ptr(ef), _ptr(et), _ptr(meas), _ptr(info),
                                        C.c_int(nR), _ptr(remove), C.c_int(cap), _ptr(off), _ptr(fr), _ptr(to), _ptr(z), _ptr(iu),
                                        _ptr(wt), _ptr(fl))
        if rc < 0:
            self._check(rc)
        return (off,) + tuple(a[:rc].copy() for a in (fr, to, z, iu, wt)) + (fl[:nR].copy(),)

    # scan ranking and greedy pruning (include/cgmr.h: cgmr_scan_information, cgmr_scan_prune)
    @staticmethod
    def _scan_args(cfg, ranges, robot_poses):
        ranges = np.ascontiguousarray(ranges, dtype=np.float32)
        poses = np.ascontiguousarray(robot_poses, dtype=np.float64).reshape(-1, 3)
        if ranges.ndim != 2 or ranges.shape[0] != poses.shape[0]:
            raise ValueError("ranges [n_scans, n_beams], robot_poses [n_scans, 3]")
        return ranges, poses, (int(cfg.rows), int(cfg.cols))

    def scan_information(self, cfg, ranges, robot_poses, scratch_bytes_limit=0):
        """What every scan tells the occupancy map of all of them (``cfg``: an occupancy.OccupancyConfig as cgmr_occupancy_map
        takes it).  Returns a dict: ``delta`` [n] the entropy, in nats, the map gains if the scan is dropped; ``cells`` [n] the
        cells the scan touches; ``hit_sum`` / ``miss_sum`` [n] int64; ``hits`` / ``misses`` [rows, cols] the totals;
        ``map_entropy``; ``kernel_seconds``.  ``scratch_bytes_limit``: the bytes of scan windows alive at one time (0: the
        library's default); the result does not depend on it."""
        ranges, poses, shape = self._scan_args(cfg, ranges, robot_poses)
        n = ranges.shape[0]
        out = dict(delta=np.zeros(n), cells=np.zeros(n, dtype=np.int32), hit_sum=np.zeros(n, dtype=np.int64),
                   miss_sum=np.zeros(n, dtype=np.int64), hits=np.zeros(shape, dtype=np.int32), misses=np.zeros(shape, dtype=np.int32))
        ent, ks = C.c_double(), C.c_double()
        rc = self.lib.cgmr_scan_information(self.h, C.byref(cfg), C.c_int(n), C.c_int(ranges.shape[1]), _ptr(ranges), _ptr(poses),
                                            C.c_int64(int(scratch_bytes_limit)), _ptr(out["delta"]), _ptr(out["cells"]),
                                            _ptr(out["hit_sum"]), _ptr(out["miss_sum"]), _ptr(out["hits"]), _ptr(out["misses"]),
                                            C.byref(ent), C.byref(ks))
        self._check(rc)
        out.update(map_entropy=ent.value, kernel_seconds=ks.value)
        return out

    def scan_prune(self, cfg, ranges, robot_poses, max_remove, max_entropy_increase=-1.0, protected=None, scratch_bytes_limit=0):
        """Greedy pruning: scans are taken one at a time, each time the unprotected one whose loss raises the map's entropy
        least (ties: the lower index), until ``max_remove`` are gone, none is left, or -- ``max_entropy_increase`` >= 0 -- the
        sum of the taken deltas would exceed it.  Returns a dict: ``order`` [k] the scans in the order taken, ``delta`` [k];
        ``entropy_before`` / ``entropy_after``; ``hits`` / ``misses`` the totals of the kept scans; ``kernel_seconds``."""
        ranges, poses, shape = self._scan_args(cfg, ranges, robot_poses)
        n = ranges.shape[0]
        prot = None
        if protected is not None:
            prot = np.ascontiguousarray(np.asarray(protected).astype(bool), dtype=np.uint8).reshape(-1)
            if len(prot) != n:
                raise ValueError("protected: one flag per scan")
        cap = max(min(int(max_remove), n), 1)
        order, delta = np.zeros(cap, dtype=np.int32), np.zeros(cap)
        hits, misses = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
        k, before, after, ks = C.c_int32(), C.c_double(), C.c_double(), C.c_double()
        rc = self.lib.cgmr_scan_prune(self.h, C.byref(cfg), C.c_int(n), C.c_int(ranges.shape[1]), _ptr(ranges), _ptr(poses), _ptr(prot),
                                      C.c_int(int(max_remove)), C.c_double(float(max_entropy_increase)),
                                      C.c_int64(int(scratch_bytes_limit)), _ptr(order), _ptr(delta), C.byref(k), C.byref(before),
                                      C.byref(after), _ptr(hits), _ptr(misses), C.byref(ks))
        self._check(rc)
        return dict(order=order[:k.value].copy(), delta=delta[:k.value].copy(), entropy_before=before.value, entropy_after=after.value,
                    hits=hits, misses=misses, kernel_seconds=ks.value)

    def scan_info_last_stats(self):
        """(bytes of all scan windows, chunks, largest window in bytes, greedy rounds queued) of the last ranking / pruning call."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.cgmr_scan_info_last_stats(self.h, _ptr(out)))
        return tuple(int(v) for v in out)

    # joint and pairwise blocks of H^-1, relative-pose uncertainty (include/cgmr.h: cgmr_marginals_joint ...).  ``kind`` None: the
    # plain call; otherwise robust kernels as marginals_robust takes them, and (e2 [nE], weights [nE]) are appended.
    # ``vertex_kind`` / ``edge_kind`` (either given): the typed entry point (cgmr_marginals_joint_typed ...), kinds as for
    # gn_optimize_typed; a point's third row and column come back exactly zero.
    def _joint_call(self, entry, poses, fixed, ef, et, meas, info, tail, kind, delta, vertex_kind=None, edge_kind=None, typed=False):
        poses, ef, et, meas, info = self._graph_args(poses, ef, et, meas, info)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        rk, e2, w, _keep = self._robust(kind, delta, len(ef)) if kind is not None else (None, None, None, None)
        types = ()
        if typed or vertex_kind is not None or edge_kind is not None:
            ft, _keep_ft = factor_types(vertex_kind, edge_kind, poses.shape[0], len(ef))
            types = (C.byref(ft),)
            if not typed:
                entry += "_typed"
        rc = getattr(self.lib, entry)(self.h, C.c_int(poses.shape[0]), _ptr(poses), _ptr(fixed), C.c_int(len(ef)), _ptr(ef), _ptr(et),
                                      _ptr(meas), _ptr(info), *tail, *types, C.byref(rk) if rk is not None else C.c_void_p(0))
        self._check(rc)
        return () if kind is None else (e2, w)

    @staticmethod
    def _pair_arrays(pair_a, pair_b):
        a = np.ascontiguousarray(pair_a, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(pair_b, dtype=np.int32).reshape(-1)
        if a.shape != b.shape:
            raise ValueError(f"pairs: {a.shape[0]} first vertices, {b.shape[0]} second vertices")
        return a, b

    def marginals_joint(self, poses, fixed, ef, et, meas, info, query, kind=None, delta=1.0, vertex_kind=None, edge_kind=None):
        """The joint covariance of the query vertices, ``[3 nK, 3 nK]`` in query order (block (k, l) = Sigma of query[k],
        query[l]); exactly symmetric, zeros for fixed / inactive vertices.  At most JOINT_MAX_QUERIES unique vertices."""
        query = np.ascontiguousarray(query, dtype=np.int32).reshape(-1)
        cov = np.zeros((3 * len(query), 3 * len(query)))
        st = self._joint_call("cgmr_marginals_joint", poses, fixed, ef, et, meas, info,
                              (C.c_int(len(query)), _ptr(query), _ptr(cov)), kind, delta, vertex_kind, edge_kind)
        return (cov,) + st if st else cov

    def marginals_pairs(self, poses, fixed, ef, et, meas, info, pair_a, pair_b, kind=None, delta=1.0, vertex_kind=None,
                        edge_kind=None):
        """(Sigma_aa, Sigma_ab, Sigma_bb), each ``[nP, 3, 3]``, for the vertex pairs (pair_a[p], pair_b[p]) -- any two vertices,
        not only a graph edge's; rows of Sigma_ab index a."""
        a, b = self._pair_arrays(pair_a, pair_b)
        aa, ab, bb = (np.zeros((len(a), 3, 3)) for _ in range(3))
        st = self._joint_call("cgmr_marginals_pairs", poses, fixed, ef, et, meas, info,
                              (C.c_int(len(a)), _ptr(a), _ptr(b), _ptr(aa), _ptr(ab), _ptr(bb)), kind, delta, vertex_kind, edge_kind)
        return (aa, ab, bb) + st

    def relative_covariance(self, poses, fixed, ef, et, meas, info, pair_a, pair_b, hyp_meas=None, hyp_info=None, kind=None,
                            delta=1.0):
        """(z [nP, 3], Sigma_z [nP, 3, 3], d2 [nP] or None): z = x_a^-1 x_b and its first-order covariance from the joint
        covariance of (x_a, x_b).  ``hyp_meas`` [nP, 3] (and ``hyp_info`` [nP, 6], upper triangle, optional): d2 is the squared
        Mahalanobis distance of that hypothesis from z under Sigma_z (+ hyp_info^-1); NaN where not positive definite."""
        a, b = self._pair_arrays(pair_a, pair_b)
        n = len(a)
        hm = hi = d2 = None
        if hyp_meas is not None:
            hm = np.ascontiguousarray(hyp_meas, dtype=np.float64).reshape(n, 3)
            d2 = np.zeros(n)
        if hyp_info is not None:
            if hm is None:
                raise ValueError("hyp_info needs hyp_meas")
            hi = np.ascontiguousarray(hyp_info, dtype=np.float64).reshape(n, 6)
        z, cz = np.zeros((n, 3)), np.zeros((n, 3, 3))
        st = self._joint_call("cgmr_relative_covariance", poses, fixed, ef, et, meas, info,
                              (C.c_int(n), _ptr(a), _ptr(b), _ptr(z), _ptr(cz), _ptr(hm), _ptr(hi), _ptr(d2)), kind, delta)
        return (z, cz, d2) + st

    def observation_covariance(self, poses, fixed, ef, et, meas, info, pair_a, pair_b, obs_kind=None, hyp_meas=None, hyp_info=None,
                               vertex_kind=None, edge_kind=None, kind=None, delta=1.0):
        """Data association (cgmr_observation_covariance): pair p predicted as a factor of kind ``obs_kind[p]`` -- 0 pose-pose
        (relative_covariance), 1 EDGE_SE2_XY, 2 EDGE_BEARING_SE2_XY, from pose pair_a[p] to pair_b[p]; None: all 0.  Returns
        (z [nP, 3], S [nP, 3, 3], d2 [nP] or None), padded with zeros outside the factor's dimension; ``hyp_meas`` [nP, 3] /
        ``hyp_info`` [nP, 6] as for relative_covariance, read in the factor's dimension (a bearing: hyp_meas[:, 0] and
        hyp_info[:, 0]).  ``kind`` / ``delta``: robust kernels, (e2, weights) appended."""
        a, b = self._pair_arrays(pair_a, pair_b)
        n = len(a)
        ok = None if obs_kind is None else np.ascontiguousarray(obs_kind, dtype=np.uint8).reshape(-1)
        if ok is not None and ok.shape != (n,):
            raise ValueError(f"observation kinds: {ok.shape[0]} given for {n} pairs")
        hm = hi = d2 = None
        if hyp_meas is not None:
            hm = np.ascontiguousarray(hyp_meas, dtype=np.float64).reshape(n, 3)
            d2 = np.zeros(n)
        if hyp_info is not None:
            if hm is None:
                raise ValueError("hyp_info needs hyp_meas")
            hi = np.ascontiguousarray(hyp_info, dtype=np.float64).reshape(n, 6)
        z, cz = np.zeros((n, 3)), np.zeros((n, 3, 3))
        st = self._joint_call("cgmr_observation_covariance", poses, fixed, ef, et, meas, info,
                              (C.c_int(n), _ptr(a), _ptr(b), _ptr(ok), _ptr(z), _ptr(cz), _ptr(hm), _ptr(hi), _ptr(d2)), kind, delta,
                              vertex_kind, edge_kind, typed=True)
        return (z, cz, d2) + st

    # pairwise consistency maximisation of closure candidates (include/cgmr.h: cgmr_closure_consistency, cgmr_max_clique_greedy)
    @staticmethod
    def _adj_bool(words, n):
        """[n, n] bool from rows of 64-bit words: bit (l & 63) of word (k, l >> 6)."""
        if n == 0:
            return np.zeros((0, 0), dtype=bool)
        bits = (words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
        return bits.reshape(n, -1)[:, :n].astype(bool)

    @staticmethod
    def _adj_words(adj):
        adj = np.asarray(adj)
        if adj.dtype == np.uint64:                                  # rows of words already ([n, W])
            return np.ascontiguousarray(adj.reshape(adj.shape[0], -1)), adj.shape[0]
        n = adj.shape[0]
        if adj.shape != (n, n):
            raise ValueError(f"adjacency: a square matrix, not {adj.shape}")
        W = (n + 63) // 64
        bits = np.zeros((n, 64 * W), dtype=np.uint64)
        bits[:, :n] = adj.astype(bool)
        words = (bits.reshape(n, W, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
        return np.ascontiguousarray(words), n

    def closure_consistency(self, poses, fixed, ef, et, meas, info, cl_a, cl_b, cl_meas, cl_info, gamma, kind=None, delta=1.0):
        """Pairwise consistency of N closure candidates (a, b, meas [N, 3], info_upper [N, 6]) that are not edges of the graph:
        ``(d2 [N, N], adj [N, N] bool, clique, seed)`` -- d2 the squared Mahalanobis distance of the loop every pair closes
        under the joint covariance of its four poses (NaN where not positive definite, 0 on the diagonal), adj = d2 < gamma off
        the diagonal, clique the indices (ascending) of the greedy maximum clique of adj and the seed it grew from.  A greedy
        heuristic, not an exact solver.  At most PCM_MAX_CLOSURES candidates.  ``kind`` / ``delta``: robust kernels on the
        graph's edges, (e2, weights) appended."""
        a, b = self._pair_arrays(cl_a, cl_b)
        n = len(a)
        cm = np.ascontiguousarray(cl_meas, dtype=np.float64).reshape(n, 3)
        ci = np.ascontiguousarray(cl_info, dtype=np.float64).reshape(n, 6)
        W = (n + 63) // 64
        d2, words = np.zeros((n, n)), np.zeros((n, W), dtype=np.uint64)
        clique, size, seed = np.full(n, -1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
        st = self._joint_call("cgmr_closure_consistency", poses, fixed, ef, et, meas, info,
                              (C.c_int(n), _ptr(a), _ptr(b), _ptr(cm), _ptr(ci), C.c_double(float(gamma)), _ptr(d2), _ptr(words),
                               _ptr(clique), _ptr(size), _ptr(seed)), kind, delta)
        return (d2, self._adj_bool(words, n), clique[:int(size[0])].copy(), int(seed[0])) + st

    def max_clique_greedy(self, adj):
        """``(clique, seed)`` of a symmetric adjacency with a clear diagonal -- [n, n] bool, or rows of 64-bit words [n, W]
        uint64 --: the greedy clique of closure_consistency (from every seed, the candidate with most neighbours left joins;
        the largest over the seeds, ties to the lowest).  At most PCM_MAX_CLOSURES vertices."""
        words, n = self._adj_words(adj)
        clique, size, seed = np.full(n, -1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
        self._check(self.lib.cgmr_max_clique_greedy(self.h, C.c_int(n), _ptr(words), _ptr(clique), _ptr(size), _ptr(seed)))
        return clique[:int(size[0])].copy(), int(seed[0])

    def closure_consistency_exact(self, poses, fixed, ef, et, meas, info, cl_a, cl_b, cl_meas, cl_info, gamma,
                                  node_limit=EXACT_DEFAULT_NODE_LIMIT, kind=None, delta=1.0):
        """closure_consistency with the exact maximum clique of adj (cgmr_closure_consistency_exact): ``(d2, adj, clique,
        proven)``, d2 and adj the plain call's.  ``node_limit``: as for max_clique_exact; when ``proven`` is False the clique is
        the best found, never smaller than the greedy one.  ``kind`` / ``delta``: robust kernels, (e2, weights) appended."""
        a, b = self._pair_arrays(cl_a, cl_b)
        n = len(a)
        cm = np.ascontiguousarray(cl_meas, dtype=np.float64).reshape(n, 3)
        ci = np.ascontiguousarray(cl_info, dtype=np.float64).reshape(n, 6)
        W = (n + 63) // 64
        d2, words = np.zeros((n, n)), np.zeros((n, W), dtype=np.uint64)
        clique, size, proven = np.full(n, -1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        st = self._joint_call("cgmr_closure_consistency_exact", poses, fixed, ef, et, meas, info,
                              (C.c_int(n), _ptr(a), _ptr(b), _ptr(cm), _ptr(ci), C.c_double(float(gamma)), _ptr(d2), _ptr(words),
                               C.c_int64(int(node_limit)), _ptr(clique), _ptr(size), _ptr(proven)), kind, delta)
        return (d2, self._adj_bool(words, n), clique[:int(size[0])].copy(), bool(proven[0])) + st

    def max_clique_exact(self, adj, node_limit=EXACT_DEFAULT_NODE_LIMIT):
        """``(clique, proven, nodes)`` of a symmetric adjacency with a clear diagonal, given as for max_clique_greedy: a maximum
        clique (members ascending) by branch and bound behind the greedy one (cgmr_max_clique_exact).  Every root's search
        stops after ``node_limit`` nodes in each of its EXACT_ROUNDS rounds; ``proven`` is True when none was stopped in its
        last round -- then the size is the clique number --, otherwise the clique is the best found, never smaller than the
        greedy one.  ``nodes``: the nodes expanded, at most n * EXACT_ROUNDS * node_limit.  Deterministic."""
        words, n = self._adj_words(adj)
        clique, size, proven = np.full(n, -1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        nodes = np.zeros(1, dtype=np.int64)
        self._check(self.lib.cgmr_max_clique_exact(self.h, C.c_int(n), _ptr(words), C.c_int64(int(node_limit)), _ptr(clique),
                                                   _ptr(size), _ptr(proven), _ptr(nodes)))
        return clique[:int(size[0])].copy(), bool(proven[0]), int(nodes[0])

    # inter-robot PCM: candidates that end at a peer's vertex (include/cgmr.h: cgmr_closure_consistency_inter)
    @staticmethod
    def _inter_arrays(cl_a, peer_pose, peer_cov, cl_meas, cl_info):
        a = np.ascontiguousarray(cl_a, dtype=np.int32).reshape(-1)
        n = len(a)
        pp = np.ascontiguousarray(peer_pose, dtype=np.float64).reshape(n, 3)
        pc = None
        if peer_cov is not None:
            pc = np.ascontiguousarray(peer_cov, dtype=np.float64)
            if pc.shape != (3 * n, 3 * n):
                raise ValueError(f"peer_cov: [{3 * n}, {3 * n}] for {n} candidates, not {pc.shape}")
        cm = np.ascontiguousarray(cl_meas, dtype=np.float64).reshape(n, 3)
        ci = np.ascontiguousarray(cl_info, dtype=np.float64).reshape(n, 6)
        return a, pp, pc, cm, ci

    def closure_consistency_inter(self, poses, fixed, ef, et, meas, info, cl_a, peer_pose, cl_meas, cl_info, gamma, peer_cov=None,
                                  kind=None, delta=1.0):
        """closure_consistency for N candidates between this graph and a peer robot's: candidate k goes from the own vertex
        ``cl_a[k]`` to a peer vertex that is in no graph, known by the pose ``peer_pose[k]`` the peer sent (its frame does not
        matter: only p_k^-1 p_l enters).  ``peer_cov`` [3 N, 3 N]: the joint covariance of the peer poses, indexed by candidate
        (only its lower triangle is read); None: the peer's poses are taken as exact, which under-states the loop's covariance
        -- the gate is then stricter than the data justify.  Returns ``(d2, adj, clique, seed)`` as closure_consistency;
        ``kind`` / ``delta``: robust kernels on the graph's edges, (e2, weights) appended."""
        a, pp, pc, cm, ci = self._inter_arrays(cl_a, peer_pose, peer_cov, cl_meas, cl_info)
        n = len(a)
        W = (n + 63) // 64
        d2, words = np.zeros((n, n)), np.zeros((n, W), dtype=np.uint64)
        clique, size, seed = np.full(n, -1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
        st = self._joint_call("cgmr_closure_consistency_inter", poses, fixed, ef, et, meas, info,
                              (C.c_int(n), _ptr(a), _ptr(pp), _ptr(pc), _ptr(cm), _ptr(ci), C.c_double(float(gamma)), _ptr(d2),
                               _ptr(words), _ptr(clique), _ptr(size), _ptr(seed)), kind, delta)
        return (d2, self._adj_bool(words, n), clique[:int(size[0])].copy(), int(seed[0])) + st

    def closure_consistency_inter_exact(self, poses, fixed, ef, et, meas, info, cl_a, peer_pose, cl_meas, cl_info, gamma,
                                        peer_cov=None, node_limit=EXACT_DEFAULT_NODE_LIMIT, kind=None, delta=1.0):
        """closure_consistency_inter with the exact maximum clique of adj (cgmr_closure_consistency_inter_exact): ``(d2, adj,
        clique, proven)``, as closure_consistency_exact."""
        a, pp, pc, cm, ci = self._inter_arrays(cl_a, peer_pose, peer_cov, cl_meas, cl_info)
        n = len(a)
        W = (n + 63) // 64
        d2, words = np.zeros((n, n)), np.zeros((n, W), dtype=np.uint64)
        clique, size, proven = np.full(n, -1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        st = self._joint_call("cgmr_closure_consistency_inter_exact", poses, fixed, ef, et, meas, info,
                              (C.c_int(n), _ptr(a), _ptr(pp), _ptr(pc), _ptr(cm), _ptr(ci), C.c_double(float(gamma)), _ptr(d2),
                               _ptr(words), C.c_int64(int(node_limit)), _ptr(clique), _ptr(size), _ptr(proven)), kind, delta)
        return (d2, self._adj_bool(words, n), clique[:int(size[0])].copy(), bool(proven[0])) + st

    # joint-compatibility data association of landmark observations (include/cgmr.h: cgmr_jcbb_dense, cgmr_joint_compatibility)
    @staticmethod
    def _jc_outputs(nM, nL):
        return (np.zeros((nM, nL)), np.full(nM, -1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1),
                np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64))

    @staticmethod
    def _jc_gamma(gamma_by_dof, nM):
        g = np.ascontiguousarray(JC_GAMMA_99 if gamma_by_dof is None else gamma_by_dof, dtype=np.float64).reshape(-1)
        if len(g) < 2 * nM + 1:
            raise ValueError(f"gamma_by_dof: {len(g)} entries, {2 * nM + 1} needed (index = degrees of freedom, 0 unused)")
        return np.ascontiguousarray(g[:2 * nM + 1])

    def jcbb_dense(self, obs_pose_slot, obs_dim, sigma, e, J, R_upper, gamma_by_dof=None, node_limit=JC_DEFAULT_NODE_LIMIT):
        """Joint compatibility branch and bound on a caller's covariance (cgmr_jcbb_dense): M observations, observation i made
        from pose ``obs_pose_slot[i]`` in dimension ``obs_dim[i]`` (2 xy, 1 bearing), against L landmarks.  ``sigma``
        [3 nA + 2 L, 3 nA + 2 L]: the poses first, then the landmarks (the lower triangle is read); ``e`` [M, L, 2], ``J``
        [M, L, 2, 5] the innovation and Jacobian of every pair, ``R_upper`` [M, 3] = (R00, R01, R11).  ``gamma_by_dof``: the
        thresholds by degrees of freedom (None: JC_GAMMA_99).  Returns ``(assign [M] landmark positions or -1, count, d2, dof,
        proven, ic [M, L], nodes)``: the admissible hypothesis with the most pairings, among those the smallest joint d2;
        ``proven`` False: some root's search stopped at ``node_limit``, the result is the best found.  Deterministic."""
        slot = np.ascontiguousarray(obs_pose_slot, dtype=np.int32).reshape(-1)
        dim = np.ascontiguousarray(obs_dim, dtype=np.int32).reshape(-1)
        nM = len(slot)
        sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        e = np.ascontiguousarray(e, dtype=np.float64).reshape(nM, -1, 2) if nM else np.zeros((0, 0, 2))
        nL = e.shape[1]
        nA = (sigma.shape[0] - 2 * nL) // 3
        if dim.shape != (nM,) or sigma.shape != (3 * nA + 2 * nL, 3 * nA + 2 * nL) or nA < 0:
            raise ValueError(f"jcbb_dense: {nM} observations, {nL} landmarks, sigma {sigma.shape}")
        J = np.ascontiguousarray(J, dtype=np.float64).reshape(nM, nL, 2, 5)
        R = np.ascontiguousarray(R_upper, dtype=np.float64).reshape(nM, 3)
        g = self._jc_gamma(gamma_by_dof, nM)
        ic, assign, count, d2, dof, proven, nodes = self._jc_outputs(nM, nL)
        self._check(self.lib.cgmr_jcbb_dense(self.h, C.c_int(nM), C.c_int(nL), C.c_int(nA), _ptr(slot), _ptr(dim), _ptr(sigma), _ptr(e),
                                             _ptr(J), _ptr(R), _ptr(g), C.c_int64(int(node_limit)), _ptr(ic), _ptr(assign),
                                             _ptr(count), _ptr(d2), _ptr(dof), _ptr(proven), _ptr(nodes)))
        return assign, int(count[0]), float(d2[0]), int(dof[0]), bool(proven[0]), ic, int(nodes[0])

    def joint_compatibility(self, poses, fixed, ef, et, meas, info, obs_pose, obs_kind, obs_meas, obs_info, landmarks,
                            gamma_by_dof=None, node_limit=JC_DEFAULT_NODE_LIMIT, vertex_kind=None, edge_kind=None, kind=None,
                            delta=1.0):
        """jcbb_dense on the graph's own covariance (cgmr_joint_compatibility): observation i made from pose vertex
        ``obs_pose[i]`` as a factor of ``obs_kind[i]`` (1 EDGE_SE2_XY, 2 EDGE_BEARING_SE2_XY) with ``obs_meas`` [M, 3] /
        ``obs_info`` [M, 6] (or None: no measurement noise) read as observation_covariance reads a hypothesis; ``landmarks``:
        the candidate point vertices.  Returns jcbb_dense's tuple with ``assign`` in vertex indices; ``kind`` / ``delta``:
        robust kernels, (e2, weights) appended."""
        op = np.ascontiguousarray(obs_pose, dtype=np.int32).reshape(-1)
        nM = len(op)
        ok = np.ascontiguousarray(obs_kind, dtype=np.uint8).reshape(-1)
        if ok.shape != (nM,):
            raise ValueError(f"observation kinds: {ok.shape[0]} given for {nM} observations")
        om = np.ascontiguousarray(obs_meas, dtype=np.float64).reshape(nM, 3)
        oi = None if obs_info is None else np.ascontiguousarray(obs_info, dtype=np.float64).reshape(nM, 6)
        lm = np.ascontiguousarray(landmarks, dtype=np.int32).reshape(-1)
        nL = len(lm)
        g = self._jc_gamma(gamma_by_dof, nM)
        ic, assign, count, d2, dof, proven, nodes = self._jc_outputs(nM, nL)
        st = self._joint_call("cgmr_joint_compatibility", poses, fixed, ef, et, meas, info,
                              (C.c_int(nM), _ptr(op), _ptr(ok), _ptr(om), _ptr(oi), C.c_int(nL), _ptr(lm), _ptr(g),
                               C.c_int64(int(node_limit)), _ptr(ic), _ptr(assign), _ptr(count), _ptr(d2), _ptr(dof), _ptr(proven),
                               _ptr(nodes)), kind, delta, vertex_kind, edge_kind, typed=True)
        return (assign, int(count[0]), float(d2[0]), int(dof[0]), bool(proven[0]), ic, int(nodes[0])) + st

    def set_symbolic_cache(self, on: bool):
        """Reuse of the ordering / symbolic analysis / structure upload across calls on the same edge list (default on)."""
        self._check(self.lib.cgmr_set_symbolic_cache(self.h, C.c_int(1 if on else 0)))

    def host_threads_info(self):
        """Threads behind the symbolic analysis: {threads, pinned, home_cpu, cpus_allowed, moves} (cgmr_host_threads_info)."""
        out = np.zeros(5, dtype=np.int32)
        self._check(self.lib.cgmr_host_threads_info(_ptr(out)))
        return {"threads": int(out[0]), "pinned": bool(out[1]), "home_cpu": int(out[2]), "cpus_allowed": int(out[3]),
                "moves": int(out[4])}

    def symbolic_cache_stats(self):
        out = np.zeros(3, dtype=np.int64)
        self._check(self.lib.cgmr_symbolic_cache_stats3(self.h, _ptr(out)))
        return {"hits": int(out[0]), "misses": int(out[1]), "extended": int(out[2])}

    def gn_timeouts(self) -> int:
        """Bounded device-side waits of the chained backward solve that ran out on this context (cgmr_gn_timeouts)."""
        self.lib.cgmr_gn_timeouts.restype = C.c_int64
        return int(self.lib.cgmr_gn_timeouts(self.h))

    def switches(self):
        """The environment switches this context holds (cgmr_switches): {name: value}, read when the context was created
        (the process-scoped ones: when the process first needed them).  Flags and numbers are ints, a path is a string."""
        return {r["name"]: r["value"] for r in _switch_rows(self.lib, self.h)}

    def gn_last_timing(self):
        out = np.zeros(5)
        self._check(self.lib.cgmr_gn_last_timing(self.h, _ptr(out)))
        return dict(zip(["order", "structure", "upload", "device", "total"], out.tolist()))

    def set_profiling(self, on: bool):
        self._check(self.lib.cgmr_set_profiling(self.h, C.c_int(1 if on else 0)))

    def gn_kernel_times(self):
        sec = np.zeros(12)
        n = np.zeros(12, dtype=np.int64)
        self._check(self.lib.cgmr_gn_kernel_times_ex(self.h, _ptr(sec), _ptr(n)))
        names = ["linearize", "assemble", "chi2", "front_factor", "front_update", "top_block", "solve_bwd", "update", "front_level"]
        return {k: (float(s), int(c)) for k, s, c in zip(names, sec, n)}

    def pcm_kernel_times(self):
        """Profiling mode, classes 9..11 of cgmr_gn_kernel_times_ex: what closure_consistency spent in the forward solve and the
        Gram tiles, in k_closure_consistency, and in the bit words and the clique (max_clique_greedy: the clique alone;
        min_spanning_tree and condense_tree count their spanning-tree launch into the same class);
        (seconds, launches) each, added up since set_profiling(True)."""
        sec = np.zeros(12)
        n = np.zeros(12, dtype=np.int64)
        self._check(self.lib.cgmr_gn_kernel_times_ex(self.h, _ptr(sec), _ptr(n)))
        return {k: (float(sec[i]), int(n[i])) for i, k in zip((9, 10, 11), ("gram", "consistency", "bits_clique"))}


def _switch_rows(lib, h):
    need = lib.cgmr_switches(h, None, C.c_int(0))
    if need <= 0:
        raise CgmrError(need, "cgmr_switches failed")
    buf = C.create_string_buffer(need)
    lib.cgmr_switches(h, buf, C.c_int(need))
    rows = []
    for line in buf.value.decode().splitlines():
        name, scope, value, effect = line.split("\t")
        rows.append(dict(name=name, scope=scope, value=int(value) if value.lstrip("-").isdigit() else value, effect=effect))
    return rows


def switch_table():
    """Every environment switch of the library (csrc/switches.h), no device needed: a list of dict(name, scope, value, effect)
    with ``value`` the default."""
    return _switch_rows(load_library(), None)


_SYM_KEYS = ["free_poses", "offdiag_blocks", "fronts", "levels", "L_doubles", "U_doubles", "max_border",
             "factor_flops", "order_us", "structure_us", "max_children", "max_children_small_border", "panel_doubles",
             "launch_levels", "top_block_fronts", "top_block_cols"]


def gn_symbolic_info_grown(nV0, nE0, nV_steps, nE_steps, ef, et):
    """Host-only: analyse the first (nV0, nE0) vertices / edges, then extend step by step (the key-frame pattern).  Returns
    (info of the last analysis, its vertex -> column permutation, number of steps that re-used the ordering)."""
    lib = load_library()
    ef = np.ascontiguousarray(ef, dtype=np.int32)
    et = np.ascontiguousarray(et, dtype=np.int32)
    nv = np.ascontiguousarray(nV_steps, dtype=np.int32)
    ne = np.ascontiguousarray(nE_steps, dtype=np.int32)
    out = np.zeros(16, dtype=np.int64)
    nV = int(nv[-1]) if len(nv) else nV0
    perm = np.zeros(nV, dtype=np.int32)
    next_ = C.c_int32(0)
    rc = lib.cgmr_gn_symbolic_info_grown(C.c_int(nV0), C.c_int(nE0), C.c_int(len(nv)), _ptr(nv), _ptr(ne), _ptr(ef), _ptr(et),
                                         _ptr(out), _ptr(perm), C.byref(next_))
    if rc != 0:
        raise CgmrError(rc, "cgmr_gn_symbolic_info_grown rejected the graph")
    return dict(zip(_SYM_KEYS, out.tolist())), perm, int(next_.value)


def gn_front_table(nV, fixed, ef, et):
    """Host-only: the fronts of the elimination tree, one row each: (first block column, block columns, border block
    rows, parent, level, children) -- cgmr_debug_fronts."""
    lib = load_library()
    fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
    ef = np.ascontiguousarray(ef, dtype=np.int32)
    et = np.ascontiguousarray(et, dtype=np.int32)
    cap = max(64, int(nV))
    out = np.zeros(6 * cap, dtype=np.int32)
    n = lib.cgmr_debug_fronts(C.c_int(nV), _ptr(fixed), C.c_int(len(ef)), _ptr(ef), _ptr(et), C.c_int(cap), _ptr(out))
    if n < 0 or n > cap:
        raise CgmrError(n, "cgmr_debug_fronts rejected the graph")
    return out[:6 * n].reshape(n, 6)


def gn_symbolic_info(nV, fixed, ef, et, want_perm=False):
    """Host-only ordering / symbolic analysis statistics (no GPU needed)."""
    lib = load_library()
    fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
    ef = np.ascontiguousarray(ef, dtype=np.int32)
    et = np.ascontiguousarray(et, dtype=np.int32)
    out = np.zeros(16, dtype=np.int64)
    perm = np.zeros(nV, dtype=np.int32) if want_perm else None
    rc = lib.cgmr_gn_symbolic_info(C.c_int(nV), _ptr(fixed), C.c_int(len(ef)), _ptr(ef), _ptr(et), _ptr(out),
                                   _ptr(perm))
    if rc != 0:
        raise CgmrError(rc, "cgmr_gn_symbolic_info rejected the graph")
    keys = ["free_poses", "offdiag_blocks", "fronts", "levels", "L_doubles", "U_doubles", "max_border",
            "factor_flops", "order_us", "structure_us", "max_children", "max_children_small_border", "panel_doubles",
            "launch_levels", "top_block_fronts", "top_block_cols"]
    info = dict(zip(keys, out.tolist()))
    return (info, perm) if want_perm else info
