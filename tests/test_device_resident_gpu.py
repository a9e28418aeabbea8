"""The device-pointer entry points no other test reaches (include/cgmr.h: cgmr_lm_optimize_dev, cgmr_dl_optimize_dev plain and
with robust kinds / deltas as device arrays, cgmr_gn / lm / dl_optimize_typed_dev, cgmr_chordal_initialize_typed_dev,
cgmr_match_close_vset_batch_dev with cgmr_scan_transforms), each against its host twin, bit for bit -- the same launches on
the same bytes -- and the twin in the same test against the float64 reference its own file holds it to, at that file's bar:
tests/test_lm_gpu.py and tests/test_dogleg_gpu.py (check_trace), tests/test_typed_gpu.py (chi2 at CHI_RTOL, a step within
OMEGA_MAX), tests/test_chordal_gpu.py (_check), tests/test_matcher_config_gpu.py (the oracle, bit for bit).  A _dev call must
leave its measurements and information untouched and write nothing behind the 3 nV doubles of its poses.  Also: both staging
paths of cgmr_match_close_vset_batch, one batch on each side of the 4 MiB threshold."""
import ctypes as C

import numpy as np
import pytest

import chordal_cases as CC
import ref_dogleg
import ref_lm
import ref_robust as RR
import ref_typed as T
import reference_cases as RC
import test_dogleg_gpu as DL
import test_lm_gpu as LM
import typed_cases as TC
import vset_cases as VC
from test_chordal_gpu import _check as chordal_check
from test_matcher_config_gpu import MAX_SCORE, N_FULL, _matcher, _same

pytestmark = pytest.mark.gpu

ITERS = 4
GUARD = 64                     # doubles behind the poses of a _dev call
GUARD_VALUE = -7.25


@pytest.fixture(scope="module")
def ctx():
    from cg_mrslam_amd import Context
    c = Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class DeviceProblem:
    """Fresh device tensors of a graph: the poses with GUARD doubles behind them, measurements, information."""

    def __init__(self, g):
        import torch
        self.g, self.nV = g, len(g["poses"])
        host = np.full(3 * self.nV + GUARD, GUARD_VALUE)
        host[:3 * self.nV] = np.ascontiguousarray(g["poses"], dtype=np.float64).reshape(-1)
        self.d_p, self.d_m, self.d_i = _dev(host), _dev(np.asarray(g["meas"], np.float64)), _dev(np.asarray(g["info"], np.float64))
        torch.cuda.synchronize()      # (torch's stream and the context's are not ordered against each other)

    def args(self):
        g = self.g
        return (self.d_p.data_ptr(), self.nV, g["fixed"], g["edge_from"], g["edge_to"], self.d_m.data_ptr(), self.d_i.data_ptr())

    def check(self, host_poses, what):
        """The poses equal the host twin's, the guard, the measurements and the information are as they were: byte for byte."""
        import torch
        torch.cuda.synchronize()
        p = self.d_p.cpu().numpy()
        assert p[:3 * self.nV].tobytes() == np.ascontiguousarray(host_poses, dtype=np.float64).tobytes(), (what, "poses")
        assert np.all(p[3 * self.nV:] == GUARD_VALUE), (what, "written behind the poses", p[3 * self.nV:])
        assert self.d_m.cpu().numpy().tobytes() == np.asarray(self.g["meas"], np.float64).tobytes(), (what, "meas")
        assert self.d_i.cpu().numpy().tobytes() == np.asarray(self.g["info"], np.float64).tobytes(), (what, "info")


def _records_equal(dev, host, what):
    """Every returned array of the _dev call (status first) against the host twin's (status, poses, then the same)."""
    assert dev[0] == host[0], (what, dev[0], host[0])
    assert len(dev) == len(host) - 1, what
    for k, (a, b) in enumerate(zip(dev[1:], host[2:])):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (what, "returned array", k, a, b)


# ------------------------------------------------------------------------------------ Levenberg-Marquardt, dogleg: plain
@pytest.mark.parametrize("name", ["pg500", "v5e4"])
def test_lm_and_dogleg_dev_equal_their_host_twins_and_the_reference(ctx, name):
    g = RC.CASES[name][0]()
    a = RC.args(g)
    floor = LM.rounding_floor(g)
    # Levenberg-Marquardt
    host = ctx.lm_optimize(*a, ITERS)
    assert host[0] == 0
    k = LM.check_trace(name, ref_lm.lm_optimize(*a, ITERS), *host[2:], floor)
    assert k >= 1 or name == "v5e4", (name, "nothing compared")      # (v5e4 starts at its optimum to rounding)
    dp = DeviceProblem(g)
    dev = ctx.lm_optimize_dev(*dp.args(), ITERS)
    _records_equal(dev, host, name + " lm")
    dp.check(host[1], name + " lm")
    # dogleg
    host = ctx.dl_optimize(*a, ITERS)
    assert host[0] == 0
    k = DL.check_trace(name, ref_dogleg.dl_optimize(*a, ITERS), *host[2:], floor)
    assert k >= 1 or name == "v5e4", (name, "nothing compared")
    dp = DeviceProblem(g)
    dev = ctx.dl_optimize_dev(*dp.args(), ITERS)
    _records_equal(dev, host, name + " dl")
    dp.check(host[1], name + " dl")


# ------------------------------------------------------------------------------------ dogleg: robust kinds and deltas on the device
def test_dogleg_dev_with_device_kinds_and_deltas(ctx):
    """pg500 with the mixed settings of tests/test_robust_gpu.py: Huber on the closures with seven deltas, nothing on the
    odometry chain.  The _dev call reads the kinds and deltas back once to check them and hands the device arrays on."""
    name = "pg500"
    g = RC.CASES[name][0]()
    a = RC.args(g)
    nV, nE = len(g["poses"]), len(g["edge_from"])
    closure = np.arange(nE) >= nV - 1                        # (the odometry chain comes first)
    kind = np.where(closure, 1, 0).astype(np.uint8)
    delta = np.where(closure, 0.5 + (np.arange(nE) % 7) * 0.25, 1.0)
    assert (RR.weights(*a[:1], *a[2:], kind, delta) < 1).sum() > 100      # (the kernels are at work from the first linearisation)
    host = ctx.dl_optimize(*a, ITERS, kind=kind, delta=delta)
    assert host[0] == 0
    ref = ref_dogleg.dl_optimize(*a, ITERS, kind=kind, delta=delta)
    k = DL.check_trace(name, ref, *host[2:7], LM.rounding_floor(g))
    assert k >= 1, "nothing compared"
    e2, w = host[7], host[8]
    np.testing.assert_allclose(w, RR.rho(kind, delta, e2)[1], rtol=1e-12, atol=1e-300)       # tests/test_dogleg_gpu.py's bar
    assert np.all(w[~closure] == 1.0) and (w[closure] < 1).any()
    dp = DeviceProblem(g)
    d_k, d_d = _dev(kind), _dev(delta)
    import torch
    torch.cuda.synchronize()
    dev = ctx.dl_optimize_dev(*dp.args(), ITERS, d_kind_ptr=d_k.data_ptr(), d_delta_ptr=d_d.data_ptr())
    _records_equal(dev, host, "dl robust")
    dp.check(host[1], "dl robust")
    assert d_k.cpu().numpy().tobytes() == kind.tobytes() and d_d.cpu().numpy().tobytes() == delta.tobytes()
    # ... and the plain call is another answer: the comparison above is not about kernels that do nothing
    assert not np.array_equal(ctx.dl_optimize(*a, ITERS)[2], host[2])


# ------------------------------------------------------------------------------------ typed Gauss-Newton, LM, dogleg
def _iterations_above_the_floor(ref_chi2, floor):
    """How many iterations (ITERS at most) a trust-region call is run for: as long as the REFERENCE's chi2 stays above the
    rounding floor of the case (tests/test_lm_gpu.py's rounding_floor).  A chi2 below it is made of rounded residuals, two
    correct solvers do not agree on it to 1e-9, and check_trace of tests/test_lm_gpu.py compares the chi2 an iteration
    starts from before it looks at the floor.  wrap_prior (two poses, started 0.1 m from its optimum) gets there after two
    iterations; the other cases run all ITERS."""
    n = 0
    while n < ITERS and n + 1 < len(ref_chi2) and ref_chi2[n + 1] > floor:
        n += 1
    assert n >= 1 and ref_chi2[0] > floor
    return n


@pytest.mark.parametrize("name", ["mixed257", "tree600", "wrap_prior"])
def test_typed_dev_equal_their_host_twins_and_the_reference(ctx, name):
    _, why, reach = TC.CASES[name]
    g = TC.case(name)
    assert reach(g), why
    vk, ek = TC.kinds(g)
    a = TC.args(g)
    kw = dict(vertex_kind=vk, edge_kind=ek)
    floor = LM.rounding_floor(g)
    # Gauss-Newton: chi2 before every iteration, one step's backward error
    host = ctx.gn_optimize_typed(*a, ITERS, **kw)
    assert host[0] == 0
    _, chi_ref, _ = T.gn_optimize(*a, ITERS, vk, ek)
    np.testing.assert_allclose(host[2], chi_ref, rtol=TC.CHI_RTOL, atol=1e-18)
    one = ctx.gn_optimize_typed(*a, 1, **kw)
    om = T.step_backward_error(g["poses"], one[1], *a[1:], vk, ek)
    assert one[0] == 0 and om <= TC.OMEGA_MAX, (name, om / T.U)
    for iters, h in ((ITERS, host), (1, one)):
        dp = DeviceProblem(g)
        dev = ctx.gn_optimize_typed_dev(*dp.args(), iters, **kw)
        _records_equal(dev, h, f"{name} gn {iters}")
        dp.check(h[1], f"{name} gn {iters}")
        assert np.all(h[1][vk == 1, 2] == 0.0)
    # Levenberg-Marquardt
    n_lm = _iterations_above_the_floor(T.lm_optimize(*a, ITERS, vk, ek)["chi2"], floor)
    host = ctx.lm_optimize_typed(*a, n_lm, **kw)
    assert host[0] == 0
    k_lm = LM.check_trace(name, T.lm_optimize(*a, n_lm, vk, ek), *host[2:], floor)
    dp = DeviceProblem(g)
    dev = ctx.lm_optimize_typed_dev(*dp.args(), n_lm, **kw)
    _records_equal(dev, host, name + " lm")
    dp.check(host[1], name + " lm")
    # dogleg
    n_dl = _iterations_above_the_floor(T.dl_optimize(*a, ITERS, vk, ek)["chi2"], floor)
    host = ctx.dl_optimize_typed(*a, n_dl, **kw)
    assert host[0] == 0
    k_dl = DL.check_trace(name, T.dl_optimize(*a, n_dl, vk, ek), *host[2:], floor)
    dp = DeviceProblem(g)
    dev = ctx.dl_optimize_typed_dev(*dp.args(), n_dl, **kw)
    _records_equal(dev, host, name + " dl")
    dp.check(host[1], name + " dl")
    print(f"{name}: omega {om / T.U:.1f} u; LM {n_lm} iterations, {k_lm} compared with the reference; dogleg {n_dl}, {k_dl}")
    assert name != "mixed257" or (k_lm >= 1 and k_dl >= 1), "nothing compared"       # (as tests/test_typed_gpu.py asks of it)


# ------------------------------------------------------------------------------------ chordal initialisation, typed
@pytest.mark.parametrize("stages", [1, 2, 3])
@pytest.mark.parametrize("name", list(CC.TYPED))
def test_chordal_typed_dev_equals_its_host_twin_and_the_reference(ctx, name, stages):
    """The _dev call decides which vertices a stage's terms touch from the information it reads back from the device."""
    g = CC.case(name)
    kw = CC.kinds(g)
    assert kw, name
    host = ctx.chordal_initialize(*CC.args(g), stages, **kw)
    chordal_check(name, stages, host)
    dp = DeviceProblem(g)
    dev = ctx.chordal_initialize_dev(*dp.args(), stages, **kw)
    assert dev["status"] == host["status"] == 0 and "poses" not in dev
    assert dev["chi2"].tobytes() == host["chi2"].tobytes() and dev["counts"].tobytes() == host["counts"].tobytes()
    dp.check(host["poses"], f"{name} stages {stages}")


# ------------------------------------------------------------------------------------ the matcher: reference sets of several scans
def _vset_host(m, ref, rel, cur, guess, want_nres):
    """cgmr_match_close_vset_batch with or without out_nresults (ScanMatcher.closeScanMatchingVSetBatch passes none)."""
    rr = np.ascontiguousarray(ref, dtype=np.float32)
    P, S, B = rr.shape
    rq = np.ascontiguousarray(cur, dtype=np.float32).reshape(P, B)
    rl = np.ascontiguousarray(rel, dtype=np.float64).reshape(P, S, 3)
    gs = np.ascontiguousarray(guess, dtype=np.float64).reshape(P, 3)
    xyt, score, found, nres = np.zeros((P, 3)), np.zeros(P), np.zeros(P, dtype=np.uint8), np.full(P, 7, dtype=np.int32)
    rc = m.ctx.lib.cgmr_match_close_vset_batch(m.ctx.h, C.byref(m.cfg), C.c_int(P), C.c_int(S), C.c_void_p(rr.ctypes.data),
                                               C.c_void_p(rl.ctypes.data), C.c_void_p(rq.ctypes.data), C.c_void_p(gs.ctypes.data),
                                               C.c_double(MAX_SCORE), C.c_void_p(xyt.ctypes.data), C.c_void_p(score.ctypes.data),
                                               C.c_void_p(found.ctypes.data), C.c_void_p(nres.ctypes.data if want_nres else 0))
    m.ctx._check(rc)
    return (found.astype(bool), xyt, score) + ((nres,) if want_nres else ())


@pytest.mark.parametrize("name", VC.VSET_ENTRIES)
def test_vset_dev_equals_the_oracle_and_the_host_call(ctx, oracle, name):
    import torch
    cfg, ref, rel, cur, guess = VC.sets(name)
    want = VC.expected(oracle, name)
    m = _matcher(ctx, cfg)
    xf = m.scan_transforms(rel).reshape(VC.N_SETS, 3, 4)
    perm = np.random.default_rng(5).permutation(np.arange(N_FULL) % VC.N_SETS)
    for sel in (np.arange(VC.N_SETS), np.array([2]), perm):
        P = len(sel)
        host = m.closeScanMatchingVSetBatch(ref[sel], rel[sel], cur[sel], guess[sel], MAX_SCORE)
        _same(host, want, sel)
        d_r, d_t, d_q, d_g = (_dev(x[sel]) for x in (ref, xf, cur, guess))
        for nres in (False, True):
            d_x = torch.full((P, 3), 7.0, dtype=torch.float64, device="cuda:0")
            d_s = torch.full((P,), 7.0, dtype=torch.float64, device="cuda:0")
            d_f = torch.full((P,), 7, dtype=torch.uint8, device="cuda:0")
            d_n = torch.full((P,), 7, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            m.closeScanMatchingVSet_dev(d_r.data_ptr(), d_t.data_ptr(), d_q.data_ptr(), d_g.data_ptr(), P, 3, d_x.data_ptr(),
                                        d_s.data_ptr(), d_f.data_ptr(), maxScore=MAX_SCORE, d_nres=d_n.data_ptr() if nres else 0)
            torch.cuda.synchronize()
            assert set(np.unique(d_f.cpu().numpy()).tolist()) <= {0, 1}
            got = (d_f.cpu().numpy().astype(bool), d_x.cpu().numpy(), d_s.cpu().numpy()) + ((d_n.cpu().numpy(),) if nres else ())
            _same(got, want, sel)
            for u, v in zip(got[:3], host):
                assert u.tobytes() == v.tobytes()
            if not nres:
                assert np.all(d_n.cpu().numpy() == 7)             # (no pointer given: nothing written)
            for d, h in ((d_r, ref[sel]), (d_t, xf[sel]), (d_q, cur[sel]), (d_g, guess[sel])):      # the inputs: untouched
                assert d.cpu().numpy().tobytes() == np.ascontiguousarray(h).tobytes()


def test_vset_host_call_on_both_sides_of_the_staging_threshold(ctx, oracle):
    """cgmr_match_close_vset_batch stages an input of up to 4 MiB through the context's pinned block and copies a larger one
    straight from the caller's arrays: the ten sets tiled to the largest batch below the threshold and the smallest above it,
    both against the oracle's answer for the ten, row for row, with and without the result counts."""
    name = "kr_03"
    cfg, ref, rel, cur, guess = VC.sets(name)
    want = VC.expected(oracle, name)
    m = _matcher(ctx, cfg)
    B = cfg["n_beams"]
    P = VC.pairs_across_threshold(3, B)
    assert VC.in_bytes(P, 3, B) > VC.STAGING_THRESHOLD >= VC.in_bytes(P - 1, 3, B)
    for n in (P - 1, P):
        sel = np.arange(n) % VC.N_SETS
        assert ref[sel].nbytes + cur[sel].nbytes <= VC.in_bytes(n, 3, B)
        _same(m.closeScanMatchingVSetBatch(ref[sel], rel[sel], cur[sel], guess[sel], MAX_SCORE), want, sel)
        for nres in (False, True):
            _same(_vset_host(m, ref[sel], rel[sel], cur[sel], guess[sel], nres), want, sel)
    print(f"staging threshold: {B} beams, 3 scans per set: {P - 1} pairs = {VC.in_bytes(P - 1, 3, B)} bytes staged, "
          f"{P} pairs = {VC.in_bytes(P, 3, B)} bytes unstaged")
