"""Contexts created on a stream the caller owns (cgmr_ctx_create(device, hip_stream), Context(0, stream=...)): every other test
lets the library own its stream, and synchronises the whole device before a device-pointer call.  Here the inputs of a _dev
call are still being produced on the context's stream when the call is made (tests/stream_cases.py: a decoy, a device-side
delay, the real input), the host entry points, the matcher's table upload, the side stream of the asynchronous condensed
graphs and the teardown run on a torch.cuda.Stream(), and two contexts take turns.  Every comparison is bit for bit with the
same call made in the ordinary way -- which tests/test_device_resident_gpu.py and the files it names hold to the float64
references.  The matcher's results are compared with the oracle's directly (bit for bit as well, and the oracle's answer is
computed anyway), the robot graph's steps also with tests/test_robot_graph_reference_gpu.py's backward-error bar."""
import ctypes as C

import numpy as np
import pytest

import matcher_configs as MC
import reference_cases as RC
import stream_cases as SC
import typed_cases as TC
import vset_cases as VC
from cg_mrslam_amd import synth
from test_matcher_config_gpu import MAX_SCORE, _matcher, _same, _sp

pytestmark = pytest.mark.gpu

N_PAIRS = 10
_CACHE = {}


@pytest.fixture(scope="module")
def own():
    """A context that owns its stream, as every other test's: what a caller-stream context is compared with."""
    from cg_mrslam_amd import Context
    c = Context(0)
    yield c
    c.close()
    if SC.MARGINS_MS:
        print(f"caller-stream tests: delay {SC._DELAY}, {len(SC.MARGINS_MS)} late calls, inputs still pending for "
              f"{min(SC.MARGINS_MS):.1f} .. {max(SC.MARGINS_MS):.1f} ms when the call was made")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _pairs(oracle, name):
    """(cfg, ranges_ref, ranges_cur, guess, the oracle's answer) of ten ordinary single-scan pairs at a table entry."""
    if name not in _CACHE:
        sp = _sp()
        cfg = MC.full_config(name, sp)
        rr, rq = (np.ascontiguousarray(sp[k][:N_PAIRS], dtype=np.float32) for k in ("ranges_ref", "ranges_qry"))
        g = np.ascontiguousarray(sp["guess"][:N_PAIRS], dtype=np.float64)
        _CACHE[name] = (cfg, rr, rq, g, MC.expected_close_batch(oracle, cfg, rr, rq, g, MAX_SCORE))
    return _CACHE[name]


def _pg500():
    if "pg500" not in _CACHE:
        _CACHE["pg500"] = RC.CASES["pg500"][0]()
    return _CACHE["pg500"]


def _mixed_robust(g):
    nV, nE = len(g["poses"]), len(g["edge_from"])
    closure = np.arange(nE) >= nV - 1
    return np.where(closure, 1, 0).astype(np.uint8), np.where(closure, 0.5 + (np.arange(nE) % 7) * 0.25, 1.0)


def _unit_info(n):
    return np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), (n, 1))


class LateInputs:
    """Device buffers whose real content arrives late on the caller's stream; ``sources`` / ``decoys``: host arrays."""

    def __init__(self, sources, decoys):
        import torch
        self.src = [_dev(a) for a in sources]
        self.dec = [_dev(a) for a in decoys]
        self.buf = [torch.empty_like(a) for a in self.src]
        for a, b in zip(sources, decoys):
            assert np.shape(a) == np.shape(b) and not np.array_equal(a, b)
        torch.cuda.synchronize()          # (setup: the sources and decoys are resident before anything is timed)

    def ptrs(self):
        return [b.data_ptr() for b in self.buf]

    def late(self, s):
        return SC.late(s, self.buf, self.src, self.dec)

    def settle(self, s, which):
        """The buffers filled with the sources (or the decoys) and everything waited for: the ordinary way to call."""
        import torch
        with torch.cuda.stream(s):
            for b, x in zip(self.buf, which):
                b.copy_(x)
        torch.cuda.synchronize()


def _equal(a, b, what):
    assert len(a) == len(b), what
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), (what, k, u, v)


def _flat(out):
    """A call's results as a list of arrays (dict results: by sorted key)."""
    if isinstance(out, dict):
        return [np.asarray(out[k]) for k in sorted(out)]
    return [np.asarray(x) for x in out]


def _run_late(s, li, call, n_out):
    """``call()`` made while ``li``'s inputs are still pending on ``s``, then after a full synchronise, then on the decoys:
    the first two agree bit for bit -- the results and the first ``n_out`` buffers --, the decoys give another answer."""
    assert n_out >= 2
    l = li.late(s)
    l.pending()
    got = _flat(call()) + SC.read(s, *li.buf[:n_out])
    margin = l.margin_ms()
    li.settle(s, li.src)
    want = _flat(call()) + SC.read(s, *li.buf[:n_out])
    li.settle(s, li.dec)
    other = _flat(call()) + SC.read(s, *li.buf[:n_out])
    return got, want, other, margin


# ------------------------------------------------------------------------------------------------------------------- 1
SOLVER_ENTRIES = ("gn_optimize_dev", "lm_optimize_robust_dev", "chordal_initialize_dev", "gn_optimize_typed_dev")


@pytest.mark.parametrize("entry", SOLVER_ENTRIES)
def test_solver_inputs_produced_late_on_the_contexts_stream(entry):
    typed = entry == "gn_optimize_typed_dev"
    g = TC.case("mixed257") if typed else _pg500()
    nV, nE = len(g["poses"]), len(g["edge_from"])
    s3 = (g["fixed"], g["edge_from"], g["edge_to"])
    other_poses = g["truth"] if typed else synth.make_pose_graph(nV, nE, seed=5)["poses"]     # (a valid start, another answer)
    sources = [np.ascontiguousarray(g[k], dtype=np.float64) for k in ("poses", "meas", "info")]
    decoys = [np.ascontiguousarray(other_poses, dtype=np.float64), np.zeros((nE, 3)), _unit_info(nE)]
    if entry == "chordal_initialize_dev":
        # the call reads the information back to decide which vertices a stage's terms touch: in the decoy no edge of the last
        # vertex carries heading information, which leaves that vertex out of the rotation stage (include/cgmr.h)
        last = (g["edge_from"] == nV - 1) | (g["edge_to"] == nV - 1)
        assert last.any() and not g["fixed"][nV - 1]
        decoys[2][np.ix_(last, [2, 4, 5])] = 0.0
    if entry == "lm_optimize_robust_dev":
        kind, delta = _mixed_robust(g)
        sources += [kind, delta]
        decoys += [np.zeros(nE, np.uint8), np.full(nE, 2.0)]
    li = LateInputs(sources, decoys)
    with SC.caller_context() as (c, s):
        p = li.ptrs()
        if entry == "gn_optimize_dev":
            call = lambda: c.gn_optimize_dev(p[0], nV, *s3, p[1], p[2], 3, raise_on_cholesky=False)   # noqa: E731
        elif entry == "lm_optimize_robust_dev":
            call = lambda: c.lm_optimize_robust_dev(p[0], nV, *s3, p[1], p[2], 3, d_kind_ptr=p[3], d_delta_ptr=p[4])   # noqa: E731
        elif entry == "chordal_initialize_dev":
            call = lambda: c.chordal_initialize_dev(p[0], nV, *s3, p[1], p[2], 3, raise_on_cholesky=False)   # noqa: E731
        else:
            call = lambda: c.gn_optimize_typed_dev(p[0], nV, *s3, p[1], p[2], 3, vertex_kind=g["vk"], edge_kind=g["ek"],   # noqa: E731
                                                   raise_on_cholesky=False)
        got, want, other, margin = _run_late(s, li, call, len(sources))
    print(f"{entry}: inputs still pending for {margin:.1f} ms when the call was made")
    _equal(got, want, entry)
    assert not np.array_equal(other[-len(sources)], want[-len(sources)]), (entry, "the decoy gives the same poses: it checks nothing")
    if entry == "chordal_initialize_dev":                # (results by sorted key: chi2, counts, status)
        assert want[1][0] == other[1][0] + 1, ("the decoy's information leaves no vertex out of the rotation stage", want[1], other[1])
    for k in range(1, len(sources)):                     # measurements, information, kinds, deltas: as they were given
        assert want[-len(sources) + k].tobytes() == np.ascontiguousarray(sources[k]).tobytes(), (entry, k)


def test_matcher_inputs_produced_late_on_the_contexts_stream(oracle):
    import torch
    name = "kr_03"
    cfg, rr, rq, g, want = _pairs(oracle, name)
    li = LateInputs([rr, rq, g], [np.zeros_like(rr), np.zeros_like(rq), np.zeros_like(g)])
    with SC.caller_context() as (c, s):
        m = _matcher(c, cfg)
        outs = [torch.full((N_PAIRS, 3), 7.0, dtype=torch.float64, device="cuda:0"), torch.full((N_PAIRS,), 7.0, dtype=torch.float64, device="cuda:0"),
                torch.full((N_PAIRS,), 7, dtype=torch.uint8, device="cuda:0"), torch.full((N_PAIRS,), 7, dtype=torch.int32, device="cuda:0")]
        torch.cuda.synchronize()
        l = li.late(s)
        l.pending()
        m.closeScanMatching_dev(*li.ptrs(), N_PAIRS, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), maxScore=MAX_SCORE,
                                d_nres=outs[3].data_ptr())
        x, sc, f, n = SC.read(s, *outs)
        print(f"closeScanMatching_dev: inputs still pending for {l.margin_ms():.1f} ms when the call was made")
    _same((f.astype(bool), x, sc, n), want)
    assert want[0].sum() >= 8                                 # (all-zero ranges, the decoy, match nothing)


def test_vset_matcher_inputs_produced_late_on_the_contexts_stream(oracle):
    import torch
    name = "kr_03"
    cfg, ref, rel, cur, guess = VC.sets(name)
    want = VC.expected(oracle, name)
    with SC.caller_context() as (c, s):
        m = _matcher(c, cfg)
        xf = m.scan_transforms(rel).reshape(VC.N_SETS, 3, 4)
        identity = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (VC.N_SETS, 3, 1))
        li = LateInputs([ref, xf, cur, guess], [np.zeros_like(ref), identity, np.zeros_like(cur), np.zeros_like(guess)])
        P = VC.N_SETS
        outs = [torch.full((P, 3), 7.0, dtype=torch.float64, device="cuda:0"), torch.full((P,), 7.0, dtype=torch.float64, device="cuda:0"),
                torch.full((P,), 7, dtype=torch.uint8, device="cuda:0"), torch.full((P,), 7, dtype=torch.int32, device="cuda:0")]
        torch.cuda.synchronize()
        l = li.late(s)
        l.pending()
        m.closeScanMatchingVSet_dev(*li.ptrs(), P, 3, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), maxScore=MAX_SCORE,
                                    d_nres=outs[3].data_ptr())
        x, sc, f, n = SC.read(s, *outs)
        print(f"closeScanMatchingVSet_dev: inputs still pending for {l.margin_ms():.1f} ms when the call was made")
    _same((f.astype(bool), x, sc, n), want)


# ------------------------------------------------------------------------------------------------------------------- 2
def test_host_entry_points_on_a_callers_stream(own, oracle):
    g = _pg500()
    a = RC.args(g)
    query = np.array([3, 77, 200, 410, 499], np.int32)
    e = (g["edge_from"], g["edge_to"], g["meas"], g["info"])
    cfg, ref, rel, cur, guess = VC.sets("kr_03")
    want = VC.expected(oracle, "kr_03")

    def calls(c):
        out = list(c.gn_optimize(*a, 3))
        out.append(c.marginals(*a, query))
        out += list(c.condense(g["poses"], *e, 50, query))
        out += list(_matcher(c, cfg).closeScanMatchingVSetBatch(ref, rel, cur, guess, MAX_SCORE))
        return out

    with SC.caller_context() as (c, s):
        got = calls(c)
        c.synchronize()
        assert s.query()
    ref_out = calls(own)
    _equal(got, ref_out, "host entry points")
    assert got[0] == 0 and len(got[4]) >= len(query) - 1      # (status of the optimisation; the condensed star's edges)
    _same(tuple(got[-3:]), want)


# ------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("late_inputs", [False, True])
def test_table_upload_behind_queued_work(oracle, late_inputs):
    """kr_03, res_004, kr_03 on one caller-stream context: the beam and kernel table of the context is rewritten for the second
    call and again for the third.  late_inputs: the second call is the device-pointer one, made while its inputs are still
    being produced on the stream -- the table is rewritten with work queued in front of it."""
    import torch
    a, b = _pairs(oracle, "kr_03"), _pairs(oracle, "res_004")
    with SC.caller_context() as (c, s):
        ma, mb = _matcher(c, a[0]), _matcher(c, b[0])
        _same(ma.closeScanMatching(a[1], a[2], a[3], maxScore=MAX_SCORE, want_nresults=True), a[4])
        if late_inputs:
            li = LateInputs([b[1], b[2], b[3]], [np.zeros_like(b[1]), np.zeros_like(b[2]), np.zeros_like(b[3])])
            outs = [torch.full((N_PAIRS, 3), 7.0, dtype=torch.float64, device="cuda:0"), torch.full((N_PAIRS,), 7.0, dtype=torch.float64, device="cuda:0"),
                    torch.full((N_PAIRS,), 7, dtype=torch.uint8, device="cuda:0"), torch.full((N_PAIRS,), 7, dtype=torch.int32, device="cuda:0")]
            torch.cuda.synchronize()
            l = li.late(s)
            l.pending()
            mb.closeScanMatching_dev(*li.ptrs(), N_PAIRS, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), maxScore=MAX_SCORE,
                                     d_nres=outs[3].data_ptr())
            x, sc, f, n = SC.read(s, *outs)
            l.margin_ms()
            _same((f.astype(bool), x, sc, n), b[4])
        else:
            _same(mb.closeScanMatching(b[1], b[2], b[3], maxScore=MAX_SCORE, want_nresults=True), b[4])
        _same(ma.closeScanMatching(a[1], a[2], a[3], maxScore=MAX_SCORE, want_nresults=True), a[4])
    assert not (np.array_equal(a[4][1], b[4][1]) and np.array_equal(a[4][2], b[4][2]))     # (the two tables give two answers)


# ------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("gn_on_caller", [True, False])
def test_two_contexts_interleaved(oracle, gn_on_caller):
    """A on a caller's stream, B on its own; Gauss-Newton on one, the matcher on the other, in turns, on four problems: each
    result equals the same sequence on a context nobody else runs beside."""
    from cg_mrslam_amd import Context
    g1, g2 = _pg500(), synth.make_pose_graph(300, 900, seed=23)
    p1, p2 = _pairs(oracle, "kr_03"), _pairs(oracle, "res_004")

    def gn(c, g):
        return list(c.gn_optimize(*RC.args(g), 3))

    def match(c, p):
        return list(_matcher(c, p[0]).closeScanMatching(p[1], p[2], p[3], maxScore=MAX_SCORE, want_nresults=True))

    b_ctx = Context(0)
    try:
        with SC.caller_context() as (a_ctx, s):
            cg, cm = (a_ctx, b_ctx) if gn_on_caller else (b_ctx, a_ctx)
            got = [gn(cg, g1), match(cm, p1), gn(cg, g2), match(cm, p2)]
    finally:
        b_ctx.close()
    alone = []
    for seq in ((lambda c: [gn(c, g1), gn(c, g2)]), (lambda c: [match(c, p1), match(c, p2)])):
        c = Context(0)
        try:
            alone.append(seq(c))
        finally:
            c.close()
    want = [alone[0][0], alone[1][0], alone[0][1], alone[1][1]]
    for k in range(4):
        _equal(got[k], want[k], ("call", k))
    _same(tuple(got[1]), p1[4])
    _same(tuple(got[3]), p2[4])
    assert got[0][0] == 0 and got[2][0] == 0


# ------------------------------------------------------------------------------------------------------------------- 5
ROBOT_CASE = (2, 1200, 4000, 44, 60, 7)       # tests/test_robot_graph_reference_gpu.py's 2robots, the first seven rounds


def _robot_rounds(streams):
    """The rounds of ROBOT_CASE with asynchronous condensed graphs and the device exchange, one context per robot, on the
    streams given (None: contexts that own theirs).  Returns (steps, final poses per robot, condensed graphs per robot and peer)."""
    import contextlib
    from cg_mrslam_amd import Context
    from robot_sequences import checked_rounds, make_robot_rounds
    nr, nv, ne, seed, chunk, n_rounds = ROBOT_CASE
    with contextlib.ExitStack() as stack:
        if streams is None:
            ctxs = [Context(0) for _ in range(nr)]
            for c in ctxs:
                stack.callback(c.close)
        else:
            ctxs = [Context(0, stream=s.cuda_stream) for s in streams]
            for c in ctxs:
                stack.callback(c.close)
        rounds = make_robot_rounds(ctxs, nv, ne, seed, chunk, async_condense=True)
        for rr in rounds:
            stack.callback(rr.g.close)
        steps, _, _ = checked_rounds(rounds, n_rounds, device=True)
        for rr in rounds:
            rr.g.condensed_wait()
        poses = [rr.g.poses() for rr in rounds]
        conds = [[rr.g.condensed(p) for p in range(nr) if p != rr.g.robot] for rr in rounds]
        assert [c.gn_timeouts() for c in ctxs] == [0] * nr
    return steps, poses, conds


def test_robot_graph_rounds_on_callers_streams():
    import torch
    from test_robot_graph_reference_gpu import _check_steps
    streams = [torch.cuda.Stream() for _ in range(ROBOT_CASE[0])]
    steps, poses, conds = _robot_rounds(streams)
    for s in streams:                                         # the streams are the caller's still
        s.synchronize()
    _, n_recv = _check_steps("caller streams, async, device exchange", steps)
    assert n_recv >= 2 and any(s["start"] == 3 and len(s["ef"]) > s["n_own"] for s in steps), n_recv
    assert sum(len(c[1]) for rob in conds for c in rob) >= 4, "no condensed graph was built"
    steps0, poses0, conds0 = _robot_rounds(None)
    assert len(steps) == len(steps0)
    for a, b in zip(steps, steps0):
        assert (a["t"], a["robot"], a["start"]) == (b["t"], b["robot"], b["start"])
        assert a["p0"].tobytes() == b["p0"].tobytes() and a["p1"].tobytes() == b["p1"].tobytes(), (a["t"], a["robot"], a["start"])
    for r in range(len(poses)):
        assert poses[r].tobytes() == poses0[r].tobytes(), r
        for x, y in zip(conds[r], conds0[r]):
            assert x[0] == y[0], r
            _equal(x[1:], y[1:], ("condensed", r))


# ------------------------------------------------------------------------------------------------------------------- 6
def test_accessors_and_teardown(own):
    import torch
    fn = own.lib.cgmr_ctx_stream
    fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p]
    assert fn(own.h)                                          # a context that owns its stream: not null
    assert fn(None) is None
    g = _pg500()
    with SC.caller_context() as (c, s):
        assert fn(c.h) == s.cuda_stream
        assert fn(c.h) != fn(own.h)
        d_p, d_m, d_i = _dev(g["poses"]), _dev(g["meas"]), _dev(g["info"])
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(SC.delay_cycles() // 10)
        assert c.gn_optimize_dev(d_p.data_ptr(), len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"], d_m.data_ptr(), d_i.data_ptr(), 2)[0] == 0
        with torch.cuda.stream(s):
            torch.cuda._sleep(SC.delay_cycles() // 10)
            x = torch.ones(1000, device="cuda:0")
        c.synchronize()
        assert s.query()
    # closed: the stream is the caller's and goes on working
    with torch.cuda.stream(s):
        y = (x * 3).sum()
    s.synchronize()
    assert s.query() and float(y) == 3000.0
    from cg_mrslam_amd import Context
    c3 = Context(0, stream=s.cuda_stream)                     # ... and so does the library, on the same stream again
    try:
        assert fn(c3.h) == s.cuda_stream
        assert c3.gn_optimize(*RC.args(g), 1)[0] == 0
    finally:
        c3.close()
    s.synchronize()
