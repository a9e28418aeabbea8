"""The wire kernels (mrslam_kernels.hip: k_wire_read, k_accept_gather_edges, k_gather_edges, k_wire_write_edges) against the
reference's own compiled serialiser, bit for bit: the records and decoded values come from tests/golden/msg_ref.npz (what
src/mrslam/msg_factory.cpp wrote and read back; tests/ref_msg_cases.py), never from a layout restated here.  They hold every
double whose narrowing to float32 can go wrong -- subnormal images, exact ties, one ulp beside a tie, the values around
FLT_MAX, signed zeros, infinities.  Shapes: three robots, 130 edges per slice (two 128-thread blocks with a ragged tail),
exactly full and nearly empty slices, accepted sets with holes, a kept set beside a fresh one.  Exact equality throughout."""
import os

import numpy as np
import pytest

import ref_msg_cases as RC
from cg_mrslam_amd.condensed import WIRE_EDGE_DTYPE, RobotGraph, wire_narrow_edges, wire_narrow_edges_batched
from cg_mrslam_amd.messages import from_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, CAP, ME = 3, 130, 1
HOLES = (40, 77)                       # sender 0's edges whose far end robot 1 does not know


@pytest.fixture(scope="module")
def fx():
    return RC.load_fixture(os.path.join(ROOT, "tests", "golden", "msg_ref.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _case(fx, name):
    """(input record, the reference's 44-byte records [n, 44] uint8, the reference's decoded record)"""
    rec, ref, dec = RC.fixture_case(fx, name)
    return rec, RC.wire_records(ref), dec


def _wire_buffer(sender, slices):
    """One rank's all-gather buffer (include/cgmr.h): ``slices`` = {peer: (records [n, 44] uint8, closure ids)}."""
    hdr = np.zeros(2 + 2 * R, dtype=np.int32)
    hdr[0], hdr[1] = sender, R
    edges = np.zeros((R, CAP, 44), dtype=np.uint8)
    clos = np.zeros((R, CAP), dtype=np.int32)
    for p, (recs, ids) in slices.items():
        hdr[2 + p], hdr[2 + R + p] = len(recs), len(ids)
        edges[p, :len(recs)] = recs
        clos[p, :len(ids)] = ids
    return np.concatenate([hdr.view(np.uint8), edges.reshape(-1), clos.view(np.uint8).reshape(-1)])


def _expect(dec, keep=None):
    k = np.arange(len(dec["from_to"])) if keep is None else keep
    return dec["from_to"][k, 0], dec["from_to"][k, 1], dec["edge_numbers"][k, :3], dec["edge_numbers"][k, 3:]


def _check_sets(g, want):
    """``want`` = {sender: (from, to, est, info)}: the staging (received_edges) and the solver's compact segment, exactly."""
    seg_m, seg_i = [], []
    for s in range(R):
        f, t, m, i = g.received_edges(s)
        if s not in want:
            assert len(f) == 0
            continue
        wf, wt, wm, wi = want[s]
        assert np.array_equal(f, wf) and np.array_equal(t, wt), s
        assert np.array_equal(_bits(m), _bits(wm)), s
        assert np.array_equal(_bits(i), _bits(wi)), s
        seg_m.append(wm)
        seg_i.append(wi)
    m, i = g.debug_received_segment()
    assert np.array_equal(_bits(m), _bits(np.concatenate(seg_m))) and np.array_equal(_bits(i), _bits(np.concatenate(seg_i)))


def test_read_side_equals_the_reference_decoder(ctx, fx):
    import torch
    _, rec130, dec130 = _case(fx, "condensed130")          # from robot 0
    _, rec1, dec1 = _case(fx, "condensed1")                # from robot 2
    _, rec3, dec3 = _case(fx, "condensed3")
    _, recE, decE = _case(fx, "edge130")                   # robot 2's ids
    assert len(rec130) == CAP == len(recE)
    # every hard float32 pattern the fixture has is in est and in info of sender 0's full slice
    with np.errstate(over="ignore"):
        hard = set(RC.HARD.astype(np.float32).view(np.uint32).tolist())
    f32 = np.ascontiguousarray(rec130[:, 8:]).view("<u4")
    assert hard <= set(f32[:, :3].reshape(-1).tolist()) and hard <= set(f32[:, 3:].reshape(-1).tolist())

    g = RobotGraph(ctx, ME, R, cap_edges=CAP)
    hole_ids = dec130["from_to"][list(HOLES), 1]
    known = np.setdiff1d(np.concatenate([d["from_to"].reshape(-1) for d in (dec130, dec1, dec3, decE)]), hole_ids)
    assert not np.isin(hole_ids, known).any() and np.isin(dec130["from_to"][:, 0], known).all()
    g.add_vertices(known, np.zeros((len(known), 3)))
    wb = g.wire_bytes()
    keep = np.setdiff1d(np.arange(CAP), HOLES)
    other, other3 = recE[::-1].copy(), rec3[::-1].copy()   # what is addressed to robots 0 and 2: ids robot 1 knows, other numbers
    ask = np.array([3, 5], dtype=np.int32)                 # closure requests for vertices robot 1 does not have: no effect

    def ingest(buffers):
        buf = np.concatenate(buffers)
        assert len(buf) == R * wb
        t = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        n = g.ingest(t.data_ptr())
        ctx.synchronize()
        return list(n)

    mine = _wire_buffer(ME, {0: (other, ask), ME: (recE, ask), 2: (other, ask)})      # my own buffer comes back too: ignored
    # round 1: a full slice with two holes from robot 0, a single edge from robot 2
    n = ingest([_wire_buffer(0, {0: (other, ask), ME: (rec130, ask), 2: (other, ask)}), mine,
                _wire_buffer(2, {0: (other3, ask), ME: (rec1, ask), 2: (other3, ask)})])
    assert n == [CAP - len(HOLES), 0, 1]
    want = {0: _expect(dec130, keep), 2: _expect(dec1)}
    _check_sets(g, want)
    # round 2: nothing from robot 0 (its set is kept: gathered from the staging), 129 edges from robot 2 (fresh)
    n = ingest([_wire_buffer(0, {0: (other, ask), ME: (rec130[:0], ask), 2: (other, ask)}), mine,
                _wire_buffer(2, {0: (other3, ask), ME: (recE[:129], ask), 2: (other3, ask)})])
    assert n == [0, 0, 129]
    want[2] = _expect(decE, np.arange(129))
    _check_sets(g, want)
    # round 3: one message from robot 2 through the one-peer path (host widening, upload, k_gather_edges)
    _, ref3, _ = RC.fixture_case(fx, "condensed3")
    assert g.message_from(from_bytes(ref3)) == 3
    want[2] = _expect(dec3)
    _check_sets(g, want)
    # round 4: robot 0 sends a full slice of edges robot 1 cannot place -- the widened wire data of its slots is overwritten,
    # its set is still the one of round 1 -- and robot 2 sends nothing: both sets come from the staging
    strangers = recE.copy()
    strangers[:, :8].view("<i4")[:] += 50000
    n = ingest([_wire_buffer(0, {0: (other, ask), ME: (strangers, ask), 2: (other, ask)}), mine,
                _wire_buffer(2, {0: (other3, ask), ME: (rec1[:0], ask), 2: (other3, ask)})])
    assert n == [0, 0, 0]
    _check_sets(g, want)
    assert g.skipped_messages() == 0 and len(g.closures(0, "out")) == 0 and len(g.closures(2, "out")) == 0
    g.close()


@pytest.mark.timeout(120)
def test_ingests_and_one_peer_messages_in_sequence_on_the_device(ctx):
    """The four steps of tests/message_sequence.py on a device graph -- a round buffer through k_wire_read and
    k_accept_gather_edges, two one-peer messages through the host widening and k_gather_edges (one accepted, one that keeps the
    set), a round buffer again: the host mirror of the staging goes stale, fresh, fresh, stale, and both users of the slot list
    run.  After every step the staging (received_edges) and the solver's compact segment hold, bit for bit, what the restatement
    holds -- which test_condensed_cpu.py shows a host-only graph of this library to hold as well."""
    import torch
    import message_sequence as MS
    from ref_condensed import RefRobotGraph
    g, ref = RobotGraph(ctx, MS.ME, MS.R, cap_edges=MS.CAP), RefRobotGraph(None, MS.ME, MS.R, cap_edges=MS.CAP)
    MS.fill(g); MS.fill(ref)
    for kind, what, accepted in MS.steps():
        if kind == "round":
            t = torch.from_numpy(what).cuda()
            torch.cuda.synchronize()
            assert list(g.ingest(t.data_ptr())) == list(ref.ingest_host(what)) == accepted
        else:
            assert g.message_from(what) == ref.buf.ingest_from(what.robotId, what.edges, what.closures) == accepted
        ctx.synchronize()
        want = MS.state(ref)
        MS.assert_same_state(MS.state(g), want)
        m, i = g.debug_received_segment()
        assert np.array_equal(_bits(m), _bits(np.concatenate([want[0][p][2] for p in range(MS.R)])))
        assert np.array_equal(_bits(i), _bits(np.concatenate([want[0][p][3] for p in range(MS.R)])))
        assert g.counts() == ref.counts() and g.skipped_messages() == 0
    g.close()


def _index_map(to_ids, seed):
    """A shuffled id table and, per edge, the index of its far end in it: a permutation, nowhere the identity by luck alone."""
    ids = np.random.default_rng(seed).permutation(np.unique(to_ids)).astype(np.int32)
    where = {int(v): k for k, v in enumerate(ids)}
    return ids, np.array([where[int(v)] for v in to_ids], dtype=np.int32)


@pytest.mark.parametrize("n", [1, 127, 128, 129, 130])
def test_write_side_equals_the_reference_encoder(ctx, fx, n):
    rec, recs, _ = _case(fx, "edge130")
    ft, en = rec["from_to"][:n], rec["edge_numbers"][:n]
    ids, to_vertex = _index_map(ft[:, 1], 5)
    assert len(ids) == n and (n == 1 or not np.array_equal(to_vertex, np.arange(n)))
    out = wire_narrow_edges(ctx, ft[0, 0], to_vertex, ids, en[:, :3], en[:, 3:])
    assert out.dtype == WIRE_EDGE_DTYPE and out.tobytes() == recs[:n].tobytes()


def test_batched_write_side_equals_the_reference_encoder(ctx, fx):
    """Four jobs in one launch.  Job j reads its vertex indices by j, everything else by its output slot; slots, strides and
    counts are chosen so that any mix-up of the two, a count taken from the wrong job or a store past ``nq`` shows."""
    cases = [_case(fx, "condensed130"), None, _case(fx, "condensed1"), _case(fx, "edge130")]
    nq = np.array([130, 0, 1, 129], dtype=np.int32)
    out_slot = np.array([3, 2, 0, 1], dtype=np.int32)
    assert not (out_slot == np.arange(4)).any() and sorted(out_slot) == [0, 1, 2, 3]
    gauge = np.array([c[0]["from_to"][0, 0] if c else 999 for c in cases], dtype=np.int32)
    assert len(set(gauge.tolist())) == 4
    ms, es, fs, ws = 4 * 130 + 24, 24 * 130 + 40, 48 * 130 + 64, 44 * 130 + 52        # strides beyond the payload
    ids, _ = _index_map(np.concatenate([c[0]["from_to"][:, 1] for c in cases if c]), 9)
    where = {int(v): k for k, v in enumerate(ids)}
    tv = np.full(4 * ms, 0xEE, dtype=np.uint8)
    est, info = np.full(4 * es, 0xEE, dtype=np.uint8), np.full(4 * fs, 0xEE, dtype=np.uint8)
    sentinel = 0xA5
    wire = np.full(4 * ws, sentinel, dtype=np.uint8)
    for j, c in enumerate(cases):
        q, s = int(nq[j]), int(out_slot[j])
        if not q:
            continue
        rec = c[0]
        idx = np.array([where[int(v)] for v in rec["from_to"][:q, 1]], dtype=np.int32)
        tv[j * ms:j * ms + 4 * q] = idx.view(np.uint8)
        est[s * es:s * es + 24 * q] = np.ascontiguousarray(rec["edge_numbers"][:q, :3]).view(np.uint8).reshape(-1)
        info[s * fs:s * fs + 48 * q] = np.ascontiguousarray(rec["edge_numbers"][:q, 3:]).view(np.uint8).reshape(-1)
    out = wire_narrow_edges_batched(ctx, nq, gauge, out_slot, (ms, es, fs, ws), tv, ids, est, info, wire)
    assert (wire == sentinel).all() and out.shape == wire.shape
    for j, c in enumerate(cases):
        q, s = int(nq[j]), int(out_slot[j])
        slot = out[s * ws:(s + 1) * ws]
        if q:
            assert slot[:44 * q].tobytes() == c[1][:q].tobytes(), j
        assert (slot[44 * q:] == sentinel).all(), j          # records beyond nq and the gap keep the sentinel
