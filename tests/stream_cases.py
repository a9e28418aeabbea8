"""Contexts on a stream the caller owns, and inputs that arrive late on that stream (tests/test_caller_stream_gpu.py).
TEST INFRASTRUCTURE ONLY.

``late`` queues, on the caller's stream: a decoy into the input buffers (a valid input whose correct answer differs), a
device-side delay, the real input, an event.  A library call made while the event is still pending sees the real input only
if everything it does with the buffers is ordered behind the work already queued on the context's stream."""
import contextlib
import time

TARGET_MS = 100.0
_DELAY = {}
MARGINS_MS = []          # per checked call: how long the inputs were still to be pending when the call was made (estimated)


def delay_cycles():
    """The argument of torch.cuda._sleep for about TARGET_MS on this device, timed once per process with events."""
    import torch
    if "cycles" not in _DELAY:
        s = torch.cuda.Stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        probe = 20_000_000
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)                       # (the kernel's first launch loads its code)
            a.record()
            torch.cuda._sleep(probe)
            b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.1, ("the delay kernel cannot be timed", ms)
        _DELAY.update(cycles=int(probe * TARGET_MS / ms), probe_ms=ms)
        print(f"stream_cases: torch.cuda._sleep({probe}) took {ms:.2f} ms; {_DELAY['cycles']} cycles for {TARGET_MS:.0f} ms")
    return _DELAY["cycles"]


@contextlib.contextmanager
def caller_context():
    """(Context(0, stream=s.cuda_stream), s) for a fresh torch.cuda.Stream(); the context is closed afterwards."""
    import torch
    from cg_mrslam_amd import Context
    s = torch.cuda.Stream()
    c = Context(0, stream=s.cuda_stream)
    try:
        yield c, s
    finally:
        c.close()


class Late:
    """What ``late`` queued: ``pending()`` is the condition that keeps a test from passing vacuously."""

    def __init__(self, start, done, t_host):
        self.start, self.done, self.t_host, self.t_query = start, done, t_host, None

    def query(self):
        return self.done.query()

    def pending(self):
        """Call immediately before the library call: the inputs must not have arrived yet."""
        self.t_query = time.perf_counter()
        assert not self.done.query(), "the delayed inputs arrived before the call: the delay is too short to check anything"

    def margin_ms(self):
        """After the results were read: the delay as the device ran it minus the host time between queueing it and the
        call (the stream was idle when it was queued).  Recorded in MARGINS_MS."""
        self.done.synchronize()
        m = self.start.elapsed_time(self.done) - 1e3 * (self.t_query - self.t_host)
        MARGINS_MS.append(m)
        return m


def late(s, dst, src, decoy):
    """Under torch.cuda.stream(s): fill ``dst`` with ``decoy``, queue the delay, queue dst.copy_(src), record an event.
    ``dst`` / ``src`` / ``decoy``: device tensors, or equally long lists of them (one delay for all).  Returns a Late."""
    import torch
    if isinstance(dst, torch.Tensor):
        dst, src, decoy = [dst], [src], [decoy]
    assert len(dst) == len(src) == len(decoy)
    cycles = delay_cycles()
    start, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        for d, x in zip(dst, decoy):
            assert d.shape == x.shape and d.dtype == x.dtype
            d.copy_(x)
        t_host = time.perf_counter()
        start.record()
        torch.cuda._sleep(cycles)
        for d, x in zip(dst, src):
            assert d.shape == x.shape and d.dtype == x.dtype
            d.copy_(x)
        done.record()
    return Late(start, done, t_host)


def read(s, *tensors):
    """Stream-ordered copies to the host under torch.cuda.stream(s) (each waits for the stream, and for nothing else)."""
    import torch
    with torch.cuda.stream(s):
        out = [t.cpu().numpy() for t in tensors]
    return out[0] if len(out) == 1 else out
