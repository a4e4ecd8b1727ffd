"""Bounded gates on a stream, for the stream-ordering probes of tests/test_gpu_stream_order.py (no test functions here).

A gate is ``torch.cuda._sleep``: a kernel that spins for a given number of clock ticks and ends BY ITSELF -- never one that
waits for a host-written flag or for another stream.  While it runs, whatever is queued behind it on its stream has not
happened yet, and whatever another stream does happens first: that turns "which stream was this enqueued on" into a
deterministic difference in the values read.

  blocker(stream)        queue a gate of about GATE_MS on ``stream``; returns the event recorded behind it
  gate_held(event)       is the gate still running?  Taken right after the call under test returns on the host: a call that is
                         asynchronous and waits for no other stream returns long before the gate ends
  poisoned_block(nbytes) a NaN-filled block of that size, freed at once: the next ``torch.empty`` of that size on the same
                         stream gets poison instead of stale, plausible values -- and, queued behind a gate, gets it LATE
  NOTES                  (what, milliseconds) pairs the probes record: gate lengths and the host time of every probed call
"""
import time

GATE_MS = 100.0
_CAL_TICKS = 20_000_000
_ticks_per_ms = None
NOTES = []


def calibrate(torch):
    """ticks of ``torch.cuda._sleep`` per millisecond, timed once with events on the idle device (the second of two runs: the
    first pays for loading the kernel)"""
    global _ticks_per_ms
    if _ticks_per_ms is None:
        torch.cuda.synchronize()
        ms = 0.0
        for _ in range(2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(_CAL_TICKS)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
        assert ms > 0.0, "the sleep kernel took no time: no gate can be built from it"
        _ticks_per_ms = _CAL_TICKS / ms
        NOTES.append(("calibration: %d ticks" % _CAL_TICKS, ms))
    return _ticks_per_ms


def blocker(stream, ms=GATE_MS):
    """Queue a gate of about ``ms`` milliseconds on ``stream``; the event recorded behind it.  ``event.started`` is an event
    recorded ahead of the gate, so that ``gate_ms`` can report its length afterwards."""
    import torch
    ticks = int(calibrate(torch) * ms)
    with torch.cuda.stream(stream):
        start = torch.cuda.Event(enable_timing=True)
        done = torch.cuda.Event(enable_timing=True)
        start.record()
        torch.cuda._sleep(ticks)
        done.record()
    done.started = start
    return done


def gate_held(event):
    return not event.query()


def gate_ms(event):
    """the event-timed length of a finished gate"""
    event.synchronize()
    return event.started.elapsed_time(event)


def poisoned_block(nbytes, stream=None):
    """Allocate ``nbytes`` filled with NaN (the fill is queued on torch's current stream, or ``stream``), then free them."""
    import torch
    if nbytes <= 0:
        return
    with torch.cuda.stream(stream):
        t = torch.empty((int(nbytes) + 7) // 8, dtype=torch.float64, device="cuda")
        t.fill_(float("nan"))
        del t


class timed:
    """``with timed(what):`` -- the host time of the block goes into NOTES"""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        self.ms = (time.perf_counter() - self.t0) * 1e3
        NOTES.append((self.what, self.ms))
        return False
