"""Make the device lag behind the host, the way it does in the steps: a bounded busy kernel (`torch.cuda._sleep`) is put on
the current stream, and the calls under test are made while it still runs.  Test infrastructure of tests/test_gpu_lag.py;
importing it touches no GPU.

    stall(ms)            enqueue a busy kernel of about `ms` on the current stream -> the event recorded right behind it
    lagging(ev)          the device has not reached `ev` yet
    Behind(ms)           context manager: `call(name, thunk)` runs a thunk behind the stall and records whether the device was
                         still lagging just before the call and just after it returned, and the host time it took
    run_behind(...)      the same for a list of thunks

Nothing here can wait for ever: the kernel spins for a fixed number of clock cycles, calibrated once per process with two
events, and a stall is at most STALL_MAX_MS long."""
import collections
import time

import torch

STALL_MIN_MS = 100.0
STALL_MAX_MS = 1000.0
HOST_FACTOR = 10.0         # the stall covers ten times the host time of the warm sequence: jitter of a shared host

_cycles_per_ms = None

Lag = collections.namedtuple("Lag", "name before after host_ms")


def cycles_per_ms():
    """Cycles of `torch.cuda._sleep` per millisecond on the current device, measured once per process."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda._sleep(100000)                           # the first launch loads the kernel
        torch.cuda.synchronize()
        cycles, ms = 2000000, 0.0
        for _ in range(8):                                  # grow until the timed kernel is long against the events' noise
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 20.0:
                break
            cycles *= 4
        if not ms > 0.5:
            raise RuntimeError("torch.cuda._sleep(%d) took %.3f ms: it cannot be calibrated on this device" % (cycles, ms))
        _cycles_per_ms = cycles / ms
        print("lag: torch.cuda._sleep runs %.0f cycles per ms (%d cycles took %.2f ms)" % (_cycles_per_ms, cycles, ms))
    return _cycles_per_ms


def stall(ms):
    """Enqueue about `ms` (at most STALL_MAX_MS) of busy kernel on the current stream; -> the event recorded behind it."""
    ms = min(float(ms), STALL_MAX_MS)
    torch.cuda._sleep(max(1, int(ms * cycles_per_ms())))
    ev = torch.cuda.Event()
    ev.record()
    return ev


def lagging(ev):
    return not ev.query()


def stall_ms_for(host_ms):
    """The stall of a sequence whose warm, un-stalled run took `host_ms` of host time."""
    return min(STALL_MAX_MS, max(STALL_MIN_MS, HOST_FACTOR * host_ms))


def timed(thunk):
    """-> (thunk's result, host milliseconds the call took)."""
    t0 = time.perf_counter()
    out = thunk()
    return out, (time.perf_counter() - t0) * 1e3


class Behind:
    """`with Behind(ms) as b:` enqueues the stall on the current stream; `b.call(name, thunk)` runs a thunk behind it,
    `b.gap(ms)` enqueues a short stall that keeps later work queued, `b.restall(ms)` starts a new long stall that the
    following calls are measured against.  `b.lags` maps a call's name to its Lag record (insertion-ordered)."""

    def __init__(self, ms):
        self.ms = ms
        self.event = None
        self.lags = collections.OrderedDict()

    def __enter__(self):
        self.event = stall(self.ms)
        return self

    def __exit__(self, *exc):
        return False

    def restall(self, ms=None):
        self.event = stall(self.ms if ms is None else ms)

    def gap(self, ms):
        stall(ms)

    def call(self, name, thunk):
        before = lagging(self.event)
        out, host_ms = timed(thunk)
        self.lags[name] = Lag(name, before, lagging(self.event), host_ms)
        return out

    def report(self, what):
        print("lag: %s behind a stall of %.0f ms" % (what, self.ms))
        for lag in self.lags.values():
            print("lag:   %-28s entered %s, returned %s, host %.3f ms" % (
                lag.name, "lagging" if lag.before else "idle", "lagging" if lag.after else "after the stall", lag.host_ms))


def run_behind(thunks, ms, gap_ms=0.0):
    """Run `thunks` (a list of (name, thunk)) behind one stall of `ms`, a short stall of `gap_ms` after each.
    -> (results, the Behind with its records)."""
    out = []
    with Behind(ms) as b:
        for name, thunk in thunks:
            out.append(b.call(name, thunk))
            if gap_ms:
                b.gap(gap_ms)
    return out, b
