"""`ops.mask_polygons` with the GPU lagging behind the host (tests/_lag.py, as tests/test_gpu_lag.py uses it): the call reads
three small results back, so it waits for the device; what it returns behind a stall must be what it returns on an idle
device.  The masks are a poison-filled buffer that a copy enqueued behind the stall overwrites: work put ahead of the stall,
or on another stream, would trace the poison (a full mask)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lag as L  # noqa: E402
import _polygon_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu


def test_mask_polygons_behind_a_stall():
    from irn_amd import ops
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(21)
    masks = rng.rand(3, 40, 67) < 0.55
    masks[1, 10:30, 10:50] = True
    masks[1, 15:25, 20:40] = False                         # a hole
    small = rng.rand(2, 9, 13) < 0.5
    real = [torch.from_numpy(m.astype(np.uint8)).to(dev) for m in (masks, small)]
    want = [P.mask_polygons(masks), P.mask_polygons(small)]
    host_ms = 0.0
    for _ in range(2):                                      # idle, twice: the first pass fills the caches
        idle, host_ms = [], 0.0
        for t in real:
            torch.cuda.synchronize()
            out, ms = L.timed(lambda: ops.mask_polygons(t))
            torch.cuda.synchronize()
            idle.append(out)
            host_ms += ms
    bufs = [torch.full_like(t, 255) for t in real]
    torch.cuda.synchronize()
    with L.Behind(L.stall_ms_for(host_ms)) as b:
        for buf, t in zip(bufs, real):
            buf.copy_(t)
        got = [b.call("mask_polygons %d" % i, lambda buf=buf: ops.mask_polygons(buf)) for i, buf in enumerate(bufs)]
    torch.cuda.synchronize()
    b.report("mask_polygons")
    lag = b.lags["mask_polygons 0"]
    assert lag.before and not lag.after                     # entered while the device lagged; it reads counts back, so it waited
    for g, i, w in zip(got, idle, want):
        for a, c, d in zip(g, i, w):
            assert a.dtype == c.dtype == d.dtype and np.array_equal(a, c) and np.array_equal(a, d)
