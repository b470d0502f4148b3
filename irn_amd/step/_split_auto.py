"""`--split_gemm auto` in the steps (net/resnet50.SPLIT_AUTO): which images left fp16's range inside the split-precision GEMMs,
decided per image from the per-sample device flags (`ops.split_sample_flags`), and what a worker keeps about them until it
computes them again on the fp32 GEMMs.  An image's files depend on that image alone: flagged, they are those of a
`--split_gemm 0` run; otherwise those of a `--split_gemm 1` run.  Nothing here waits for the device on the thread that drives it:
the flag words travel to page-locked memory on the stream of the results they belong to and are looked at behind the event
the reader of those results waits for anyway."""
import contextlib
import threading

import numpy as np
import torch

from . import _io, _report


def enabled():
    """Is the per-image fallback on in this process (IRN_SPLIT_GEMM=auto, split GEMMs not switched off meanwhile)?"""
    from ..net import resnet50 as _r50
    return bool(_r50.SPLIT_AUTO and _r50.SPLIT_GEMM)


def recording(flags):
    """`ops.split_sample_flags(flags)`, or a block that changes nothing (and needs no library) without `flags`."""
    if flags is None:
        return contextlib.nullcontext()
    from .. import ops
    return ops.split_sample_flags(flags)


def redo_names(flags, names):
    """flags: integer array [n_scales, 2 * len(names)] (or [2 * len(names)]) — one word per trunk pass and network-input row,
    rows as [image, flip, image, flip, ...] — -> the names whose image or flip has a non-zero word in any pass, in order."""
    f = np.asarray(flags)
    if f.ndim == 1:
        f = f[None]
    if f.ndim != 2 or f.shape[1] != 2 * len(names):
        raise ValueError("redo_names: flag words of shape %s for %d images (two rows each per pass)" % (f.shape, len(names)))
    bad = (f != 0).any(axis=0).reshape(len(names), 2).any(axis=1)
    return [n for n, b in zip(names, bad) if b]


class FlagRead:
    """The flag words of one batch on their way to the host: `flags_dev` int32 [n_scales, 2 n_images] (or [2 n_images]) is
    copied into a page-locked buffer on the CURRENT stream — enqueue the results' own copies and their event behind it.
    `names()` is for whoever has waited for such an event (or passes `wait=True` to wait for this copy's own); the buffer goes
    back to the pool after `users` calls of `release()` (one per writer job that looks at it)."""

    def __init__(self, flags_dev, names, users=1):
        self.image_names = list(names)
        self._shape = tuple(flags_dev.shape)
        self._n = flags_dev.numel()
        self._buf = _io.PINNED.take(4 * self._n)
        self._buf[:4 * self._n].view(torch.int32).copy_(flags_dev.reshape(-1), non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()
        self._users = users
        self._lock = threading.Lock()

    def words(self):
        return self._buf[:4 * self._n].view(torch.int32).numpy().reshape(self._shape)

    def names(self, wait=False):
        if wait:
            self._event.synchronize()
        return redo_names(self.words(), self.image_names)

    def flagged(self, index, wait=False):
        """Did image `index` of the batch (rows 2 index, 2 index + 1) leave the range in any pass?"""
        if wait:
            self._event.synchronize()
        return bool((self.words()[..., 2 * index:2 * index + 2] != 0).any())

    def release(self):
        with self._lock:
            self._users -= 1
            last = self._users == 0
        if last and self._buf is not None:
            self._event.synchronize()          # (a buffer nobody looked at: the copy into it must have landed before it is reused)
            buf, self._buf = self._buf, None
            _io.PINNED.give(buf)


class Redo:
    """A worker's redo list of one step: image name -> what the step needs to compute it again (appended by writer threads
    and by the main thread; read by the main thread once the writer has drained)."""

    def __init__(self):
        self._items = {}
        self._lock = threading.Lock()

    def add(self, name, info=None):
        with self._lock:
            self._items.setdefault(name, info)

    def __len__(self):
        return len(self._items)

    def items(self):
        with self._lock:
            return list(self._items.items())

    def report(self, rank):
        """End of the step's redo: the count goes to the worker's counters, one line names the images (none: no line)."""
        names = [n for n, _ in self.items()]
        _report.SPLIT_STATS["fallback_images"] += len(names)
        line = _report.split_fallback_line(names)
        if line:
            _report.say("[worker %d] %s" % (int(rank), line))
