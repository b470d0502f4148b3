"""How a shard's bytes reach the device and leave it without stalling the thread that drives the GPU: loader threads
(`make_loader`), page-locked staging buffers (`PINNED`), uploads on the copy stream (`upload`), writer threads (`AsyncWriter`)
and the scaffolding every shard worker sets these up with (`shard_io`)."""
import collections
import contextlib
import threading
from concurrent.futures import ThreadPoolExecutor

import torch
from torch.utils.data import default_collate


def device_preprocess(args):
    """Steps build the multi-scale inputs on the GPU unless args.device_preprocess is set to False."""
    return bool(getattr(args, "device_preprocess", True))


class PinnedPool:
    """Page-locked staging buffers for device-to-host copies that must not stall the step: `take(nbytes)` hands out a
    uint8 buffer (recycled, rounded up to 1 MiB), `give(buf)` returns it.  Thread-safe (writer threads give back)."""

    def __init__(self):
        self._free = {}
        self._lock = threading.Lock()

    def take(self, nbytes):
        size = max(1 << 20, (int(nbytes) + (1 << 20) - 1) >> 20 << 20)
        with self._lock:
            bucket = self._free.get(size)
            if bucket:
                return bucket.pop()
        return torch.empty(size, dtype=torch.uint8, pin_memory=True)

    def give(self, buf):
        with self._lock:
            self._free.setdefault(buf.numel(), []).append(buf)


PINNED = PinnedPool()
_UPLOADS = []            # (event, page-locked staging buffer) of uploads still in flight


def upload(t, staging=None):
    """Host tensor -> device tensor WITHOUT stalling the host.  `t.cuda()` of pageable memory returns only when the stream has
    drained — in a step's loop that is "when the previous batch's trunk passes have finished", so the host could never
    enqueue the next batch under them and the GPU idled 10 % of make_cam (7.5 ms of host time per image inside `.cuda()`,
    `tools/make_cam_profile.py`, round 4).  Here the bytes go through a recycled page-locked buffer and cross on the copy
    stream; the current stream waits for the copy on the DEVICE (an event), the host moves on."""
    from .. import _host
    dev = torch.device("cuda", torch.cuda.current_device())
    src = t.contiguous()
    nbytes = src.numel() * src.element_size()
    while _UPLOADS and _UPLOADS[0][0].query():          # buffers whose copy has landed go back to the pool
        PINNED.give(_UPLOADS.pop(0)[1])
    if nbytes == 0:
        return src.cuda()
    if staging is None:
        staging = PINNED.take(nbytes)
        staging[:nbytes].copy_(src.view(-1).view(torch.uint8) if src.dtype != torch.uint8 else src.view(-1))
    # (else: `t` already lives in the page-locked buffer `staging` — a loader thread put it there, make_loader)
    cs = _host.copy_stream(dev)
    with torch.cuda.stream(cs):
        out = staging[:nbytes].to(dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record(cs)
    cur = torch.cuda.current_stream(dev)
    cur.wait_event(done)
    out.record_stream(cur)                               # allocated on the copy stream, consumed on this one
    _UPLOADS.append((done, staging))
    return out.view(src.dtype).view(src.shape)


def device_images(pack, scales, normal=None):
    """Loader item -> list over scales of GPU fp32 [2,3,Hs,Ws] (image + horizontal flip).  Raw uint8 items
    (dataset raw=True) go through irn_msf_pack; items already in the reference's format are copied as is."""
    img = pack["img"]
    if torch.is_tensor(img) and img.dtype == torch.uint8 and img.numel() == 0:
        return None                                  # the dataset skipped the pixels (VOC12ClassificationDatasetMSF skip_image)
    if torch.is_tensor(img) and img.dtype == torch.uint8:
        from .. import ops
        kw = {} if normal is None else {"mean": normal.mean, "std": normal.std}
        return ops.msf_pack(upload(img[0], pack.pop("_staging", None)), scales, **kw)
    imgs = img if isinstance(img, (list, tuple)) else [img]
    return [upload(i[0]) for i in imgs]


def set_skip_image(databin, predicate):
    """Hand the step's `skip_image` predicate to the dataset behind a shard (a `Subset` of VOC12ClassificationDatasetMSF)."""
    ds = getattr(databin, "dataset", databin)
    if hasattr(ds, "skip_image"):
        ds.skip_image = predicate


def make_loader(databin, num_workers, prefetch=4):
    """Items of `databin` in order, each collated like `DataLoader(databin, batch_size=1, shuffle=False)` collates it
    (what the reference's steps iterate over, step/make_cam.py:22).  The reference's loader workers are processes; here
    they are THREADS: the work of an item is JPEG decoding (and, with device_preprocess off, PIL resizes), which runs
    inside Pillow with the GIL released, while forking worker processes from a process that holds a HIP context costs
    2-3 s per loader on the GPU box (the parent's address space is large) — more than a 1 000-image shard takes."""
    n = len(databin)
    num_workers = min(int(num_workers), MAX_LOADER_THREADS)     # threads, not processes: more of them only fight over the GIL
    if num_workers <= 0:
        for i in range(n):
            yield default_collate([databin[i]])
        return
    pool = ThreadPoolExecutor(max_workers=num_workers)
    pending = collections.deque()
    pin = torch.cuda.is_available()

    def load(i):
        pack = default_collate([databin[i]])
        img = pack.get("img") if isinstance(pack, dict) else None
        if pin and torch.is_tensor(img) and img.dtype == torch.uint8 and img.numel():
            # the decoded image goes into page-locked memory HERE, in the loader thread: `upload` then only issues the
            # asynchronous copy (the 0.8 MB memcpy cost the step's main thread 0.4 ms per image, round 5)
            nbytes = img.numel()
            buf = PINNED.take(nbytes)
            buf[:nbytes].copy_(img.reshape(-1))
            pack["img"] = buf[:nbytes].view(img.shape)
            pack["_staging"] = buf
        return pack

    try:
        nxt = 0
        depth = num_workers * prefetch
        while nxt < n or pending:
            while nxt < n and len(pending) < depth:
                pending.append(pool.submit(load, nxt))
                nxt += 1
            yield pending.popleft().result()
    finally:
        # an early close (an exception in the consumer, a generator dropped half-way) must not strand the page-locked buffers
        # of items nobody will consume: cancel what has not started, wait for what has, hand every buffer back
        pool.shutdown(wait=True, cancel_futures=True)
        for fut in pending:
            try:
                if not fut.cancelled():
                    buf = fut.result().pop("_staging", None)
                    if buf is not None:
                        PINNED.give(buf)
            except Exception:
                pass


def progress(process_id, n_workers, it, n_items):
    """The reference prints 5 % ticks from the last rank and divides by len//20 (ZeroDivision for
    shards under 20 images, step/make_cam.py:58); guarded here."""
    step = max(n_items // 20, 1)
    if process_id == n_workers - 1 and it % step == 0:
        print("%d " % ((5 * it + 1) // step), end="", flush=True)


def writer_threads(args, n_workers):
    """Encoder / writer threads of a worker.  Measured on the `steps` leg (128 images, `tools/steps_threads_probe.py`, round 3
    session 13): 4 loader + 4 writer threads 69.4 images/s, 8 + 8 69.0, 16 + 16 64.4, 32 + 16 56.5 — beyond a handful the
    threads only contend for the interpreter lock with the thread that drives the GPU."""
    return 4


MAX_LOADER_THREADS = 8      # same measurement: `--num_workers` defaults to half the host's cores (reference run_sample.py:11)


class AsyncWriter:
    """Output files (4 MB CAM dictionaries, PNG label maps, detection dictionaries) are encoded and
    written by a small thread pool while the GPU works on the next images; at
    most `max_pending` writes are in flight, errors surface at the next submit or at close()."""

    def __init__(self, threads=4, max_pending=32):
        self._pool = ThreadPoolExecutor(max_workers=threads)
        self._pending = []
        self._max = max_pending

    def _reap(self, keep):
        while len(self._pending) > keep:
            self._pending.pop(0).result()        # re-raises a failed write

    def submit(self, fn, *args, **kw):
        self._reap(self._max - 1)
        self._pending.append(self._pool.submit(fn, *args, **kw))

    def drain(self):
        """Wait for every write submitted so far (re-raises a failed one); the writer stays open."""
        self._reap(0)

    def close(self):
        try:
            self._reap(0)
        finally:
            self._pool.shutdown(wait=True)


@contextlib.contextmanager
def shard_io(process_id, dataset, args):
    """Shard `process_id` of `dataset` with its loader and writer threads: -> (databin, number of workers, loader, writer).  The
    host's `--num_workers` loader threads are shared out among the workers; the writer is closed however the block ends."""
    databin, n = dataset[process_id], len(dataset)
    loader = make_loader(databin, int(args.num_workers) // n)
    writer = AsyncWriter(threads=writer_threads(args, n))
    try:
        yield databin, n, loader, writer
    finally:
        writer.close()
