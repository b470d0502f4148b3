"""What the host modules of more than one kernel file need: grow-only buffers, the copy stream and the read-back behind
it, the byte layout of a packed device-to-host transfer and its device staging buffer, and three argument checks."""
import torch

from ._lib import _need_cuda

_CACHE = {}            # (tag, device or "pinned") -> grow-only buffer
_COPY_STREAMS = {}     # (device type, index) -> the stream the deferred read-backs run on


def cached(tag, dev, nbytes, dtype):
    """Grow-only scratch buffers (device) / pinned staging (dev == "pinned"), one per tag and device."""
    key = (tag, str(dev))
    buf = _CACHE.get(key)
    if buf is None or buf.numel() < nbytes:
        n = int(nbytes * 1.25) + 256
        buf = torch.empty(n, dtype=dtype, pin_memory=True) if dev == "pinned" else torch.empty(n, dtype=dtype, device=dev)
        _CACHE[key] = buf
    return buf


def copy_stream(dev):
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _COPY_STREAMS:
        _COPY_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _COPY_STREAMS[key]


def read_back(src, host, side):
    """Start the copy of the device bytes `src` into the head of the page-locked buffer `host` and return the event that
    marks its end.  The copy runs on the current stream or, with `side`, on the device's copy stream behind everything
    enqueued so far: it then crosses PCIe under the kernels the caller enqueues next, and the allocator hands `src`'s block
    out again only behind it."""
    done = torch.cuda.Event()
    stream = torch.cuda.current_stream(src.device)
    if side:
        ready = torch.cuda.Event()
        ready.record(stream)
        stream = copy_stream(src.device)
        stream.wait_event(ready)
        src.record_stream(stream)
    with torch.cuda.stream(stream):
        host[:src.numel()].copy_(src, non_blocking=True)
        done.record(stream)
    return done


class PackedLayout:
    """Where the fields of one packed transfer lie.  `fields` lists them in order as (name, np.dtype, element count,
    alignment): each starts at the next multiple of its alignment behind the one before it.  `offsets` maps a field's name
    to its byte offset, `nbytes` is the end of the last one (a closing field of no elements pads the total to its
    alignment).  The pointers a C entry is handed and the numpy views the host takes of the copy both come from here, as
    lists in the order of the fields (a detection batch has hundreds of them: no look-up by name on that path)."""

    def __init__(self, fields):
        self._fields, self._spans, at = fields, [], 0
        for _, dtype, count, align in fields:
            at += -at % align
            end = at + dtype.itemsize * count
            self._spans.append((at, end, dtype))
            at = end
        self.nbytes = at

    @property
    def offsets(self):
        return {field[0]: span[0] for field, span in zip(self._fields, self._spans)}

    def ptrs(self, base):
        """Every field's address in a buffer that starts at `base`; None for a field without elements."""
        return [base + at if end > at else None for at, end, _ in self._spans]

    def views(self, raw):
        """Every field of the host copy `raw` (numpy uint8, the layout's bytes from its start on) as an array of its dtype."""
        return [raw[at:end].view(dtype) for at, end, dtype in self._spans]


def staging(tag, dev, nbytes, align, own):
    """The device buffer a packed result is written into before its read-back: `nbytes` bytes as a uint8 view that starts
    on a multiple of `align`.  With `own` it is a buffer of the call's own, for a transfer that is left in flight (the next
    batch must not write into it); otherwise the cached one of `tag`, for a transfer the call waits for."""
    n = nbytes + (align if align > 1 else 0)
    buf = torch.empty(n, dtype=torch.uint8, device=dev) if own else cached(tag, dev, n, torch.uint8)
    shift = -buf.data_ptr() % align
    return buf[shift:shift + nbytes]


def accumulator(t, shape, dev, what):
    if t is None:
        return torch.zeros(shape, dtype=torch.int64, device=dev)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
            and tuple(t.shape) == tuple(shape) and t.device == dev):
        raise ValueError("%s must be a contiguous int64 GPU tensor of shape %s on %s" % (what, tuple(shape), dev))
    return t


def u8_map(t, dev, what):
    if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.dtype in (torch.uint8, torch.bool)):
        raise ValueError("%s must be a uint8 [H,W] tensor" % what)
    return t.to(dev).view(torch.uint8).contiguous() if t.dtype == torch.bool else t.to(dev).contiguous()


def need_f32_contig(t, what, min_dim):
    _need_cuda(t, what)
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < min_dim:
        raise ValueError("%s must be a contiguous fp32 tensor of >= %d dimensions, got %s %s" % (what, min_dim, t.dtype, tuple(t.shape)))
