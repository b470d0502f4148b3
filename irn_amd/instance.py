"""Host side of irn_amd/csrc/instance.hip: the instance front end (centroid refinement, clustering, 4-connected labelling)
and the detections of a class map — dense masks, COCO run lengths, or overlap counts against ground truth — one image
at a time or a batch with its last transfer left in flight.  `irn_amd.ops` re-exports the functions.  GPU tensors in;
GPU tensors or the reference's numpy records out; no CPU fallback."""
import collections
import ctypes as C
import time

import numpy as np
import torch

from ._host import PackedLayout, accumulator, cached, read_back, staging, u8_map
from ._lib import _need_cuda, _stream, check, i32_array, lib, ptr_array


def find_centroids_with_refinement(displacement, iterations=300):
    """dp GPU fp32 [2,h,w] -> GPU int32 [2,h,w] (cy, cx); bit-identical to the reference's numpy
    (step/make_ins_seg_labels.py:18-56).  A batch of one."""
    return find_centroids_batch([displacement], iterations)[0]


def cluster_centroids(centroids, displacement, thres=2.5, as_one_hot=False):
    """-> (cluster_map GPU int32 [h,w] with values 0..K-1, K).  With ``as_one_hot`` returns the
    reference's bool [K,h,w] instead (step/make_ins_seg_labels.py:58-75).  A batch of one."""
    (cmap,), (k,) = cluster_centroids_batch([centroids], [displacement], thres)
    if as_one_hot:
        return (cmap[None] == torch.arange(k, device=cmap.device, dtype=torch.int32)[:, None, None])
    return cmap, k


def find_centroids_batch(displacements, iterations=300):
    """Batched find_centroids_with_refinement: list of GPU fp32 [2,h,w] -> list of GPU int32 [2,h,w]; one launch for
    the whole batch (irn_find_centroids_batch), nothing synchronises."""
    dps = []
    for d in displacements:
        _need_cuda(d, "displacement")
        dps.append(d.contiguous().float())
    dev = dps[0].device
    outs = [torch.empty((2,) + tuple(d.shape[1:]), dtype=torch.int32, device=dev) for d in dps]
    with torch.cuda.device(dev):
        check(lib.irn_find_centroids_batch(len(dps), ptr_array([d.data_ptr() for d in dps]),
                                           i32_array([d.shape[1] for d in dps]), i32_array([d.shape[2] for d in dps]),
                                           int(iterations), ptr_array([o.data_ptr() for o in outs]), _stream()))
    return outs


def cluster_centroids_batch(centroids, displacements, thres=2.5, k_on_device=False):
    """Batched cluster_centroids: -> (list of GPU int32 [h,w] cluster maps with values 0..K_i-1, list of K_i).
    One launch sequence for the batch and ONE device-to-host transfer for all the K (irn_cluster_centroids_batch).
    `k_on_device`: return the K as the GPU int32 [n] tensor instead — nothing waits for the device, the caller reads them
    (`.cpu()`) when it needs them (the instance step enqueues a batch's front end and goes on loading the next batch)."""
    n = len(centroids)
    dps = [d.contiguous().float() for d in displacements]
    cens = []
    for c in centroids:
        _need_cuda(c, "centroids")
        cens.append(c.to(torch.int32).contiguous())
    dev = dps[0].device
    hs, ws = i32_array([d.shape[1] for d in dps]), i32_array([d.shape[2] for d in dps])
    cmaps = [torch.empty(tuple(d.shape[1:]), dtype=torch.int32, device=dev) for d in dps]
    k_dev = torch.empty(n, dtype=torch.int32, device=dev)
    scratch = cached("cluster_scratch", dev, lib.irn_cluster_batch_scratch_bytes(n, hs, ws), torch.uint8)
    with torch.cuda.device(dev):
        check(lib.irn_cluster_centroids_batch(n, ptr_array([c.data_ptr() for c in cens]),
                                              ptr_array([d.data_ptr() for d in dps]), hs, ws, float(thres),
                                              ptr_array([m.data_ptr() for m in cmaps]), k_dev.data_ptr(),
                                              scratch.data_ptr(), _stream()))
    if k_on_device:
        return cmaps, k_dev
    return cmaps, [int(k) for k in k_dev.cpu().tolist()]


def label4(mask):
    """4-connected components of a GPU mask [n,h,w] or [h,w] (non-zero = foreground): int32 ids 1..
    per image in raster order of each component's first pixel, 0 background; and counts [n]."""
    _need_cuda(mask, "mask")
    squeeze = mask.dim() == 2
    m = (mask != 0).to(torch.uint8).contiguous()
    if squeeze:
        m = m[None]
    n, h, w = m.shape
    labels = torch.empty((n, h, w), dtype=torch.int32, device=m.device)
    counts = torch.empty(n, dtype=torch.int32, device=m.device)
    scratch = torch.empty(lib.irn_ccl_scratch_bytes(n, h, w), dtype=torch.uint8, device=m.device)
    with torch.cuda.device(m.device):
        check(lib.irn_label4(m.data_ptr(), n, h, w, labels.data_ptr(), counts.data_ptr(), scratch.data_ptr(), _stream()))
    return (labels[0], counts[0]) if squeeze else (labels, counts)


def detect_instance(rw_up, argmax, class_ids, n_channels, max_fragment_size=0):
    """Pixel-wise instance ids -> detections (reference step/make_ins_seg_labels.py:82-105), on GPU.

    rw_up: fp32 [C',H,W] normalised scores; argmax: int32 [H,W] (0 = bg, c+1 = channel c);
    class_ids: int64 [C'] (np.repeat(keys, K)).  Every 4-connected component of every channel's
    mask becomes a detection: score = max(rw_up[c] over the component), or 0 when it has fewer than
    max_fragment_size pixels.  Labelling, areas, scores and the [N,H,W] masks are produced by
    libirn_hip.so (irn_detect_instance_batch_count / _emit, a batch of one): one pass over the class map,
    one 4-byte sync for N, one transfer of the result.  Returns the reference's numpy dict {'score','mask','class'}
    in its order (channel ascending, component ascending by first pixel).  Raises ValueError when
    nothing is detected (the reference crashes in np.stack([]) — SURVEY.md §3.5)."""
    _need_cuda(rw_up, "rw_up")
    _need_cuda(argmax, "argmax")
    h, w = argmax.shape
    if tuple(rw_up.shape) != (int(n_channels), h, w):
        raise ValueError("rw_up must be [%d,%d,%d], got %s" % (n_channels, h, w, tuple(rw_up.shape)))
    found = detect_instance_batch([rw_up], [argmax], [class_ids], [n_channels], [max_fragment_size])[0]
    if isinstance(found, ValueError):
        raise found
    return found


_NOTHING = "detect_instance: no foreground pixel in any channel"
_F32, _I32, _I64, _U8 = (np.dtype(t) for t in (np.float32, np.int32, np.int64, np.uint8))


class _PendingBatch:
    """Results of a batched detection whose last transfer to the host may still be in flight: `result()` waits for it once
    and returns the list the blocking call returns.  `host` is None when the batch brings nothing back.  A subclass's
    `_unpack()` returns an iterator over the results of the images that have detections, in order; `_nothing(i)` is what
    image i yields when it has none, here the ValueError `detect_instance` would raise."""

    def __init__(self, nds, host, done, timings=None, t_emit=0.0):
        self._nds, self._host, self._done, self._timings, self._t_emit = nds, host, done, timings, t_emit
        self._out = None

    def _nothing(self, i):
        return ValueError(_NOTHING)

    def result(self):
        if self._out is None:
            if self._host is not None:
                self._done.synchronize()                                           # the batch's last host round trip
            t_done = time.perf_counter()
            found = self._unpack()
            self._out = [next(found) if nd else self._nothing(i) for i, nd in enumerate(self._nds)]
            if self._timings is not None and self._host is not None:
                # seconds: emit + transfer (as far as the caller waited for it), unpacking
                _add(self._timings, "emit_d2h", t_done - self._t_emit)
                _add(self._timings, "unpack", time.perf_counter() - t_done)
        return self._out


def _add(timings, key, value):
    if timings is not None:
        timings[key] = timings.get(key, 0) + value


def _f64_array(values):
    return (C.c_double * len(values))(*[float(v) for v in values])


def _hand_out(pending, deferred):
    return pending if deferred else pending.result()


class _DetCount(collections.namedtuple("_DetCount", "n dev hs ws cs_a hs_a ws_a sc_p am_p keep scratch nds")):
    """What the emit entries take after the labelling half of a batched detection: sizes (lists and int32 arrays), the input
    pointer arrays (`keep` holds the converted inputs alive), the detect scratch and the detection counts."""


def detect_batch_count(rw_ups, argmaxes, n_channels):
    """The labelling half of a batched detection (irn_detect_instance_batch_count) and its one read-back, the detection
    counts.  -> _DetCount"""
    n = len(rw_ups)
    dev = rw_ups[0].device
    scs, ams, hs, ws = [], [], [], []
    for i in range(n):
        _need_cuda(rw_ups[i], "rw_up")
        _need_cuda(argmaxes[i], "argmax")
        am = argmaxes[i].to(torch.int32).contiguous()
        sc = rw_ups[i].contiguous().float()
        h, w = am.shape
        if sc.shape != (int(n_channels[i]), h, w):
            raise ValueError("rw_up[%d] must be [%d,%d,%d], got %s" % (i, n_channels[i], h, w, tuple(sc.shape)))
        scs.append(sc); ams.append(am); hs.append(h); ws.append(w)
    cs_a, hs_a, ws_a = i32_array(n_channels), i32_array(hs), i32_array(ws)
    sc_p, am_p = ptr_array([t.data_ptr() for t in scs]), ptr_array([t.data_ptr() for t in ams])
    scratch = cached("det_scratch_b", dev, lib.irn_detect_batch_scratch_bytes(n, cs_a, hs_a, ws_a), torch.uint8)
    n_det_dev = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.irn_detect_instance_batch_count(n, sc_p, am_p, cs_a, hs_a, ws_a, n_det_dev.data_ptr(),
                                                  scratch.data_ptr(), _stream()))
        nds = [int(v) for v in n_det_dev.cpu().tolist()]                       # host round trip 1
    return _DetCount(n, dev, hs, ws, cs_a, hs_a, ws_a, sc_p, am_p, (scs, ams), scratch, nds)


def _counted(rw_ups, argmaxes, n_channels, timings):
    """`detect_batch_count` with its time (seconds: labelling + count transfer) added to `timings["count"]`.
    -> (_DetCount, the time it returned at: the start of the emit half)"""
    t_start = time.perf_counter()
    dc = detect_batch_count(rw_ups, argmaxes, n_channels)
    t_count = time.perf_counter()
    _add(timings, "count", t_count - t_start)
    return dc, t_count


def _dense_layout(nds, hs, ws):
    """irn_detect_instance_batch_emit's output (include/irn_hip.h): per image
    score f32 [nd] | channel i32 [nd] | pad to 16 | masks u8 [nd*h*w] | pad to 16: three fields per image, named (name, image)."""
    fields = []
    for i, nd in enumerate(nds):
        fields += [(("score", i), _F32, nd, 16), (("channel", i), _I32, nd, 4), (("mask", i), _U8, nd * hs[i] * ws[i], 16)]
    return PackedLayout(fields + [("end", _U8, 0, 16)])


class PendingDetections(_PendingBatch):
    """Detections of a batch whose packed transfer to the host may still be in flight (`detect_instance_batch(...,
    deferred=True)`): `result()` waits for it and returns the list `detect_instance_batch` returns.  The transfer runs on
    a copy stream of its own, so the caller can enqueue the next batch's kernels before collecting this one."""

    def __init__(self, nds, host, done, timings, t_emit, layout, hs, ws, class_ids):
        super().__init__(nds, host, done, timings, t_emit)
        self._layout, self._hs, self._ws, self._class_ids = layout, hs, ws, class_ids

    def _unpack(self):
        v = self._layout.views(self._host.numpy())
        for i, (nd, score, chan, mask) in enumerate(zip(self._nds, v[0::3], v[1::3], v[2::3])):
            if nd:
                yield {"score": score, "mask": mask.view(np.bool_).reshape(nd, self._hs[i], self._ws[i]),
                       "class": np.asarray(self._class_ids[i])[chan]}


def detect_instance_batch(rw_ups, argmaxes, class_ids, n_channels, max_fragment_sizes, timings=None, deferred=False):
    """detect_instance for a batch of images with two host round trips in total: one 4-byte-per-image transfer of the detection counts, one packed transfer of every image's
    {score, channel, masks} (irn_detect_instance_batch_count / _emit).  Arguments are lists (one entry per image) of
    what `detect_instance` takes.  Returns a list with, per image, the reference's numpy dict or — for an image without
    any foreground pixel — the ValueError `detect_instance` would raise.  With `deferred=True` the packed transfer is
    left in flight on a copy stream and a `PendingDetections` is returned: call its `result()` after the next batch has
    been enqueued and the 2 MB of masks per image cross PCIe under that batch's kernels."""
    dc, t_count = _counted(rw_ups, argmaxes, n_channels, timings)
    n, nds = dc.n, dc.nds
    lay = _dense_layout(nds, dc.hs, dc.ws)
    host = done = None
    if lay.nbytes:
        with torch.cuda.device(dc.dev):
            packed = staging("det_out_b", dc.dev, lay.nbytes, 16, own=deferred)
            p = lay.ptrs(packed.data_ptr())[:3 * n]               # (score, channel, mask) image by image
            check(lib.irn_detect_instance_batch_emit(
                n, dc.sc_p, dc.am_p, dc.cs_a, dc.hs_a, dc.ws_a, i32_array(nds), _f64_array(max_fragment_sizes),
                ptr_array(p[0::3]), ptr_array(p[1::3]), ptr_array(p[2::3]), dc.scratch.data_ptr(), _stream()))
            # a page-locked buffer of its own for every batch: the detections are handed out as VIEWS of it (no second copy
            # of 2 MB of masks per image) and it goes back to torch's caching host allocator when the last of them is dropped
            host = torch.empty(lay.nbytes, dtype=torch.uint8, pin_memory=True)
            done = read_back(packed, host, side=deferred)
        _add(timings, "bytes", lay.nbytes)
    return _hand_out(PendingDetections(nds, host, done, timings, t_count, lay, dc.hs, dc.ws, class_ids), deferred)


def _rle_head_layout(G):
    """irn_detect_instance_batch_rle_count's output for G detections (include/irn_hip.h)."""
    return PackedLayout([("score", _F32, G, 1), ("channel", _I32, G, 1), ("area", _I32, G, 1), ("n_runs", _I32, G, 1), ("bbox", _I32, 4 * G, 1)])


class PendingRleDetections(_PendingBatch):
    """`detect_instance_rle_batch(..., deferred=True)`: the run lengths of a batch may still be crossing to the host on the
    copy stream; `result()` waits for them and returns the list `detect_instance_rle_batch` returns.  `head` is the host
    copy (numpy uint8) of the `layout` the count entry wrote, `host` the page-locked buffer of the run lengths."""

    def __init__(self, nds, host, done, timings, t_emit, layout, head, hs, ws, class_ids):
        super().__init__(nds, host, done, timings, t_emit)
        self._layout, self._head, self._hs, self._ws, self._class_ids = layout, head, hs, ws, class_ids

    def _unpack(self):
        score, chan, area, n_runs, bbox = self._layout.views(self._head)
        bbox = bbox.reshape(-1, 4)
        counts = self._host.numpy().view(np.uint32)
        g, at = 0, 0
        for i, nd in enumerate(self._nds):
            if nd == 0:
                continue
            offsets = np.zeros(nd + 1, np.int64)
            np.cumsum(n_runs[g:g + nd], out=offsets[1:])
            total = int(offsets[nd])
            yield {"score": score[g:g + nd], "class": np.asarray(self._class_ids[i])[chan[g:g + nd]],
                   "size": (self._hs[i], self._ws[i]), "counts": counts[at:at + total], "offsets": offsets,
                   "area": area[g:g + nd].astype(np.int64), "bbox": bbox[g:g + nd]}
            g += nd
            at += total


def detect_instance_rle_batch(rw_ups, argmaxes, class_ids, n_channels, max_fragment_sizes, timings=None, deferred=False):
    """`detect_instance_batch` with every mask as its COCO run-length code instead of a dense plane
    (irn_detect_instance_batch_rle_count / _emit): same arguments, same detections in the same order.  Returns per image
    {"score" f32 [N], "class" i64 [N], "size" (H, W), "counts" u32 [total], "offsets" i64 [N+1], "area" i64 [N], "bbox"
    i32 [N,4]} — detection d's run lengths are counts[offsets[d]:offsets[d+1]], exactly what
    `mask_rle(detect_instance_batch(...)["mask"])` gives — or the ValueError of an image without a foreground pixel.
    No [N,H,W] block exists on either side of PCIe.  Three host round trips per batch, one more than the dense form: the
    detection counts; then score, channel, area, n_runs and bbox of every detection (32 bytes each — the added read-back:
    the number of run lengths depends on the data and sizes the last transfer); then the run lengths.  `deferred=True`
    leaves that last transfer in flight on the copy stream and returns a `PendingRleDetections`.  `timings["bytes"]`
    counts the device-to-host bytes of all three."""
    dc, t_count = _counted(rw_ups, argmaxes, n_channels, timings)
    n, dev, nds = dc.n, dc.dev, dc.nds
    G = sum(nds)
    lay = _rle_head_layout(G)
    if G == 0:
        return _hand_out(PendingRleDetections(nds, None, None, timings, t_count, lay, None, dc.hs, dc.ws, class_ids), deferred)
    nd_a = i32_array(nds)
    with torch.cuda.device(dev):
        rle_scratch = cached("det_rle_scratch", dev, lib.irn_detect_instance_batch_rle_scratch_bytes(n, dc.hs_a, dc.ws_a, nd_a),
                             torch.uint8)
        head_dev = cached("det_rle_head", dev, lay.nbytes, torch.uint8)
        p_score, p_chan, p_area, p_runs, p_bbox = lay.ptrs(head_dev.data_ptr())
        check(lib.irn_detect_instance_batch_rle_count(
            n, dc.sc_p, dc.am_p, dc.cs_a, dc.hs_a, dc.ws_a, nd_a, _f64_array(max_fragment_sizes),
            p_score, p_chan, p_area, p_runs, p_bbox, dc.scratch.data_ptr(), rle_scratch.data_ptr(), _stream()))
        head_host = torch.empty(lay.nbytes, dtype=torch.uint8, pin_memory=True)
        read_back(head_dev[:lay.nbytes], head_host, side=False).synchronize()      # host round trip 2
        head = head_host.numpy()
        n_runs = lay.views(head)[3]
        runs, g = [], 0
        for nd in nds:
            runs.append(int(n_runs[g:g + nd].sum(dtype=np.int64)))
            g += nd
        total = sum(runs)
        ws_bytes = lib.irn_detect_instance_batch_rle_sort_bytes(total, G)
        if ws_bytes == 0:
            check(1)
        sort_ws = cached("det_rle_sort", dev, ws_bytes, torch.uint8)
        counts_dev = staging("det_rle_counts", dev, 4 * total, 1, own=deferred)
        check(lib.irn_detect_instance_batch_rle_emit(n, dc.hs_a, dc.ws_a, nd_a, (C.c_int64 * n)(*runs), counts_dev.data_ptr(),
                                                     rle_scratch.data_ptr(), sort_ws.data_ptr(), ws_bytes, _stream()))
        host = torch.empty(4 * total, dtype=torch.uint8, pin_memory=True)
        done = read_back(counts_dev, host, side=deferred)
    _add(timings, "bytes", 4 * n + lay.nbytes + 4 * total)
    return _hand_out(PendingRleDetections(nds, host, done, timings, t_count, lay, head, dc.hs, dc.ws, class_ids), deferred)


def _overlap_layout(nds, gs):
    """irn_detect_instance_batch_overlap's output (include/irn_hip.h), G detections, NG GT instances, NI = sum nd_i * g_i."""
    G, NG, NI = sum(nds), sum(gs), sum(nd * g for nd, g in zip(nds, gs))
    return PackedLayout([("inter", _I64, NI, 1), ("area_gt", _I64, NG, 1), ("area_pred", _I64, G, 1), ("score", _F32, G, 1), ("channel", _I32, G, 1)])


class PendingOverlaps(_PendingBatch):
    """`detection_overlap_batch(..., deferred=True)`: the packed counts of a batch may still be crossing to the host on the
    copy stream; `result()` waits for them and returns the list `detection_overlap_batch` returns (an image without a
    detection has a record with N = 0 and its GT areas, not an error)."""

    def __init__(self, nds, host, done, layout, gs, class_ids):
        super().__init__(nds, host, done)
        self._layout, self._gs, self._class_ids = layout, gs, class_ids

    def _unpack(self):
        # a few bytes per detection: the records are copies, the page-locked buffer is not kept by them
        raw = np.zeros(0, np.uint8) if self._host is None else self._host.numpy().copy()
        self._fields = self._layout.views(raw)
        self._at, d, a, x = [], 0, 0, 0
        for nd, g in zip(self._nds, self._gs):
            self._at.append((d, a, x))
            d, a, x = d + nd, a + g, x + nd * g
        return (self._record(i) for i, nd in enumerate(self._nds) if nd)

    def _record(self, i):
        """Image i's record; without a detection the same slices give the N = 0 record with its GT areas."""
        (nd, g), (d, a, x), (inter, area_gt, area_pred, score, chan) = (self._nds[i], self._gs[i]), self._at[i], self._fields
        return {"pred_class": np.asarray(self._class_ids[i])[chan[d:d + nd]], "pred_score": score[d:d + nd],
                "inter": inter[x:x + nd * g].reshape(nd, g), "area_pred": area_pred[d:d + nd], "area_gt": area_gt[a:a + g]}

    _nothing = _record


def detection_overlap_batch(rw_ups, argmaxes, class_ids, n_channels, max_fragment_sizes, inst_maps, n_insts, bad=None,
                            deferred=False):
    """`detect_instance_batch` + `mask_overlap` for a batch without any mask (irn_detect_instance_batch_count / _overlap):
    the detections of `detect_instance_batch` (same arguments, same order) are counted against the GT instance maps
    straight from the labelled map.  inst_maps[i]: uint8 [H,W] GPU tensor (0 = no instance, 1..n_insts[i]); values above
    n_insts[i] are counted in bad int64 [1] (added into), as `mask_overlap` counts them.  Returns per image
    {"pred_class" i64 [N], "pred_score" f32 [N], "inter" i64 [N,G], "area_pred" i64 [N], "area_gt" i64 [G]} — the counts
    `mask_overlap` gives on the masks of `detect_instance_batch`, under the names `misc.evaluation.instance_ap_voc` reads;
    an image without any detection has a record with N = 0 (and its GT areas).  Two host round trips per call: the
    detection counts, and one packed transfer of everything else; `deferred=True` leaves that one in flight on the copy
    stream and returns a `PendingOverlaps`."""
    n = len(rw_ups)
    if not (len(argmaxes) == len(class_ids) == len(n_channels) == len(max_fragment_sizes) == len(inst_maps) == len(n_insts) == n):
        raise ValueError("detection_overlap_batch: every argument is a list with one entry per image (%d score maps)" % n)
    if n == 0:
        return PendingOverlaps([], None, None, _overlap_layout([], []), [], []) if deferred else []
    dev = rw_ups[0].device
    gs = [int(g) for g in n_insts]
    insts = []
    for i in range(n):
        _need_cuda(inst_maps[i], "inst_map")
        m = u8_map(inst_maps[i], dev, "inst_map")
        if tuple(m.shape) != tuple(argmaxes[i].shape):
            raise ValueError("detection_overlap_batch: instance map %d is %s for a map of %s" % (i, tuple(m.shape), tuple(argmaxes[i].shape)))
        if not 0 <= gs[i] <= 255:
            raise ValueError("detection_overlap_batch: image %d has %d GT instances (0..255)" % (i, gs[i]))
        insts.append(m)
    bad = accumulator(bad, (1,), dev, "bad")
    dc = detect_batch_count(rw_ups, argmaxes, n_channels)                          # host round trip 1
    nds = dc.nds
    lay = _overlap_layout(nds, gs)
    host = done = None
    with torch.cuda.device(dev):
        packed = staging("det_ovl_out", dev, lay.nbytes, 8, own=deferred)
        p_inter, p_area_gt, p_area_pred, p_score, p_chan = lay.ptrs(packed.data_ptr())
        check(lib.irn_detect_instance_batch_overlap(
            n, dc.sc_p, dc.am_p, dc.cs_a, dc.hs_a, dc.ws_a, i32_array(nds), _f64_array(max_fragment_sizes),
            ptr_array([m.data_ptr() for m in insts]), i32_array(gs), p_score, p_chan, p_area_pred, p_inter, p_area_gt, bad.data_ptr(),
            dc.scratch.data_ptr(), _stream()))
        if lay.nbytes:
            host = torch.empty(lay.nbytes, dtype=torch.uint8, pin_memory=True)
            done = read_back(packed, host, side=deferred)                          # host round trip 2
    return _hand_out(PendingOverlaps(nds, host, done, lay, gs, class_ids), deferred)


def argmax_rethreshold_batch(rw_ups, argmaxes, thres):
    """The `argmax` maps `label_epilogue(..., bg_thres=thres, want_argmax=True)` returns, from the `rw_up` / `argmax` of ONE
    epilogue at a threshold not above `thres` (irn_argmax_rethreshold_batch): a pixel keeps its channel where that
    channel's score is NaN or > thres and becomes 0 elsewhere.  Lists of GPU tensors in, a list of new int32 [H,W] maps
    out, bit for bit the epilogue's."""
    n = len(rw_ups)
    if len(argmaxes) != n:
        raise ValueError("argmax_rethreshold_batch: %d score maps, %d argmax maps" % (n, len(argmaxes)))
    if n == 0:
        return []
    scs, ams = [], []
    for i in range(n):
        _need_cuda(rw_ups[i], "rw_up")
        _need_cuda(argmaxes[i], "argmax")
        sc, am = rw_ups[i].contiguous().float(), argmaxes[i].to(torch.int32).contiguous()
        if sc.dim() != 3 or am.dim() != 2 or sc.shape[0] < 1 or tuple(sc.shape[1:]) != tuple(am.shape):
            raise ValueError("argmax_rethreshold_batch: rw_up[%d] is %s for an argmax of %s" % (i, tuple(sc.shape), tuple(am.shape)))
        scs.append(sc); ams.append(am)
    dev = scs[0].device
    outs = [torch.empty_like(am) for am in ams]
    with torch.cuda.device(dev):
        check(lib.irn_argmax_rethreshold_batch(
            n, ptr_array([t.data_ptr() for t in scs]), ptr_array([t.data_ptr() for t in ams]), i32_array([t.shape[0] for t in scs]),
            i32_array([t.shape[0] for t in ams]), i32_array([t.shape[1] for t in ams]), float(thres),
            ptr_array([t.data_ptr() for t in outs]), _stream()))
    return outs
