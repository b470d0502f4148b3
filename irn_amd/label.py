"""Host side of irn_amd/csrc/label.hip: the label epilogue (x4 upsample, normalise, background, argmax), the same scores
counted against ground truth at a sweep of thresholds, and the multi-scale CAM merge.  `irn_amd.ops` re-exports the
functions.  GPU tensors in, GPU tensors out; no CPU fallback."""
import numpy as np
import torch

from ._host import accumulator
from ._lib import _need_cuda, _stream, check, i32_array, lib, ptr_array
from .eval_counts import EVAL_CLASSES, EVAL_MAX_THRES, _thres_tensor, eval_classes


def _label_inputs(rws, out_sizes, keys):
    """-> contiguous fp32 [C,h,w] score tensors, (H, W) int pairs and, where `keys` is given, flat int64 key tensors on the
    scores' device: one of each per score tensor (a short list is an IndexError)."""
    n, dev = len(rws), rws[0].device
    for r in rws:
        _need_cuda(r, "rw")
    rs = [r.reshape((-1,) + tuple(r.shape[-2:])).contiguous().float() for r in rws]
    sizes = [(int(out_sizes[i][0]), int(out_sizes[i][1])) for i in range(n)]
    if keys is not None:
        keys = [torch.as_tensor(keys[i], device=dev).to(torch.int64).reshape(-1).contiguous() for i in range(n)]
    return rs, sizes, keys


def label_epilogue(rws, out_sizes, bg_thres, keys=None, want_labels=True, want_argmax=False, want_rw_up=False, packed=False):
    """Batched x4-upsample / normalise / background / argmax.

    rws[i]: GPU fp32 [C,1,h,w] (or [C,h,w]); out_sizes[i] = (H, W) with H <= 4h, W <= 4w;
    keys[i]: GPU int64 [C] (0-based class ids, the CAM dict's ``keys``) when labels are wanted.
    Returns dict of lists: 'labels' uint8 [H,W] (0 = background, else key+1), 'argmax' int32 [H,W],
    'rw_up' fp32 [C,H,W] (divided by the global max) — each present only if requested.  With `packed` the label maps are
    views of ONE uint8 buffer, returned as 'labels_flat' (a step brings a whole batch to the host with one copy)."""
    n = len(rws)
    dev = rws[0].device
    if want_labels and keys is None:
        raise ValueError("labels need keys")
    rs, sizes, ks = _label_inputs(rws, out_sizes, keys if want_labels else None)
    cs, hs, ws = ([r.shape[d] for r in rs] for d in range(3))
    ohs, ows = [s[0] for s in sizes], [s[1] for s in sizes]
    labels = flat = None
    if want_labels and packed:
        offs = np.concatenate([[0], np.cumsum([ohs[i] * ows[i] for i in range(n)])])
        flat = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
        labels = [flat[int(offs[i]):int(offs[i + 1])].view(ohs[i], ows[i]) for i in range(n)]
    elif want_labels:
        labels = [torch.empty((ohs[i], ows[i]), dtype=torch.uint8, device=dev) for i in range(n)]
    argmax = [torch.empty((ohs[i], ows[i]), dtype=torch.int32, device=dev) for i in range(n)] if want_argmax else None
    rw_up = [torch.empty((cs[i], ohs[i], ows[i]), dtype=torch.float32, device=dev) for i in range(n)] if want_rw_up else None
    scratch = torch.empty(max(n, 64), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.irn_label_epilogue(
            n, ptr_array([r.data_ptr() for r in rs]), i32_array(cs), i32_array(hs), i32_array(ws),
            i32_array(ohs), i32_array(ows), float(bg_thres),
            None if ks is None else ptr_array([k.data_ptr() for k in ks]),
            None if labels is None else ptr_array([t.data_ptr() for t in labels]),
            None if argmax is None else ptr_array([t.data_ptr() for t in argmax]),
            None if rw_up is None else ptr_array([t.data_ptr() for t in rw_up]),
            scratch.data_ptr(), _stream()))
    out = {}
    if want_labels:
        out["labels"] = labels
        if flat is not None:
            out["labels_flat"] = flat
    if want_argmax:
        out["argmax"] = argmax
    if want_rw_up:
        out["rw_up"] = rw_up
    return out


def label_sweep_confusion(rws, out_sizes, keys, gts, thres, hist=None, bad=None, n_classes=EVAL_CLASSES):
    """`label_epilogue` + `label_confusion` at every background threshold of `thres` in one pass, for a batch (no label
    map and no upsampled tensor is written), by the epilogue's own score functions and `cam_confusion`'s counting code.

    rws, out_sizes, keys: as for `label_epilogue` (at most 20 channels per image); gts: a list of uint8 [H,W] GPU tensors
    (255 = void), or ONE flat uint8 GPU buffer that holds the maps of `out_sizes` back to back; thres: GPU fp32 [T] from
    `eval_thresholds` (or anything it takes).  Adds into hist int64 [22,21,T+1] — the layout of `cam_confusion`, so
    `cam_confusion_matrices(hist)` gives the T matrices `label_confusion` counts on the labels of each threshold — and
    bad int64 [1]; returns (hist, bad).  Everything is checked before the launch: a refusal leaves hist / bad untouched.
    With n_classes = nc (background included, 2..81): at most nc-1 channels per image and hist [nc+1,nc,T+1]."""
    nc = eval_classes(n_classes, "label_sweep_confusion")
    n = len(rws)
    if n < 1 or len(out_sizes) != n or len(keys) != n:
        raise ValueError("label_sweep_confusion: %d score maps, %d sizes, %d key lists" % (n, len(out_sizes), len(keys)))
    dev = rws[0].device
    for i, r in enumerate(rws):
        _need_cuda(r, "rw")
        if r.dim() < 2 or r.device != dev:
            raise ValueError("label_sweep_confusion: rw %d must be a [C,1,h,w] or [C,h,w] tensor on %s" % (i, dev))
    rs, sizes, ks = _label_inputs(rws, out_sizes, keys)
    if isinstance(gts, torch.Tensor):
        _need_cuda(gts, "gts")
        total = sum(hh * ww for hh, ww in sizes)
        if gts.dtype != torch.uint8 or gts.dim() != 1 or not gts.is_contiguous() or gts.numel() != total or gts.device != dev:
            raise ValueError("label_sweep_confusion: the packed ground truth must be a flat uint8 buffer of %d bytes on %s"
                             % (total, dev))
        offs = np.concatenate([[0], np.cumsum([hh * ww for hh, ww in sizes])])
        gt_ptrs = [gts.data_ptr() + int(o) for o in offs[:-1]]
        gs = gts
    else:
        if len(gts) != n:
            raise ValueError("label_sweep_confusion: %d ground-truth maps for %d images" % (len(gts), n))
        gs = []
        for i, g in enumerate(gts):
            _need_cuda(g, "gt")
            if g.dtype != torch.uint8 or g.dim() != 2 or g.device != dev:
                raise ValueError("label_sweep_confusion: gt %d must be a uint8 [H,W] tensor on %s" % (i, dev))
            if tuple(g.shape) != sizes[i]:
                raise ValueError("label_sweep_confusion: gt %d is %s for an output of %s" % (i, tuple(g.shape), sizes[i]))
            gs.append(g.contiguous())
        gt_ptrs = [g.data_ptr() for g in gs]
    for i, (r, k) in enumerate(zip(rs, ks)):
        if not 1 <= r.shape[0] <= nc - 1:
            raise ValueError("label_sweep_confusion: image %d has %d channels (1..%d)" % (i, r.shape[0], nc - 1))
        if not (1 <= sizes[i][0] <= 4 * r.shape[1] and 1 <= sizes[i][1] <= 4 * r.shape[2]):
            raise ValueError("label_sweep_confusion: image %d: output %s from a %dx%d map" % (i, sizes[i], r.shape[1], r.shape[2]))
        if k.numel() != r.shape[0]:
            raise ValueError("label_sweep_confusion: image %d: %d keys for %d channels" % (i, k.numel(), r.shape[0]))
    th, t = _thres_tensor(thres, dev)
    if not 1 <= t <= EVAL_MAX_THRES:
        raise ValueError("label_sweep_confusion: %d thresholds (1..%d)" % (t, EVAL_MAX_THRES))
    hist = accumulator(hist, (nc + 1, nc, t + 1), dev, "hist")
    bad = accumulator(bad, (1,), dev, "bad")
    scratch = torch.empty(max(n, 64), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.irn_label_sweep_confusion(
            n, ptr_array([r.data_ptr() for r in rs]), i32_array([r.shape[0] for r in rs]), i32_array([r.shape[1] for r in rs]),
            i32_array([r.shape[2] for r in rs]), i32_array([s[0] for s in sizes]), i32_array([s[1] for s in sizes]),
            ptr_array([k.data_ptr() for k in ks]), ptr_array(gt_ptrs), th.data_ptr(), t, nc, hist.data_ptr(), bad.data_ptr(),
            scratch.data_ptr(), _stream()))
    return hist, bad


def cam_merge(outputs, size, label):
    """Multi-scale CAM merge of reference step/make_cam.py:38-52 (irn_cam_merge).

    outputs: list of GPU fp32 [n_classes, hs, ws] (one per scale); size = (H, W) of the image;
    label: [n_classes] multi-hot image-level label (pass it as a HOST tensor to keep the call asynchronous).  Returns (keys int64 [K] on the same device,
    cam fp32 [K, ceil(H/4), ceil(W/4)], high_res fp32 [K, H, W]), each channel divided by its max + 1e-5."""
    for o in outputs:
        _need_cuda(o, "CAM output")
    dev = outputs[0].device
    outs = [o.contiguous().float() for o in outputs]
    n_cls = outs[0].shape[0]
    H, W = int(size[0]), int(size[1])
    label = torch.as_tensor(label)
    if label.is_cuda:
        keys = torch.nonzero(label.to(dev))[:, 0].to(torch.int64).contiguous()          # synchronises (data-dependent size)
    else:
        # the loader hands the image-level label over on the host: the present classes are found there and only the
        # key list travels, so the call never waits for the device (a device-side nonzero needs its result size)
        keys = torch.nonzero(label)[:, 0].to(torch.int64).contiguous().to(dev, non_blocking=True)
    k = int(keys.numel())
    cam = torch.empty((k, (H - 1) // 4 + 1, (W - 1) // 4 + 1), dtype=torch.float32, device=dev)
    hi = torch.empty((k, H, W), dtype=torch.float32, device=dev)
    scratch = torch.empty(2 * k, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.irn_cam_merge(len(outs), ptr_array([o.data_ptr() for o in outs]), i32_array([o.shape[1] for o in outs]),
                                i32_array([o.shape[2] for o in outs]), n_cls, keys.data_ptr(), k, H, W, cam.data_ptr(),
                                hi.data_ptr(), scratch.data_ptr(), _stream()))
    return keys, cam, hi
