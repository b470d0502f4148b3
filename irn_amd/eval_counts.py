"""Host side of irn_amd/csrc/eval.hip: the integer counts behind the evaluation steps (step/eval_cam.py,
step/eval_sem_seg.py, step/eval_ins_seg.py of the reference): irn_cam_confusion, irn_label_confusion, irn_mask_overlap,
the grid count of step/tune_ir_label.py, irn_ir_label_confusion, and the boundary bands and band counts of Boundary IoU /
Boundary AP (irn_label_band, irn_label_boundary_counts, irn_mask_boundary_overlap; not in the reference).
Accumulators are int64 GPU tensors that every call adds into; `bad` (int64 [1]) counts values outside the documented
ranges and the caller raises when it is non-zero.  `irn_amd.ops` re-exports the functions."""
import ctypes as C

import numpy as np
import torch

from ._host import accumulator, u8_map
from ._lib import _need_cuda, _stream, check, lib

EVAL_CLASSES = 21                     # background + 20 VOC classes: the default class count everywhere
EVAL_MAX_CLASSES = 81                 # IRN_EVAL_MAX_CLASSES: background + 80
EVAL_MAX_THRES = 256                  # IRN_EVAL_MAX_THRES


def eval_classes(n_classes, who):
    """`n_classes` (classes including the background) as an int in 2..EVAL_MAX_CLASSES, or a ValueError naming `who`."""
    nc = int(n_classes)
    if nc != n_classes or not 2 <= nc <= EVAL_MAX_CLASSES:
        raise ValueError("%s: n_classes %s outside 2..%d (background included)" % (who, n_classes, EVAL_MAX_CLASSES))
    return nc


def _i64_zeros(shape, dev):
    return torch.zeros(shape, dtype=torch.int64, device=dev)


def eval_thresholds(thres, dev):
    """Thresholds as the float32 GPU tensor the confusion kernel reads; ascending, 1..EVAL_MAX_THRES of them (the step
    pads the background plane with float32(t), as np.pad does on a float32 CAM)."""
    th = np.asarray(thres, np.float32).reshape(-1)
    if not 1 <= th.size <= EVAL_MAX_THRES or np.isnan(th).any() or (np.diff(th) < 0).any():
        raise ValueError("eval thresholds: 1..%d ascending values, got %s" % (EVAL_MAX_THRES, th))
    return torch.from_numpy(th).to(dev)


def _thres_tensor(thres, dev):
    """-> (flat float32 tensor on dev, its length): a float32 GPU tensor as given, anything else through `eval_thresholds`."""
    th = thres if isinstance(thres, torch.Tensor) and thres.is_cuda and thres.dtype == torch.float32 else eval_thresholds(thres, dev)
    th = th.to(dev).reshape(-1).contiguous()
    return th, int(th.numel())


def cam_confusion(high_res, keys, gt, thres, hist=None, bad=None, n_classes=EVAL_CLASSES):
    """step/eval_cam.py:14-19 + the confusion count for one image at every threshold of `thres` in one pass.

    high_res: GPU fp32 [K,H,W] (K >= 0), keys: 0-based classes [K], gt: uint8 [H,W] (255 = void), thres: GPU fp32 [T] from
    `eval_thresholds` (or anything it takes).  Adds into hist int64 [22,21,T+1] (row 21 = void GT, include/irn_hip.h) and
    bad int64 [1]; returns (hist, bad).  `cam_confusion_matrices(hist)` turns the histogram into the T matrices.
    n_classes (nc: classes including the background, 2..81): hist is [nc+1,nc,T+1], keys are 0..nc-2, GT 0..nc-1 or 255."""
    nc = eval_classes(n_classes, "cam_confusion")
    _need_cuda(high_res, "high_res")
    dev = high_res.device
    g = u8_map(gt, dev, "gt")
    h, w = g.shape
    cams = high_res.to(torch.float32).contiguous()
    k = int(cams.shape[0]) if cams.dim() == 3 else -1
    if k < 0 or (k and tuple(cams.shape[1:]) != (h, w)):
        raise ValueError("cam_confusion: high_res %s for a GT of %dx%d" % (tuple(cams.shape), h, w))
    if k > nc - 1:
        raise ValueError("cam_confusion: %d CAM planes (at most %d)" % (k, nc - 1))
    ks = torch.as_tensor(keys).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if ks.numel() != k:
        raise ValueError("cam_confusion: %d keys for %d CAM planes" % (ks.numel(), k))
    th, t = _thres_tensor(thres, dev)
    hist = accumulator(hist, (nc + 1, nc, t + 1), dev, "hist")
    bad = accumulator(bad, (1,), dev, "bad")
    with torch.cuda.device(dev):
        check(lib.irn_cam_confusion(cams.data_ptr() if k else None, ks.data_ptr() if k else None, k, g.data_ptr(), h, w,
                                    th.data_ptr(), t, nc, hist.data_ptr(), bad.data_ptr(), _stream()))
    return hist, bad


def cam_confusion_matrices(hist, n_classes=EVAL_CLASSES):
    """hist int64 [22,21,T+1] of `cam_confusion` -> (conf int64 [T,21,21] (row = GT, column = prediction), void int64
    [T,21] (predictions at GT-255 pixels)), on the GPU; with n_classes = nc, [nc+1,nc,T+1] -> [T,nc,nc] and [T,nc]."""
    nc = eval_classes(n_classes, "cam_confusion_matrices")
    _need_cuda(hist, "hist")
    t = int(hist.shape[2]) - 1
    hist = accumulator(hist, (nc + 1, nc, t + 1), hist.device, "hist")
    conf = _i64_zeros((t, nc, nc), hist.device)
    void = _i64_zeros((t, nc), hist.device)
    with torch.cuda.device(hist.device):
        check(lib.irn_cam_confusion_reduce(hist.data_ptr(), t, nc, conf.data_ptr(), void.data_ptr(), _stream()))
    return conf, void


def label_confusion(pred, gt, conf=None, bad=None, pred_255_as=0, void=None, n_classes=EVAL_CLASSES):
    """step/eval_sem_seg.py:14-17 for one image: pred, gt uint8 [H,W] GPU tensors (pred 255 reads as `pred_255_as`; None =
    out of range).  Adds into conf int64 [21,21], void int64 [21] (predictions at GT-255 pixels) and bad int64 [1];
    returns (conf, void, bad).  With n_classes = nc (background included): conf [nc,nc], void [nc], values 0..nc-1."""
    nc = eval_classes(n_classes, "label_confusion")
    _need_cuda(pred, "pred")
    dev = pred.device
    p = u8_map(pred, dev, "pred")
    g = u8_map(gt, dev, "gt")
    if p.shape != g.shape:
        raise ValueError("label_confusion: prediction %s for a GT of %s" % (tuple(p.shape), tuple(g.shape)))
    conf = accumulator(conf, (nc, nc), dev, "conf")
    void = accumulator(void, (nc,), dev, "void")
    bad = accumulator(bad, (1,), dev, "bad")
    h, w = g.shape
    with torch.cuda.device(dev):
        check(lib.irn_label_confusion(p.data_ptr(), g.data_ptr(), h, w, -1 if pred_255_as is None else int(pred_255_as),
                                      nc, conf.data_ptr(), void.data_ptr(), bad.data_ptr(), _stream()))
    return conf, void, bad


def mask_overlap(masks, inst_map, n_inst, bad=None):
    """The counts behind chainercv's mask_iou for one image: masks bool/uint8 [N,H,W] and inst_map uint8 [H,W] (0 = no
    instance, 1..n_inst) on the GPU.  Returns (inter int64 [N,G], area_pred int64 [N], area_gt int64 [G]) on the GPU, with
    IoU = inter / (area_pred + area_gt - inter); values of inst_map above n_inst are counted in bad int64 [1]."""
    _need_cuda(inst_map, "inst_map")
    dev = inst_map.device
    inst = u8_map(inst_map, dev, "inst_map")
    h, w = inst.shape
    if not (isinstance(masks, torch.Tensor) and masks.dim() == 3 and masks.dtype in (torch.uint8, torch.bool)):
        raise ValueError("mask_overlap: masks must be a bool / uint8 [N,H,W] tensor")
    m = masks.to(dev)
    m = (m.view(torch.uint8) if m.dtype == torch.bool else m).contiguous()
    n, g = int(m.shape[0]), int(n_inst)
    if tuple(m.shape[1:]) != (h, w):
        raise ValueError("mask_overlap: masks %s for an instance map of %dx%d" % (tuple(m.shape), h, w))
    inter = _i64_zeros((n, g), dev)
    area_pred = _i64_zeros((n,), dev)
    area_gt = _i64_zeros((g,), dev)
    bad = accumulator(bad, (1,), dev, "bad")
    with torch.cuda.device(dev):
        check(lib.irn_mask_overlap(m.data_ptr() if n else None, n, inst.data_ptr(), g, h, w,
                                   inter.data_ptr() if n and g else None, area_pred.data_ptr() if n else None,
                                   area_gt.data_ptr() if g else None, bad.data_ptr(), _stream()))
    return inter, area_pred, area_gt


def ir_label_confusion(planes, fg_idx, bg_idx, gt, hist=None, bad=None, n_classes=EVAL_CLASSES):
    """step/cam_to_ir_label.py:36-39 + the confusion count for every (fg, bg) pair of a threshold grid, from the planes of
    `crf_label_sweep`: planes uint8 [T,H,W] (GPU), fg_idx [F] / bg_idx [B] plane numbers (1..16 each, repeats allowed), gt
    uint8 [H,W] (255 = void).  Pair (i, j) labels a pixel planes[fg_idx[i]] where that is not 0, else 0 where
    planes[bg_idx[j]] is 0 too, else 255.  Adds into hist int64 [F,B,22,22] (row = GT, 21 = void; column = label, 21 = 255)
    and bad int64 [1]; returns (hist, bad).  No label map is written.  With n_classes = nc (background included): hist
    [F,B,nc+1,nc+1], plane values 0..nc-1; a grid too large for one workgroup's LDS is counted in several launches."""
    nc = eval_classes(n_classes, "ir_label_confusion")
    _need_cuda(planes, "planes")
    dev = planes.device
    if planes.dtype != torch.uint8 or planes.dim() != 3:
        raise ValueError("ir_label_confusion: planes must be a uint8 [T,H,W] tensor, got %s %s" % (planes.dtype, tuple(planes.shape)))
    pl = planes.contiguous()
    g = u8_map(gt, dev, "gt")
    t, h, w = (int(v) for v in pl.shape)
    if tuple(g.shape) != (h, w):
        raise ValueError("ir_label_confusion: planes %s for a GT of %s" % (tuple(pl.shape), tuple(g.shape)))
    fg = np.ascontiguousarray(np.asarray(fg_idx, np.int32).reshape(-1))
    bg = np.ascontiguousarray(np.asarray(bg_idx, np.int32).reshape(-1))
    hist = accumulator(hist, (fg.size, bg.size, nc + 1, nc + 1), dev, "hist")
    bad = accumulator(bad, (1,), dev, "bad")
    pi32 = C.POINTER(C.c_int32)
    with torch.cuda.device(dev):
        check(lib.irn_ir_label_confusion(pl.data_ptr(), t, fg.ctypes.data_as(pi32), int(fg.size), bg.ctypes.data_as(pi32),
                                         int(bg.size), g.data_ptr(), h, w, nc, hist.data_ptr(), bad.data_ptr(), _stream()))
    return hist, bad


BAND_MAX_D = 64                       # IRN_BAND_MAX_D


def boundary_distance(h, w, ratio):
    """The band width of Boundary IoU for an h x w image: max(1, round(ratio * diagonal)), in Python doubles with Python's
    round (ties to even), as the published code computes it; 375x500 at 0.02 -> 12."""
    return max(1, int(round(float(ratio) * (int(h) * int(h) + int(w) * int(w)) ** 0.5)))


def _band_d(d, who):
    if int(d) != d or not 1 <= int(d) <= BAND_MAX_D:
        raise ValueError("%s: d %s outside 1..%d" % (who, d, BAND_MAX_D))
    return int(d)


def label_band(label_map, d):
    """band(label_map, d) of DESIGN.md "Boundary IoU": label_map uint8 [H,W] on the GPU -> uint8 [H,W], 1 where the square
    window of half-width d around the pixel leaves the image or holds another byte.  Every byte value is a label."""
    _need_cuda(label_map, "label_map")
    dev = label_map.device
    m = u8_map(label_map, dev, "label_map")
    d = _band_d(d, "label_band")
    h, w = m.shape
    out = torch.empty((h, w), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.irn_label_band(m.data_ptr(), h, w, d, out.data_ptr(), _stream()))
    return out


def label_boundary_counts(pred, gt, d, counts=None, bad=None, pred_255_as=0, n_classes=EVAL_CLASSES):
    """The Boundary IoU counts of one image: pred, gt uint8 [H,W] GPU tensors as for `label_confusion`, d from
    `boundary_distance`.  Adds into counts int64 [nc,3] — per class the pixels in both bands with pred == gt == c, those of
    the prediction's band with pred == c and those of the GT's band with gt == c (void GT pixels are labels when the band is
    formed and are counted nowhere) — and bad int64 [1]; returns (counts, bad)."""
    nc = eval_classes(n_classes, "label_boundary_counts")
    _need_cuda(pred, "pred")
    dev = pred.device
    p = u8_map(pred, dev, "pred")
    g = u8_map(gt, dev, "gt")
    if p.shape != g.shape:
        raise ValueError("label_boundary_counts: prediction %s for a GT of %s" % (tuple(p.shape), tuple(g.shape)))
    d = _band_d(d, "label_boundary_counts")
    counts = accumulator(counts, (nc, 3), dev, "counts")
    bad = accumulator(bad, (1,), dev, "bad")
    h, w = g.shape
    with torch.cuda.device(dev):
        check(lib.irn_label_boundary_counts(p.data_ptr(), g.data_ptr(), h, w, d, -1 if pred_255_as is None else int(pred_255_as),
                                            nc, counts.data_ptr(), bad.data_ptr(), _stream()))
    return counts, bad


def mask_boundary_overlap(masks, inst_map, n_inst, d, bad=None, inst_band=None):
    """The Boundary AP counts of one image, arguments as for `mask_overlap`: every mask's band (the mask as a two-valued
    map, kept where it is set) against the instances' bands (band(inst_map, d) where inst_map is not 0).  Returns (inter_b
    int64 [N,G], band_pred int64 [N], band_gt int64 [G]) on the GPU; ids above n_inst are counted in bad int64 [1].
    inst_band: a flat uint8 GPU tensor of at least H*W elements to use as scratch (one of its own otherwise); the call
    leaves band(inst_map, d) in its head."""
    _need_cuda(inst_map, "inst_map")
    dev = inst_map.device
    inst = u8_map(inst_map, dev, "inst_map")
    h, w = inst.shape
    if not (isinstance(masks, torch.Tensor) and masks.dim() == 3 and masks.dtype in (torch.uint8, torch.bool)):
        raise ValueError("mask_boundary_overlap: masks must be a bool / uint8 [N,H,W] tensor")
    m = masks.to(dev)
    m = (m.view(torch.uint8) if m.dtype == torch.bool else m).contiguous()
    n, g = int(m.shape[0]), int(n_inst)
    if tuple(m.shape[1:]) != (h, w):
        raise ValueError("mask_boundary_overlap: masks %s for an instance map of %dx%d" % (tuple(m.shape), h, w))
    d = _band_d(d, "mask_boundary_overlap")
    if inst_band is None:
        inst_band = torch.empty(h * w, dtype=torch.uint8, device=dev)
    elif not (isinstance(inst_band, torch.Tensor) and inst_band.is_cuda and inst_band.device == dev and inst_band.dtype == torch.uint8
              and inst_band.dim() == 1 and inst_band.is_contiguous() and inst_band.numel() >= h * w):
        raise ValueError("mask_boundary_overlap: inst_band must be a flat contiguous uint8 GPU tensor of at least %d elements on %s" % (h * w, dev))
    bad = accumulator(bad, (1,), dev, "bad")
    inter_b = _i64_zeros((n, g), dev)
    band_pred = _i64_zeros((n,), dev)
    band_gt = _i64_zeros((g,), dev)
    with torch.cuda.device(dev):
        check(lib.irn_mask_boundary_overlap(m.data_ptr() if n else None, n, inst.data_ptr(), inst_band.data_ptr(), g, h, w, d,
                                            inter_b.data_ptr() if n and g else None, band_pred.data_ptr() if n else None,
                                            band_gt.data_ptr() if g else None, bad.data_ptr(), _stream()))
    return inter_b, band_pred, band_gt
