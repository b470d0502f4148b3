"""Host side of irn_amd/csrc/crf.hip: the dense CRF (misc/imutils.py:156-170 crf_inference_label,
step/cam_to_ir_label.py:22-39 of the reference) over include/irn_hip.h's irn_crf_* entries.  `irn_amd.ops` re-exports the
functions.  GPU tensors in, GPU tensors out; no CPU fallback."""
import ctypes as C

import numpy as np
import torch

from ._lib import _need_cuda, _stream, check, lib

CRF_T, CRF_GT_PROB = 10, 0.7          # the reference's defaults (misc/imutils.py:156)
CRF_MAX_SWEEP = 16                    # IRN_CRF_MAX_SWEEP
CRF_SCORE_EPS = np.float32(1e-5)      # the clip of the score-seeded unary
_CRF_WS = {}                          # (device index, stream) -> grow-only workspace of the CRF entries


def _crf_workspace(device, nbytes):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _CRF_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        _CRF_WS.pop(key, None)
        ws = _CRF_WS[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return ws


def _crf_rgb(img, dev):
    rgb = torch.as_tensor(img, device=dev)
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError("crf: the image must be uint8 [H,W,3] (RGB), got %s %s" % (rgb.dtype, tuple(rgb.shape)))
    return rgb.contiguous()


def crf_filter(feat, values, return_lattice=False):
    """The permutohedral filter alone: `compute(values)` of densecrf's lattice over `feat`.

    feat: GPU fp32 [N,d] (d <= 5); values: GPU fp32 [N,C].  Returns fp32 [N,C]; with `return_lattice` also the vertex keys
    int32 [M,d] (ascending lexicographic order) and the blur neighbours int32 [d+1,M,2] (-1 = none).  Synchronises."""
    _need_cuda(feat, "feat")
    _need_cuda(values, "values")
    feat = feat.float().contiguous()
    values = values.float().contiguous()
    n, d = feat.shape
    c = values.shape[1]
    if values.shape[0] != n:
        raise ValueError("crf_filter: %d feature rows, %d value rows" % (n, values.shape[0]))
    dev = feat.device
    nbytes = int(lib.irn_crf_filter_workspace_bytes(n, d, c))
    if nbytes == 0:
        raise ValueError("crf_filter: unsupported size n=%d d=%d c=%d" % (n, d, c))
    out = torch.empty((n, c), dtype=torch.float32, device=dev)
    keys = nbr = None
    if return_lattice:
        keys = torch.empty((n * (d + 1), d), dtype=torch.int32, device=dev)
        nbr = torch.empty((d + 1) * n * (d + 1) * 2, dtype=torch.int32, device=dev)
    m = C.c_int32()
    with torch.cuda.device(dev):
        ws = _crf_workspace(dev, nbytes)
        check(lib.irn_crf_filter(feat.data_ptr(), n, d, values.data_ptr(), c, out.data_ptr(), C.byref(m),
                                 None if keys is None else keys.data_ptr(), None if nbr is None else nbr.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _stream()))
    if not return_lattice:
        return out
    m = int(m.value)
    return out, keys[:m], nbr[:(d + 1) * m * 2].view(d + 1, m, 2)


def crf_inference_label(img, labels, t=CRF_T, n_labels=21, gt_prob=CRF_GT_PROB, want_q=False):
    """misc/imutils.py:156-170 on the GPU.  img: uint8 [H,W,3] RGB (GPU tensor, or anything torch.as_tensor takes);
    labels: int [H,W] in [0, n_labels).  Returns the argmax labels int32 [H,W] (GPU), and with `want_q` also Q fp32
    [n_labels,H,W]."""
    dev = labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else torch.device("cuda", torch.cuda.current_device())
    rgb = _crf_rgb(img, dev)
    h, w = rgb.shape[:2]
    lab = torch.as_tensor(labels, device=dev).to(torch.int32).contiguous()
    if tuple(lab.shape) != (h, w):
        raise ValueError("crf_inference_label: labels %s for an image of %dx%d" % (tuple(lab.shape), h, w))
    nbytes = int(lib.irn_crf_workspace_bytes(h, w, int(n_labels)))
    if nbytes == 0:
        raise ValueError("crf_inference_label: unsupported size %dx%d with %d labels" % (h, w, n_labels))
    out = torch.empty((h, w), dtype=torch.int32, device=dev)
    q = torch.empty((int(n_labels), h, w), dtype=torch.float32, device=dev) if want_q else None
    with torch.cuda.device(dev):
        ws = _crf_workspace(dev, nbytes)
        check(lib.irn_crf_inference_label(rgb.data_ptr(), lab.data_ptr(), h, w, int(n_labels), int(t), float(gt_prob),
                                          None if q is None else q.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _stream()))
    return (out, q) if want_q else out


def crf_ir_label(img, high_res, keys, fg_thres, bg_thres, t=CRF_T, gt_prob=CRF_GT_PROB, out=None):
    """step/cam_to_ir_label.py:22-39 for one image: the fg- and bg-threshold seeds of `high_res` (GPU fp32 [K,H,W]), both
    CRFs over the image's shared lattices, `keys` (0-based class ids [K]) and the confident-label combination.  Returns
    uint8 [H,W] on the GPU: 0 background, class+1 foreground, 255 unsure."""
    _need_cuda(high_res, "high_res")
    dev = high_res.device
    rgb = _crf_rgb(img, dev)
    h, w = rgb.shape[:2]
    cams = high_res.float().contiguous()
    k = int(cams.shape[0]) if cams.dim() == 3 else 0
    if k and tuple(cams.shape[1:]) != (h, w):
        raise ValueError("crf_ir_label: high_res %s for an image of %dx%d" % (tuple(cams.shape), h, w))
    ks = torch.as_tensor(keys, device=dev).to(torch.int64).reshape(-1).contiguous()
    if ks.numel() != k:
        raise ValueError("crf_ir_label: %d keys for %d CAM planes" % (ks.numel(), k))
    if out is None:
        out = torch.empty((h, w), dtype=torch.uint8, device=dev)
    ws, nbytes = None, 0
    with torch.cuda.device(dev):
        if k:
            nbytes = int(lib.irn_crf_workspace_bytes(h, w, k + 1))
            if nbytes == 0:
                raise ValueError("crf_ir_label: unsupported size %dx%d with %d classes" % (h, w, k))
            ws = _crf_workspace(dev, nbytes)
        check(lib.irn_crf_ir_label(rgb.data_ptr(), cams.data_ptr() if k else None, ks.data_ptr() if k else None, k, h, w,
                                   float(fg_thres), float(bg_thres), int(t), float(gt_prob), out.data_ptr(),
                                   None if ws is None else ws.data_ptr(), nbytes, _stream()))
    return out


def crf_label_sweep(img, high_res, keys, thres, t=CRF_T, gt_prob=CRF_GT_PROB, out=None):
    """The CRF label maps of one image at every threshold of `thres` (1..CRF_MAX_SWEEP values; cast to float32, strictly
    ascending after the cast): plane i is the CRF seeded with argmax([thres[i], high_res]) taken through `keys`, 0 background
    and class+1 foreground — the map `crf_ir_label` computes for that threshold as fg or as bg threshold, bit for bit.  The
    image's lattices are built once and the CRFs run in chunks of one filter each (include/irn_hip.h).  Returns uint8 [T,H,W]
    on the GPU; `ir_label_confusion` counts a threshold grid from it."""
    _need_cuda(high_res, "high_res")
    dev = high_res.device
    rgb = _crf_rgb(img, dev)
    h, w = rgb.shape[:2]
    cams = high_res.float().contiguous()
    k = int(cams.shape[0]) if cams.dim() == 3 else 0
    if k and tuple(cams.shape[1:]) != (h, w):
        raise ValueError("crf_label_sweep: high_res %s for an image of %dx%d" % (tuple(cams.shape), h, w))
    ks = torch.as_tensor(keys, device=dev).to(torch.int64).reshape(-1).contiguous()
    if ks.numel() != k:
        raise ValueError("crf_label_sweep: %d keys for %d CAM planes" % (ks.numel(), k))
    th = np.ascontiguousarray(np.asarray(thres, np.float32).reshape(-1))
    n_t = int(th.size)
    if not 1 <= n_t <= CRF_MAX_SWEEP or np.isnan(th).any() or (np.diff(th) <= 0).any():
        raise ValueError("crf_label_sweep: 1..%d strictly ascending float32 thresholds, got %s" % (CRF_MAX_SWEEP, th))
    if out is None:
        out = torch.empty((n_t, h, w), dtype=torch.uint8, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.uint8 and out.is_contiguous()
              and tuple(out.shape) == (n_t, h, w)):
        raise ValueError("crf_label_sweep: out must be a contiguous uint8 %s tensor on %s" % ((n_t, h, w), dev))
    ws, nbytes = None, 0
    with torch.cuda.device(dev):
        if k:
            nbytes = int(lib.irn_crf_sweep_workspace_bytes(h, w, k + 1, n_t))
            if nbytes == 0:
                raise ValueError("crf_label_sweep: unsupported size %dx%d with %d classes" % (h, w, k))
            ws = _crf_workspace(dev, nbytes)
        check(lib.irn_crf_label_sweep(rgb.data_ptr(), cams.data_ptr() if k else None, ks.data_ptr() if k else None, k, h, w,
                                      th.ctypes.data_as(C.POINTER(C.c_float)), n_t, int(t), float(gt_prob), out.data_ptr(),
                                      None if ws is None else ws.data_ptr(), nbytes, _stream()))
    return out


def crf_score_sweep(img, scores, keys, thres, t=CRF_T, out=None, want_q=False):
    """The dense CRF seeded with scores instead of labels, for one image at every background threshold of
    `thres` (1..CRF_MAX_SWEEP values; cast to float32, strictly ascending after the cast, each >= CRF_SCORE_EPS): CRF i has
    the labels [background, scores...] with -U = log(max([thres[i], scores], 1e-5)).  `scores`: GPU fp32 [C,H,W], the
    `rw_up` of `label_epilogue`; `keys`: the 0-based class ids [C].  Plane i of the result, uint8 [T,H,W] on the GPU (`out`
    when given), is the first maximum of Q through the keys: 0 background, key+1 otherwise — at t = 0 the label map of
    `label_epilogue` at that threshold.  The lattices are built once per call.  With `want_q` also Q fp32 [T,C+1,H,W]."""
    _need_cuda(scores, "scores")
    dev = scores.device
    rgb = _crf_rgb(img, dev)
    h, w = rgb.shape[:2]
    sc = scores.float().contiguous()
    c = int(sc.shape[0]) if sc.dim() == 3 else 0
    if sc.dim() != 3 or tuple(sc.shape[1:]) != (h, w):
        raise ValueError("crf_score_sweep: scores %s for an image of %dx%d (fp32 [C,H,W])" % (tuple(sc.shape), h, w))
    ks = torch.as_tensor(keys, device=dev).to(torch.int64).reshape(-1).contiguous()
    if ks.numel() != c:
        raise ValueError("crf_score_sweep: %d keys for %d score planes" % (ks.numel(), c))
    th = np.ascontiguousarray(np.asarray(thres, np.float32).reshape(-1))
    n_t = int(th.size)
    if not 1 <= n_t <= CRF_MAX_SWEEP or np.isnan(th).any() or (np.diff(th) <= 0).any() or (th < CRF_SCORE_EPS).any():
        raise ValueError("crf_score_sweep: 1..%d strictly ascending float32 thresholds of at least %g, got %s"
                         % (CRF_MAX_SWEEP, CRF_SCORE_EPS, th))
    if int(t) < 0:
        raise ValueError("crf_score_sweep: t = %d iterations" % int(t))
    if out is None:
        out = torch.empty((n_t, h, w), dtype=torch.uint8, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.uint8 and out.is_contiguous()
              and tuple(out.shape) == (n_t, h, w)):
        raise ValueError("crf_score_sweep: out must be a contiguous uint8 %s tensor on %s" % ((n_t, h, w), dev))
    ws, nbytes = None, 0
    with torch.cuda.device(dev):
        if c:
            nbytes = int(lib.irn_crf_score_sweep_workspace_bytes(h, w, c + 1, n_t))
            if nbytes == 0:
                raise ValueError("crf_score_sweep: unsupported size %dx%d with %d classes (at most %d)" % (h, w, c, 31))
            ws = _crf_workspace(dev, nbytes)
        q = torch.empty((n_t, c + 1, h, w), dtype=torch.float32, device=dev) if want_q else None
        check(lib.irn_crf_score_sweep(rgb.data_ptr(), sc.data_ptr() if c else None, ks.data_ptr() if c else None, c, h, w,
                                      th.ctypes.data_as(C.POINTER(C.c_float)), n_t, int(t), out.data_ptr(),
                                      None if q is None else q.data_ptr(), None if ws is None else ws.data_ptr(), nbytes,
                                      _stream()))
    return (out, q) if want_q else out


def crf_prob(img, prob, t=CRF_T, want_q=False):
    """The dense CRF seeded with probabilities (irn_crf_prob): -U = log(max(prob, 1e-5)), the pairwise terms,
    iterations and softmax of `crf_score_sweep`.  `img`: uint8 [H,W,3] RGB as for `crf_score_sweep`; `prob`: GPU fp32
    [L,H,W], 2 <= L <= 32 (the `prob` of `seg_fuse`).  Returns uint8 [H,W] on the GPU, the first maximum of Q as the label index
    itself — at t = 0 the arg-max of the clipped `prob` — and with `want_q` also Q fp32 [L,H,W]."""
    _need_cuda(prob, "crf_prob: prob")
    dev = prob.device
    rgb = _crf_rgb(img, dev)
    h, w = rgb.shape[:2]
    if prob.dtype != torch.float32 or prob.dim() != 3 or tuple(prob.shape[1:]) != (h, w):
        raise ValueError("crf_prob: prob %s %s for an image of %dx%d (fp32 [L,H,W])" % (prob.dtype, tuple(prob.shape), h, w))
    l = int(prob.shape[0])
    if int(t) < 0:
        raise ValueError("crf_prob: t = %d iterations" % int(t))
    nbytes = int(lib.irn_crf_prob_workspace_bytes(h, w, l))
    if nbytes == 0:
        raise ValueError("crf_prob: unsupported size %dx%d with %d labels (2..32)" % (h, w, l))
    pr = prob.contiguous()
    out = torch.empty((h, w), dtype=torch.uint8, device=dev)
    q = torch.empty((l, h, w), dtype=torch.float32, device=dev) if want_q else None
    with torch.cuda.device(dev):
        ws = _crf_workspace(dev, nbytes)
        check(lib.irn_crf_prob(rgb.data_ptr(), pr.data_ptr(), l, h, w, int(t), out.data_ptr(), None if q is None else q.data_ptr(),
                               ws.data_ptr(), ws.numel(), _stream()))
    return (out, q) if want_q else out
