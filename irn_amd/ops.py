"""Host-side wrappers of the kernels in libirn_hip.so outside the walk: label epilogue, CAM merge, the trunk's elementwise
passes (bn_act_, its differentiable form bn_act, stem_pool, upsample_bilinear), image resizing and the instance front end.  The hipBLASLt convolutions of the
trunk live in `irn_amd.gemm`; their functions are reachable from here too.

Reference functions mirrored (names kept where the reference has one):
    find_centroids_with_refinement(displacement, iterations=300)   step/make_ins_seg_labels.py:18-56
    cluster_centroids(centroids, displacement, thres=2.5)          step/make_ins_seg_labels.py:58-75
    label4(mask)                = skimage.measure.label(mask, connectivity=1, background=0)  (:66,:92)
    label_epilogue(...)         = step/make_sem_seg_labels.py:43-49, step/make_ins_seg_labels.py:137-145
    detect_instance(...)        = step/make_ins_seg_labels.py:82-105
    bicubic_resize(img, size)   = misc/imutils.py:8-17 pil_resize(img, size, order=3)
    msf_pack(img, scales)       = voc12/dataloader.py:191-201 (rescale, normalise, CHW, flip pair)
    augment_batch(images, ...)  = voc12/dataloader.py:129-156 for a batch (resize_long, normalise, mirror, crop, CHW)
    augment_pair_batch(images, labels, ...) = voc12/dataloader.py:251-267 for a batch (the image as above, the IR label
                                  nearest-rescaled, mirrored, cropped into 255 and reduced)
GPU tensors in, GPU tensors out; no CPU fallback.
"""
import collections
import ctypes as C

import numpy as np
import torch

from ._lib import _need_cuda, _need_vec, _stream, check, i32_array, lib, ptr_array
from .gemm import (conv1x1_algo_count, conv1x1_nhwc, conv3x3_split, gemm16_algo_count, gemm16_nhwc, gemm_ranks, gemm_ranks16,  # noqa: F401
                   gemm_ranks3x3, split16, split16_pad, split_overflowed, split_weight, split_weight_3x3)


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


def bn_act_(x, scale, shift, residual=None, relu=True, residual_affine=None):
    """Inference batch norm (+ residual) (+ ReLU) in one pass, IN PLACE on a convolution's output (irn_bn_act):
    ``x = act(x * scale[c] + shift[c] (+ r))`` — the elementwise tail of reference net/resnet50.py:34-54.  ``r`` is the
    residual, or ``residual * rs[c] + rb[c]`` with ``residual_affine = (rs, rb)`` (the projection shortcut's batch norm).
    x, residual: GPU fp32 [N, C, ...] contiguous; scale, shift, rs, rb: GPU fp32 [C].  Returns x."""
    _need_cuda(x, "x")
    nhwc = x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
    if x.dtype != torch.float32 or not (x.is_contiguous() or nhwc) or x.dim() < 2:
        raise ValueError("bn_act_: x must be a contiguous (or channels-last) fp32 [N, C, ...] tensor, got %s %s" % (x.dtype, tuple(x.shape)))
    n_ch = int(x.shape[1])
    if nhwc and n_ch % 4:
        raise ValueError("bn_act_: a channels-last tensor needs a multiple of 4 channels, got %d" % n_ch)
    consts = [("scale", scale), ("shift", shift)]
    if residual_affine is not None:
        if residual is None:
            raise ValueError("bn_act_: residual_affine without a residual")
        consts += [("residual scale", residual_affine[0]), ("residual shift", residual_affine[1])]
    for name, t in consts:
        _need_vec(t, "bn_act_: " + name, n_ch, x.device)
    if residual is not None and (residual.shape != x.shape or residual.dtype != torch.float32 or residual.device != x.device
                                 or not (residual.is_contiguous(memory_format=torch.channels_last) if nhwc else residual.is_contiguous())):
        raise ValueError("bn_act_: residual must match x (shape %s, fp32, same memory format, same device)" % (tuple(x.shape),))
    n_img = int(x.shape[0])
    if nhwc:
        rs, rb = (None, None) if residual_affine is None else (residual_affine[0].data_ptr(), residual_affine[1].data_ptr())
        px = int(x.shape[2]) * int(x.shape[3])
        per = max(1, (2 ** 31 - 1) // max(1, n_ch * px))
        with torch.cuda.device(x.device):
            for i in range(0, n_img, per):
                xi = x[i:i + per]
                ri = None if residual is None else residual[i:i + per]
                check(lib.irn_bn_act_nhwc(xi.data_ptr(), None if ri is None else ri.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                          rs, rb, int(xi.shape[0]) * px, n_ch, 1 if relu else 0, _stream()))
        return x
    plane = x[0, 0].numel() if n_img else 0
    rs, rb = (None, None) if residual_affine is None else (residual_affine[0].data_ptr(), residual_affine[1].data_ptr())
    # the entry point takes at most 2^31 - 1 elements: larger batches go image group by image group
    per = max(1, (2 ** 31 - 1) // max(1, n_ch * plane))
    with torch.cuda.device(x.device):
        for i in range(0, n_img, per):
            xi = x[i:i + per]
            ri = None if residual is None else residual[i:i + per]
            check(lib.irn_bn_act(xi.data_ptr(), None if ri is None else ri.data_ptr(), scale.data_ptr(), shift.data_ptr(), rs, rb,
                                 int(xi.shape[0]), n_ch, plane, 1 if relu else 0, _stream()))
    return x


def bn_fold(weight, bias, running_mean, running_var, eps):
    """(scale, shift) fp32 [C] of an inference batch norm in ONE launch (irn_bn_fold): bit for bit
    `FrozenBatchNorm._fold64()` rounded to fp32.  For the training seam, where the optimiser writes the parameters every step
    and the cached `folded()` would refold every layer with a dozen small kernels."""
    _need_cuda(weight, "bn_fold: weight")
    n_ch = int(weight.numel())
    ts = [t.detach() for t in (weight, bias, running_mean, running_var)]
    for name, t in zip(("weight", "bias", "running_mean", "running_var"), ts):
        _need_vec(t, "bn_fold: " + name, n_ch, weight.device)
    out = torch.empty((2, n_ch), dtype=torch.float32, device=weight.device)
    if n_ch:
        with torch.cuda.device(weight.device):
            check(lib.irn_bn_fold(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), float(eps), n_ch,
                                  out[0].data_ptr(), out[1].data_ptr(), _stream()))
    return out[0], out[1]


def bn_param_grads(s0, s1, running_mean, running_var, eps):
    """(grad_weight, grad_bias) fp32 [C] of an inference batch norm y = (x - mean) / sqrt(var + eps) * weight + bias from the
    channel sums S0 = sum dz and S1 = sum dz * x of the gradient dz that arrives at y (fp64 [C], `irn_bn_act_backward`):
    grad_weight = (S1 - mean * S0) / sqrt(var + eps), grad_bias = S0, in double, rounded once.  Plain tensor arithmetic:
    works on any device."""
    mean, var = running_mean.detach().double(), running_var.detach().double()
    return ((s1 - mean * s0) / torch.sqrt(var + eps)).float(), s0.float()


def _bn_act_backward(grad_out, out, x, res, scale, res_scale, relu, want_x, want_res, want_sums):
    """irn_bn_act_backward: (grad_x, grad_res, sums) with None for what was not asked for; sums fp64 [2 or 3, C]."""
    n_img, n_ch = int(grad_out.shape[0]), int(grad_out.shape[1])
    plane = grad_out[0, 0].numel() if n_img else 0
    dev = grad_out.device
    grad_x = torch.empty_like(grad_out) if want_x else None
    grad_res = torch.empty_like(grad_out) if want_res else None
    sums = ws = None
    ws_bytes = 0
    if want_sums:
        sums = torch.empty((3 if res_scale is not None else 2, n_ch), dtype=torch.float64, device=dev)
        ws_bytes = int(lib.irn_bn_act_backward_workspace_bytes(n_img, n_ch, plane))
        ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        check(lib.irn_bn_act_backward(grad_out.data_ptr(), ptr(out) if relu else None, ptr(x) if want_sums else None,
                                      ptr(res) if (want_sums and res_scale is not None) else None, ptr(scale) if want_x else None,
                                      ptr(res_scale), ptr(grad_x), ptr(grad_res), ptr(sums), n_img, n_ch, plane, 1 if relu else 0,
                                      ptr(ws), ws_bytes, _stream()))
    return grad_x, grad_res, sums


class _BnAct(torch.autograd.Function):
    """irn_bn_fold + irn_bn_act_forward with irn_bn_act_backward as the vector-Jacobian product; x is saved for the weight
    gradient, the output for the ReLU mask, the residual when it has a batch norm of its own."""

    @staticmethod
    def forward(ctx, x, weight, bias, mean, var, residual, r_weight, r_bias, r_mean, r_var, eps, r_eps, relu):
        scale, shift = bn_fold(weight, bias, mean, var, eps)
        res_bn = r_weight is not None
        rs, rb = bn_fold(r_weight, r_bias, r_mean, r_var, r_eps) if res_bn else (None, None)
        out = torch.empty_like(x)
        n_img = int(x.shape[0])
        if x.numel():
            with torch.cuda.device(x.device):
                check(lib.irn_bn_act_forward(x.data_ptr(), None if residual is None else residual.data_ptr(), scale.data_ptr(),
                                             shift.data_ptr(), None if rs is None else rs.data_ptr(), None if rb is None else rb.data_ptr(),
                                             out.data_ptr(), n_img, int(x.shape[1]), x[0, 0].numel(), 1 if relu else 0, _stream()))
        ctx.relu, ctx.res_bn, ctx.has_res, ctx.eps, ctx.r_eps = relu, res_bn, residual is not None, eps, r_eps
        ctx.save_for_backward(x, out if relu else None, residual if res_bn else None, scale, rs, mean, var, r_mean, r_var)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, out, residual, scale, rs, mean, var, r_mean, r_var = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_x, want_res = need[0], ctx.has_res and need[5]
        want_sums = need[1] or need[2] or (ctx.res_bn and (need[6] or need[7]))
        grads = [None] * 13
        if not (want_x or want_res or want_sums):
            return tuple(grads)
        grad_out = grad_out.contiguous().float()
        if grad_out.data_ptr() % 16:
            grad_out = grad_out.clone()
        if grad_out.numel() == 0:
            gx, gr, sums = (torch.zeros_like(x) if want_x else None, torch.zeros_like(x) if want_res else None,
                            torch.zeros((3 if ctx.res_bn else 2, x.shape[1]), dtype=torch.float64, device=x.device))
        else:
            gx, gr, sums = _bn_act_backward(grad_out, out, x, residual, scale, rs, ctx.relu, want_x, want_res, want_sums)
        grads[0], grads[5] = gx, gr
        if need[1] or need[2]:
            gw, gb = bn_param_grads(sums[0], sums[1], mean, var, ctx.eps)
            grads[1], grads[2] = (gw if need[1] else None), (gb if need[2] else None)
        if ctx.res_bn and (need[6] or need[7]):
            gw, gb = bn_param_grads(sums[0], sums[2], r_mean, r_var, ctx.r_eps)
            grads[6], grads[7] = (gw if need[6] else None), (gb if need[7] else None)
        return tuple(grads)


def bn_act(x, weight, bias, running_mean, running_var, eps, residual=None, relu=True, residual_bn=None):
    """Inference-statistics batch norm (+ residual) (+ ReLU) as ONE differentiable pass out of place — the training form of
    `bn_act_`, the elementwise tail of reference net/resnet50.py:34-54 under autograd:
    ``out = act((x - mean) / sqrt(var + eps) * weight + bias (+ r))``, r = residual or, with ``residual_bn`` (a batch-norm
    module, or a tuple (weight, bias, running_mean, running_var, eps): the projection shortcut's), that layer applied to the
    residual.  Differentiable once in x, residual and the two layers' weight and bias (irn_bn_act_backward; no atomics, the
    same bits every time); the forward equals `bn_act_` on the folded constants bit for bit.  x, residual: GPU fp32
    [N, C, ...] contiguous and 16-byte aligned, fewer than 2^31 elements; the parameters GPU fp32 [C]."""
    _need_cuda(x, "bn_act: x")
    if x.dtype != torch.float32 or x.dim() < 2 or not x.is_contiguous() or x.data_ptr() % 16 or x.numel() >= 2 ** 31:
        raise ValueError("bn_act: x must be a contiguous, 16-byte aligned fp32 [N, C, ...] tensor of fewer than 2^31 elements, got %s %s"
                         % (x.dtype, tuple(x.shape)))
    n_ch = int(x.shape[1])
    if residual is not None and (not isinstance(residual, torch.Tensor) or residual.shape != x.shape or residual.dtype != torch.float32
                                 or residual.device != x.device or not residual.is_contiguous() or residual.data_ptr() % 16):
        raise ValueError("bn_act: residual must match x (shape %s, fp32, contiguous, 16-byte aligned, same device)" % (tuple(x.shape),))
    r = (None,) * 5
    if residual_bn is not None:
        if residual is None:
            raise ValueError("bn_act: residual_bn without a residual")
        r = tuple(residual_bn) if isinstance(residual_bn, (tuple, list)) else (
            residual_bn.weight, residual_bn.bias, residual_bn.running_mean, residual_bn.running_var, residual_bn.eps)
        if len(r) != 5:
            raise ValueError("bn_act: residual_bn is a module or (weight, bias, running_mean, running_var, eps)")
    names = ("weight", "bias", "running_mean", "running_var")
    for name, t in list(zip(names, (weight, bias, running_mean, running_var))) + (
            [("residual " + n, t) for n, t in zip(names, r[:4])] if residual_bn is not None else []):
        if not isinstance(t, torch.Tensor):
            raise ValueError("bn_act: %s must be a tensor" % name)
        _need_vec(t, "bn_act: " + name, n_ch, x.device)
    return _BnAct.apply(x, weight, bias, running_mean, running_var, residual, r[0], r[1], r[2], r[3], float(eps),
                        None if r[4] is None else float(r[4]), bool(relu))


def _need_f32_contig(t, what, min_dim):
    _need_cuda(t, what)
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < min_dim:
        raise ValueError("%s must be a contiguous fp32 tensor of >= %d dimensions, got %s %s" % (what, min_dim, t.dtype, tuple(t.shape)))


def stem_pool(x, scale, shift):
    """Batch norm + ReLU + 3x3 / stride 2 / pad 1 max pool of the trunk's stem in one pass (irn_stem_pool; reference
    net/resnet50.py:94-97).  x: GPU fp32 [N, C, H, W] (conv1's output, left untouched) -> [N, C, (H-1)//2+1, (W-1)//2+1]."""
    _need_f32_contig(x, "stem_pool: x", 4)
    n, c, h, w = (int(v) for v in x.shape)
    _need_vec(scale, "stem_pool: scale", c, x.device)
    _need_vec(shift, "stem_pool: shift", c, x.device)
    out = torch.empty((n, c, (h - 1) // 2 + 1 if h else 0, (w - 1) // 2 + 1 if w else 0), dtype=torch.float32, device=x.device)
    if out.numel():
        with torch.cuda.device(x.device):
            check(lib.irn_stem_pool(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), n, c, h, w, out.data_ptr(), _stream()))
    return out


def _upsample_bilinear_backward(grad_out, out, factor, relu):
    """irn_upsample_bilinear_backward: the exact adjoint as a gather (no atomics, bit-reproducible).  grad_out: GPU fp32
    [..., h*factor, w*factor]; out: the forward's output (the ReLU mask) or None -> [..., h, w]."""
    ho, wo = int(grad_out.shape[-2]), int(grad_out.shape[-1])
    h, w = ho // factor, wo // factor
    grad_in = torch.empty(tuple(grad_out.shape[:-2]) + (h, w), dtype=torch.float32, device=grad_out.device)
    if grad_in.numel():
        with torch.cuda.device(grad_out.device):
            check(lib.irn_upsample_bilinear_backward(grad_out.data_ptr(), out.data_ptr() if relu else None, grad_out.numel() // (ho * wo),
                                                     h, w, factor, 1 if relu else 0, grad_in.data_ptr(), _stream()))
    return grad_in


class _UpsampleBilinear(torch.autograd.Function):
    """irn_upsample_bilinear with irn_upsample_bilinear_backward as its vector-Jacobian product; behind a ReLU the output is
    saved for the mask."""

    @staticmethod
    def forward(ctx, x, factor, relu):
        out = _upsample_bilinear_forward(x, factor, relu)
        ctx.factor, ctx.relu = factor, relu
        if relu:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        out = ctx.saved_tensors[0] if ctx.relu else None
        return _upsample_bilinear_backward(grad_out.contiguous().float(), out, ctx.factor, ctx.relu), None, None


def upsample_bilinear(x, factor, relu=False):
    """nn.Upsample(scale_factor=factor, mode='bilinear', align_corners=False) (+ ReLU) of the IRNet heads in one pass
    (irn_upsample_bilinear; reference net/resnet50_irn.py:36-48, :72-84).  x: GPU fp32 [..., h, w] -> [..., h*factor, w*factor].
    Differentiable w.r.t. ``x``: under autograd the same forward runs inside an autograd function whose backward is a gather
    without atomics (irn_upsample_bilinear_backward)."""
    _need_f32_contig(x, "upsample_bilinear: x", 2)
    if int(factor) != factor or not 1 <= factor <= 64:
        raise ValueError("upsample_bilinear: integer factor in 1..64 expected, got %r" % (factor,))
    factor = int(factor)
    if x.requires_grad and torch.is_grad_enabled():
        return _UpsampleBilinear.apply(x, factor, bool(relu))
    return _upsample_bilinear_forward(x, factor, relu)


def _upsample_bilinear_forward(x, factor, relu):
    h, w = int(x.shape[-2]), int(x.shape[-1])
    out = torch.empty(tuple(x.shape[:-2]) + (h * factor, w * factor), dtype=torch.float32, device=x.device)
    if out.numel():
        with torch.cuda.device(x.device):
            check(lib.irn_upsample_bilinear(x.data_ptr(), x.numel() // (h * w), h, w, factor, 1 if relu else 0, out.data_ptr(),
                                            _stream()))
    return out


_LUTS = {}


def rescale_size(h, w, scale):
    """misc/imutils.py:19-22: target size of pil_rescale (np.round: half to even)."""
    return int(np.round(h * scale)), int(np.round(w * scale))


def bicubic_plan(in_size, out_size):
    """Host-only: Pillow's fixed-point bicubic tap table of one axis -> (lo [out], count [out], weights [out, ksize])."""
    ks = C.c_int32()
    check(lib.irn_bicubic_plan(int(in_size), int(out_size), C.byref(ks), None, None, None, 0))
    lo = np.empty(out_size, np.int32)
    cnt = np.empty(out_size, np.int32)
    k = np.empty((out_size, ks.value), np.int32)
    as_p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    check(lib.irn_bicubic_plan(int(in_size), int(out_size), C.byref(ks), as_p(lo), as_p(cnt), as_p(k), k.size))
    return lo, cnt, k


def bicubic_resize(img, size):
    """GPU uint8 [H,W,C] (C in 1,3,4) or [H,W] -> GPU uint8 resized to size=(h,w); bit-identical to
    np.asarray(Image.fromarray(img).resize(size[::-1], Image.BICUBIC)) (misc/imutils.py:8-17)."""
    _need_cuda(img, "img")
    if img.dtype != torch.uint8:
        raise ValueError("bicubic_resize: uint8 image expected (Pillow's 8-bit path)")
    squeeze = img.dim() == 2
    src = (img[..., None] if squeeze else img).contiguous()
    h, w, ch = src.shape
    hs, ws = int(size[0]), int(size[1])
    if (hs, ws) == (h, w):
        return img
    out = torch.empty((hs, ws, ch), dtype=torch.uint8, device=src.device)
    scratch = torch.empty(max(lib.irn_bicubic_scratch_bytes(h, w, hs, ws, ch), 1), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        check(lib.irn_bicubic_resize_u8(src.data_ptr(), h, w, ch, hs, ws, out.data_ptr(), scratch.data_ptr(), _stream()))
    return out[..., 0] if squeeze else out


def normalize_lut(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """fp32 [3,256]: TorchvisionNormalize (voc12/dataloader.py:65-78) of every byte value, computed in float64
    and stored as float32 exactly like the reference's `proc_img[..., c] = (imgarr[..., c] / 255. - mean) / std`."""
    v = np.arange(256, dtype=np.uint8)
    return np.stack([((v / 255. - mean[c]) / std[c]).astype(np.float32) for c in range(3)])


def msf_pack(img, scales, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """GPU uint8 [H,W,3] -> list over scales of GPU fp32 [2,3,Hs,Ws]: the `img` entry of a
    VOC12ClassificationDatasetMSF item (voc12/dataloader.py:191-201), bit-identical to the PIL/numpy path."""
    _need_cuda(img, "img")
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("msf_pack: uint8 [H,W,3] image expected")
    src = img.contiguous()
    dev = src.device
    h, w = int(src.shape[0]), int(src.shape[1])
    sizes = [(h, w) if s == 1 else rescale_size(h, w, s) for s in scales]
    lut = _lut(mean, std, dev)
    outs = [torch.empty((2, 3, hs, ws), dtype=torch.float32, device=dev) for hs, ws in sizes]
    nbytes = max([lib.irn_bicubic_scratch_bytes(h, w, hs, ws, 3) for hs, ws in sizes] + [1])
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.irn_msf_pack(src.data_ptr(), h, w, len(sizes), i32_array([s[0] for s in sizes]),
                               i32_array([s[1] for s in sizes]), lut.data_ptr(), ptr_array([o.data_ptr() for o in outs]),
                               scratch.data_ptr(), _stream()))
    return outs


def _lut(mean, std, dev):
    key = ("msf_lut", tuple(mean), tuple(std), str(dev))
    lut = _LUTS.get(key)
    if lut is None:
        lut = _LUTS[key] = torch.from_numpy(normalize_lut(mean, std)).to(dev).contiguous()
    return lut


AUGMENT_DESC_WORDS = 16               # IRN_AUGMENT_DESC_WORDS
AugmentTables = collections.namedtuple("AugmentTables", "meta src_offsets pixels_bytes scratch_bytes")
_PLANS = {}


def _plan(in_size, out_size):
    """`bicubic_plan`, kept per size pair (read-only: a training epoch meets a few hundred of them again and again)."""
    key = (int(in_size), int(out_size))
    if key not in _PLANS:
        if len(_PLANS) >= 8192:
            _PLANS.clear()
        _PLANS[key] = bicubic_plan(*key)
    return _PLANS[key]


def augment_tables(sizes, params, crop):
    """Host-only: the descriptors and tap tables `irn_augment_batch` takes (include/irn_hip.h), for images of `sizes[i]` =
    (h, w) and the draws `params[i]` = (hs, ws, flip, box): the image resized to hs x ws (`rescale_size`), mirrored when
    `flip`, then `box` = (c_top, c_left, i_top, i_left, rows, cols) of `imutils._crop_box` applied to that.  The X table of
    an image holds, for column j of its box, the full-axis plan row of resized column i_left + j (ws - 1 - (i_left + j) when
    mirrored); the Y table the rows i_top .. i_top + rows - 1 with `lo` counted from r0, the first source row any of them
    reads.  -> AugmentTables(meta int32 [words], byte offset of every image in the packed pixel buffer, its size, the
    scratch size)."""
    n = len(sizes)
    crop = int(crop)
    desc = np.zeros((n, AUGMENT_DESC_WORDS), np.int32)
    tabs, src_offsets = [], []
    word, src, mid = n * AUGMENT_DESC_WORDS, 0, 0
    for i, ((h, w), (hs, ws, flip, box)) in enumerate(zip(sizes, params)):
        h, w, hs, ws = int(h), int(w), int(hs), int(ws)
        c_top, c_left, i_top, i_left, rows, cols = (int(v) for v in box)
        if (min(h, w, hs, ws, rows, cols) < 1 or min(c_top, c_left, i_top, i_left) < 0 or i_top + rows > hs or i_left + cols > ws
                or c_top + rows > crop or c_left + cols > crop):
            raise ValueError("augment_tables: image %d: box %s does not fit a %dx%d image in a %d^2 crop" % (i, tuple(box), hs, ws, crop))
        xlo, xcnt, xk = _plan(w, ws)
        ylo, ycnt, yk = _plan(h, hs)
        xs = np.arange(i_left, i_left + cols)
        if flip:
            xs = ws - 1 - xs
        ys = np.arange(i_top, i_top + rows)
        r0 = int(ylo[ys].min())
        r1 = int((ylo[ys] + ycnt[ys]).max())
        xt = np.concatenate([xlo[xs], xcnt[xs], xk[xs].reshape(-1)])
        yt = np.concatenate([ylo[ys] - r0, ycnt[ys], yk[ys].reshape(-1)])
        desc[i, :14] = (h, w, c_top, c_left, rows, cols, r0, r1 - r0, xk.shape[1], yk.shape[1], src, mid, word, word + xt.size)
        tabs += [xt, yt]
        src_offsets.append(src)
        word += xt.size + yt.size
        src += h * w * 3
        mid += (r1 - r0) * cols * 3
    if max(src, mid, word) >= 2 ** 31:
        raise ValueError("augment_tables: the batch's pixels, intermediates or tables exceed 2^31 - 1")
    meta = np.concatenate([desc.reshape(-1)] + tabs).astype(np.int32, copy=False) if n else np.zeros(0, np.int32)
    return AugmentTables(meta, src_offsets, src, mid)


AUGMENT_LABEL_DESC_WORDS = 12         # IRN_AUGMENT_LABEL_DESC_WORDS
LabelTables = collections.namedtuple("LabelTables", "meta src_offsets labels_bytes")
_NEAREST = {}


def nearest_plan(in_size, out_size):
    """Host-only: the source index Pillow's NEAREST reads for every cell of one axis resized in_size -> out_size, int32
    [out_size] (read-only, kept per size pair like `_plan`).  Pillow walks the axis in doubles: it starts at
    0.5 * in / out, adds in / out once per output cell and truncates each position — the running sum, not the textbook
    floor((x + 0.5) * in / out), which rounds differently in about one size pair out of five."""
    key = (int(in_size), int(out_size))
    tab = _NEAREST.get(key)
    if tab is None:
        if key[0] < 1 or key[1] < 1:
            raise ValueError("nearest_plan: sizes must be >= 1 (got %d -> %d)" % key)
        a = key[0] / key[1]
        steps = np.full(key[1], a, np.float64)
        steps[0] = 0.5 * a
        tab = np.cumsum(steps).astype(np.int64).astype(np.int32)           # (sequential double additions, as Pillow's loop)
        tab.setflags(write=False)
        if len(_NEAREST) >= 8192:
            _NEAREST.clear()
        _NEAREST[key] = tab
    return tab


def augment_label_tables(sizes, params, crop, reduce):
    """Host-only: the descriptors and index tables `irn_augment_label_batch` takes (include/irn_hip.h), for label maps of
    `sizes[i]` = (h, w) and the draws `params[i]` = (hs, ws, flip, box) as `augment_tables` takes them: the row table of an
    image holds `nearest_plan(h, hs)` for the rows i_top .. i_top + rows - 1 of its box, the column table
    `nearest_plan(w, ws)` for the columns i_left + j (ws - 1 - (i_left + j) when mirrored).  -> LabelTables(meta int32
    [words], byte offset of every map in the packed label buffer, its size)."""
    n = len(sizes)
    crop, reduce = int(crop), int(reduce)
    if reduce < 1 or crop % reduce:
        raise ValueError("augment_label_tables: reduce %d does not divide the crop %d" % (reduce, crop))
    desc = np.zeros((n, AUGMENT_LABEL_DESC_WORDS), np.int32)
    tabs, src_offsets = [], []
    word, src = n * AUGMENT_LABEL_DESC_WORDS, 0
    for i, ((h, w), (hs, ws, flip, box)) in enumerate(zip(sizes, params)):
        h, w, hs, ws = int(h), int(w), int(hs), int(ws)
        c_top, c_left, i_top, i_left, rows, cols = (int(v) for v in box)
        if (min(h, w, hs, ws, rows, cols) < 1 or min(c_top, c_left, i_top, i_left) < 0 or i_top + rows > hs or i_left + cols > ws
                or c_top + rows > crop or c_left + cols > crop):
            raise ValueError("augment_label_tables: image %d: box %s does not fit a %dx%d image in a %d^2 crop" % (i, tuple(box), hs, ws, crop))
        xs = np.arange(i_left, i_left + cols)
        if flip:
            xs = ws - 1 - xs
        rt = nearest_plan(h, hs)[i_top:i_top + rows]
        ct = nearest_plan(w, ws)[xs]
        desc[i, :9] = (h, w, c_top, c_left, rows, cols, src, word, word + rows)
        tabs += [rt, ct]
        src_offsets.append(src)
        word += rows + cols
        src += h * w
    if max(src, word) >= 2 ** 31:
        raise ValueError("augment_label_tables: the batch's labels or tables exceed 2^31 - 1")
    meta = np.concatenate([desc.reshape(-1)] + tabs).astype(np.int32, copy=False) if n else np.zeros(0, np.int32)
    return LabelTables(meta, src_offsets, src)


_AUG_STAGED = {}          # device -> event behind the last upload out of the page-locked staging buffers


def _augment_device(images, device):
    if device is None:
        on_dev = [im.device for im in images if im.is_cuda]
        device = on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _augment(images, labels, params, crop, reduce, mean, std, dev, out, out_label):
    """The body of `augment_batch` (labels None) and `augment_pair_batch`: the label maps ride behind the pixels in the
    same page-locked staging buffer and the same upload, their tables behind the image tables in the same meta buffer."""
    n = len(images)
    t = augment_tables([im.shape[:2] for im in images], params, crop)
    words = int(t.meta.size)
    lt = augment_label_tables([lb.shape for lb in labels], params, crop, reduce) if labels is not None else None
    lwords = int(lt.meta.size) if lt else 0
    lbytes = lt.labels_bytes if lt else 0
    if t.pixels_bytes + lbytes >= 2 ** 31:
        raise ValueError("augment: the batch's packed pixels and label maps exceed 2^31 - 1 bytes")
    sources = list(zip(images, t.src_offsets))
    if lt:
        sources += [(lb, t.pixels_bytes + off) for lb, off in zip(labels, lt.src_offsets)]
    with torch.cuda.device(dev):
        lut = _lut(mean, std, dev)
        pixels = torch.empty(t.pixels_bytes + lbytes, dtype=torch.uint8, device=dev)
        scratch = torch.empty(max(t.scratch_bytes, 1), dtype=torch.uint8, device=dev)
        meta_dev = torch.empty(words + lwords, dtype=torch.int32, device=dev)
        staged = _AUG_STAGED.get(str(dev))
        if staged is not None:
            staged.synchronize()                     # the staging buffers are free again once the last call's copies have run
        meta_host = _cached("aug_meta", "pinned", words + lwords, torch.int32)
        meta_host[:words].copy_(torch.from_numpy(t.meta))
        if lt:
            meta_host[words:words + lwords].copy_(torch.from_numpy(lt.meta))
        if all(not src.is_cuda for src, _ in sources):
            stage = _cached("aug_pixels", "pinned", pixels.numel(), torch.uint8)
            for src, off in sources:
                stage[off:off + src.numel()].copy_(src.reshape(-1))
            pixels.copy_(stage[:pixels.numel()], non_blocking=True)
        else:
            for src, off in sources:
                pixels[off:off + src.numel()].copy_(src.reshape(-1), non_blocking=True)
        meta_p = C.cast(meta_host.data_ptr(), C.POINTER(C.c_int32))
        check(lib.irn_augment_batch(n, crop, meta_p, words, pixels.data_ptr(), t.pixels_bytes, lut.data_ptr(), out.data_ptr(),
                                    out.numel(), scratch.data_ptr(), scratch.numel(), meta_dev.data_ptr(), words, _stream()))
        if lt:
            lmeta_p = C.cast(meta_host.data_ptr() + 4 * words, C.POINTER(C.c_int32))
            check(lib.irn_augment_label_batch(n, crop, reduce, lmeta_p, lwords, pixels.data_ptr() + t.pixels_bytes, lbytes,
                                              out_label.data_ptr(), out_label.numel(), meta_dev.data_ptr() + 4 * words, lwords,
                                              _stream()))
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        _AUG_STAGED[str(dev)] = done


def augment_batch(images, params, crop, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), device=None, out=None):
    """The CAM training step's input batch on the GPU (irn_augment_batch): `images` is a list of uint8 [H,W,3] tensors (on the
    host or the device, ragged), `params[i]` = (hs, ws, flip, box) the draws of image i as `augment_tables` takes them ->
    GPU fp32 [B,3,crop,crop], bit-identical to resize (PIL bicubic) -> TorchvisionNormalize -> fliplr -> box into zeros -> CHW
    per image.  Two launches per batch; host images are packed into one page-locked buffer that is reused across calls and
    cross in one non-blocking copy, the descriptors and tables in a second one.  `out`: a contiguous fp32 [B,3,crop,crop]
    GPU tensor to write into (every cell is written)."""
    n = len(images)
    for im in images:
        if not (isinstance(im, torch.Tensor) and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3):
            raise ValueError("augment_batch: uint8 [H,W,3] images expected")
    dev = _augment_device(images, device)
    crop = int(crop)
    if out is None:
        out = torch.empty((n, 3, crop, crop), dtype=torch.float32, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == dev and out.is_contiguous()
              and tuple(out.shape) == (n, 3, crop, crop)):
        raise ValueError("augment_batch: out must be a contiguous fp32 [%d,3,%d,%d] tensor on %s" % (n, crop, crop, dev))
    if n == 0:
        return out
    _augment(images, None, params, crop, 1, mean, std, dev, out, None)
    return out


def augment_pair_batch(images, labels, params, crop, reduce=4, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), device=None,
                       out=None, out_label=None):
    """The IRNet training step's (image, label) batch on the GPU: `images` as `augment_batch` takes them, `labels[i]` the uint8
    [H,W] IR label map of image i (same size), `params[i]` = (hs, ws, flip, box) the one set of draws both halves share ->
    (GPU fp32 [B,3,crop,crop], GPU uint8 [B,crop/reduce,crop/reduce]).  The image half is `augment_batch`; the label half
    (irn_augment_label_batch, one more launch) is bit-identical to Pillow NEAREST resize to hs x ws -> fliplr -> box into a
    container of 255 -> pil_rescale(label, 1 / reduce, 0) (voc12/dataloader.py:251-267 with reduce 4; reduce 1 is the whole
    cropped label).  Host pixels and labels cross in ONE upload out of the page-locked staging buffer.  `out` / `out_label`:
    contiguous GPU tensors of those shapes to write into (every cell is written)."""
    n = len(images)
    crop, reduce = int(crop), int(reduce)
    if reduce < 1 or crop % reduce:
        raise ValueError("augment_pair_batch: reduce %d does not divide the crop %d" % (reduce, crop))
    if len(labels) != n or len(params) != n:
        raise ValueError("augment_pair_batch: %d images, %d labels, %d draws" % (n, len(labels), len(params)))
    for im, lb in zip(images, labels):
        if not (isinstance(im, torch.Tensor) and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3):
            raise ValueError("augment_pair_batch: uint8 [H,W,3] images expected")
        if not (isinstance(lb, torch.Tensor) and lb.dtype == torch.uint8 and lb.dim() == 2):
            raise ValueError("augment_pair_batch: uint8 [H,W] label maps expected")
        if tuple(lb.shape) != tuple(im.shape[:2]):
            raise ValueError("augment_pair_batch: a %dx%d label map for a %dx%d image" % (tuple(lb.shape) + tuple(im.shape[:2])))
    dev = _augment_device(images, device)
    grid = crop // reduce
    if out is None:
        out = torch.empty((n, 3, crop, crop), dtype=torch.float32, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == dev and out.is_contiguous()
              and tuple(out.shape) == (n, 3, crop, crop)):
        raise ValueError("augment_pair_batch: out must be a contiguous fp32 [%d,3,%d,%d] tensor on %s" % (n, crop, crop, dev))
    if out_label is None:
        out_label = torch.empty((n, grid, grid), dtype=torch.uint8, device=dev)
    elif not (isinstance(out_label, torch.Tensor) and out_label.dtype == torch.uint8 and out_label.device == dev
              and out_label.is_contiguous() and tuple(out_label.shape) == (n, grid, grid)):
        raise ValueError("augment_pair_batch: out_label must be a contiguous uint8 [%d,%d,%d] tensor on %s" % (n, grid, grid, dev))
    if n:
        _augment(images, labels, params, crop, reduce, mean, std, dev, out, out_label)
    return out, out_label


def find_centroids_with_refinement(displacement, iterations=300):
    """dp GPU fp32 [2,h,w] -> GPU int32 [2,h,w] (cy, cx); bit-identical to the reference's numpy
    (step/make_ins_seg_labels.py:18-56)."""
    _need_cuda(displacement, "displacement")
    dp = displacement.contiguous().float()
    _, h, w = dp.shape
    out = torch.empty((2, h, w), dtype=torch.int32, device=dp.device)
    with torch.cuda.device(dp.device):
        check(lib.irn_find_centroids(dp.data_ptr(), h, w, int(iterations), out.data_ptr(), _stream()))
    return out


def cluster_centroids(centroids, displacement, thres=2.5, as_one_hot=False):
    """-> (cluster_map GPU int32 [h,w] with values 0..K-1, K).  With ``as_one_hot`` returns the
    reference's bool [K,h,w] instead (step/make_ins_seg_labels.py:58-75)."""
    _need_cuda(centroids, "centroids")
    dp = displacement.contiguous().float()
    cen = centroids.to(torch.int32).contiguous()
    _, h, w = dp.shape
    cmap = torch.empty((h, w), dtype=torch.int32, device=dp.device)
    scratch = torch.empty(lib.irn_cluster_scratch_bytes(h, w), dtype=torch.uint8, device=dp.device)
    k = C.c_int()
    with torch.cuda.device(dp.device):
        check(lib.irn_cluster_centroids(cen.data_ptr(), dp.data_ptr(), h, w, float(thres), cmap.data_ptr(),
                                        C.byref(k), scratch.data_ptr(), _stream()))
    if as_one_hot:
        return (cmap[None] == torch.arange(k.value, device=dp.device, dtype=torch.int32)[:, None, None])
    return cmap, k.value


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
    scratch = _cached("cluster_scratch", dev, lib.irn_cluster_batch_scratch_bytes(n, hs, ws), torch.uint8)
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
    libirn_hip.so (irn_detect_instance_count / _emit): one pass over the class map, one 4-byte sync
    for N, one transfer of the result.  Returns the reference's numpy dict {'score','mask','class'}
    in its order (channel ascending, component ascending by first pixel).  Raises ValueError when
    nothing is detected (the reference crashes in np.stack([]) — SURVEY.md §3.5)."""
    _need_cuda(rw_up, "rw_up")
    _need_cuda(argmax, "argmax")
    dev = rw_up.device
    sc = rw_up.contiguous().float()
    am = argmax.to(torch.int32).contiguous()
    n_channels = int(n_channels)
    h, w = am.shape
    if sc.shape != (n_channels, h, w):
        raise ValueError("rw_up must be [%d,%d,%d], got %s" % (n_channels, h, w, tuple(sc.shape)))
    class_ids = np.asarray(class_ids)
    npx = h * w
    scratch = _cached("det_scratch", dev, lib.irn_detect_scratch_bytes(n_channels, h, w), torch.uint8)
    n = C.c_int()
    with torch.cuda.device(dev):
        check(lib.irn_detect_instance_count(sc.data_ptr(), am.data_ptr(), n_channels, h, w, C.byref(n),
                                            scratch.data_ptr(), _stream()))
        nd = n.value
        if nd == 0:
            raise ValueError("detect_instance: no foreground pixel in any channel")
        # one packed device buffer [score fp32 | channel int32 | masks uint8] -> one transfer into pinned memory
        # (a pageable .cpu() of the masks plus fresh allocations cost 3.6 ms per 512^2 image: 10x the rest of the step)
        head = 8 * nd
        packed = _cached("det_out", dev, head + nd * npx, torch.uint8)
        base = packed.data_ptr()
        check(lib.irn_detect_instance_emit(sc.data_ptr(), am.data_ptr(), n_channels, h, w, nd, float(max_fragment_size),
                                           base, base + 4 * nd, base + head, scratch.data_ptr(), _stream()))
        host = _cached("det_host", "pinned", head + nd * npx, torch.uint8)
        host[:head + nd * npx].copy_(packed[:head + nd * npx], non_blocking=True)
        torch.cuda.current_stream().synchronize()
    raw = host.numpy()
    score = raw[:4 * nd].view(np.float32).copy()
    chan = raw[4 * nd:head].view(np.int32)
    mask = raw[head:head + nd * npx].view(np.bool_).reshape(nd, h, w).copy()
    return {"score": score, "mask": mask, "class": class_ids[chan]}


_NOTHING = "detect_instance: no foreground pixel in any channel"


class _PendingBatch:
    """Results of a batched detection whose last transfer to the host may still be in flight: `result()` waits for it once
    and returns the list the blocking call returns, an image without any detection holding its ValueError.  `host` is None
    when no image of the batch has one.  A subclass's `_unpack()` yields the results of the images that have detections,
    in order."""

    def __init__(self, nds, host, done, timings, t_emit):
        self._nds, self._host, self._done, self._timings, self._t_emit = nds, host, done, timings, t_emit
        self._out = None

    def result(self):
        if self._out is not None:
            return self._out
        import time
        if self._host is None:
            self._out = [ValueError(_NOTHING) for _ in self._nds]
            return self._out
        self._done.synchronize()                                                   # the batch's last host round trip
        t_done = time.perf_counter()
        found = self._unpack()
        self._out = [next(found) if nd else ValueError(_NOTHING) for nd in self._nds]
        if self._timings is not None:            # seconds: emit + transfer (as far as the caller waited for it), unpacking
            self._timings["emit_d2h"] = self._timings.get("emit_d2h", 0.0) + t_done - self._t_emit
            self._timings["unpack"] = self._timings.get("unpack", 0.0) + time.perf_counter() - t_done
        return self._out


class PendingDetections(_PendingBatch):
    """Detections of a batch whose packed transfer to the host may still be in flight (`detect_instance_batch(...,
    deferred=True)`): `result()` waits for it and returns the list `detect_instance_batch` returns.  The transfer runs on
    a copy stream of its own, so the caller can enqueue the next batch's kernels before collecting this one."""

    def __init__(self, nds, host, done, timings, t_emit, offs, hs, ws, class_ids):
        super().__init__(nds, host, done, timings, t_emit)
        self._offs, self._hs, self._ws, self._class_ids = offs, hs, ws, class_ids

    def _unpack(self):
        raw = self._host.numpy()
        for i, nd in enumerate(self._nds):
            if nd == 0:
                continue
            o_sc, o_ch, o_mk = self._offs[i]
            score = raw[o_sc:o_sc + 4 * nd].view(np.float32)
            chan = raw[o_ch:o_ch + 4 * nd].view(np.int32)
            mask = raw[o_mk:o_mk + nd * self._hs[i] * self._ws[i]].view(np.bool_).reshape(nd, self._hs[i], self._ws[i])
            yield {"score": score, "mask": mask, "class": np.asarray(self._class_ids[i])[chan]}


_COPY_STREAMS = {}


def _copy_stream(dev):
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
        stream = _copy_stream(src.device)
        stream.wait_event(ready)
        src.record_stream(stream)
    with torch.cuda.stream(stream):
        host[:src.numel()].copy_(src, non_blocking=True)
        done.record(stream)
    return done


class _DetCount(collections.namedtuple("_DetCount", "n dev hs ws cs_a hs_a ws_a sc_p am_p keep scratch nds")):
    """What the emit entries take after the labelling half of a batched detection: sizes (lists and int32 arrays), the input
    pointer arrays (`keep` holds the converted inputs alive), the detect scratch and the detection counts."""


def _detect_batch_count(rw_ups, argmaxes, n_channels):
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
    scratch = _cached("det_scratch_b", dev, lib.irn_detect_batch_scratch_bytes(n, cs_a, hs_a, ws_a), torch.uint8)
    n_det_dev = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.irn_detect_instance_batch_count(n, sc_p, am_p, cs_a, hs_a, ws_a, n_det_dev.data_ptr(),
                                                  scratch.data_ptr(), _stream()))
        nds = [int(v) for v in n_det_dev.cpu().tolist()]                       # host round trip 1
    return _DetCount(n, dev, hs, ws, cs_a, hs_a, ws_a, sc_p, am_p, (scs, ams), scratch, nds)


def detect_instance_batch(rw_ups, argmaxes, class_ids, n_channels, max_fragment_sizes, timings=None, deferred=False):
    """detect_instance for a batch of images with two host round trips in total (the per-image form has three per
    image): one 4-byte-per-image transfer of the detection counts, one packed transfer of every image's
    {score, channel, masks} (irn_detect_instance_batch_count / _emit).  Arguments are lists (one entry per image) of
    what `detect_instance` takes.  Returns a list with, per image, the reference's numpy dict or — for an image without
    any foreground pixel — the ValueError `detect_instance` would raise.  With `deferred=True` the packed transfer is
    left in flight on a copy stream and a `PendingDetections` is returned: call its `result()` after the next batch has
    been enqueued and the 2 MB of masks per image cross PCIe under that batch's kernels."""
    import time
    t_start = time.perf_counter()
    dc = _detect_batch_count(rw_ups, argmaxes, n_channels)
    n, nds = dc.n, dc.nds
    t_count = time.perf_counter()
    if timings is not None:          # seconds: labelling + count transfer
        timings["count"] = timings.get("count", 0.0) + t_count - t_start
    # packed output: per image [score fp32 x nd | channel int32 x nd | pad to 16 | masks uint8 nd x h x w | pad to 16]
    offs, total = [], 0
    for i in range(n):
        head = (8 * nds[i] + 15) // 16 * 16
        offs.append((total, total + 4 * nds[i], total + head))
        total += head + (nds[i] * dc.hs[i] * dc.ws[i] + 15) // 16 * 16
    host = done = None
    if total:
        with torch.cuda.device(dc.dev):
            # the device-side staging buffer: the cached one when the call waits for its transfer, one of the batch's own
            # when the transfer is left in flight (the next batch must not write into it)
            packed = (torch.empty(total + 16, dtype=torch.uint8, device=dc.dev) if deferred
                      else _cached("det_out_b", dc.dev, total + 16, torch.uint8))
            base = (packed.data_ptr() + 15) // 16 * 16
            shift = base - packed.data_ptr()
            live = [nd > 0 for nd in nds]
            check(lib.irn_detect_instance_batch_emit(
                n, dc.sc_p, dc.am_p, dc.cs_a, dc.hs_a, dc.ws_a, i32_array(nds),
                (C.c_double * n)(*[float(v) for v in max_fragment_sizes]),
                ptr_array([base + o[0] if l else None for o, l in zip(offs, live)]),
                ptr_array([base + o[1] if l else None for o, l in zip(offs, live)]),
                ptr_array([base + o[2] if l else None for o, l in zip(offs, live)]), dc.scratch.data_ptr(), _stream()))
            # a page-locked buffer of its own for every batch: the detections are handed out as VIEWS of it (no second copy
            # of 2 MB of masks per image) and it goes back to torch's caching host allocator when the last of them is dropped
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            done = read_back(packed[shift:shift + total], host, side=deferred)
        if timings is not None:
            timings["bytes"] = timings.get("bytes", 0) + total
    pending = PendingDetections(nds, host, done, timings, t_count, offs, dc.hs, dc.ws, class_ids)
    return pending if deferred else pending.result()


class PendingRleDetections(_PendingBatch):
    """`detect_instance_rle_batch(..., deferred=True)`: the run lengths of a batch may still be crossing to the host on the
    copy stream; `result()` waits for them and returns the list `detect_instance_rle_batch` returns."""

    def __init__(self, nds, host, done, timings, t_emit, head, hs, ws, class_ids):
        super().__init__(nds, host, done, timings, t_emit)
        self._head, self._hs, self._ws, self._class_ids = head, hs, ws, class_ids

    def _unpack(self):
        score, chan, area, n_runs, bbox = self._head
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
    import time
    t_start = time.perf_counter()
    dc = _detect_batch_count(rw_ups, argmaxes, n_channels)
    n, dev, nds = dc.n, dc.dev, dc.nds
    t_count = time.perf_counter()
    if timings is not None:
        timings["count"] = timings.get("count", 0.0) + t_count - t_start
    G = sum(nds)
    if G == 0:
        pending = PendingRleDetections(nds, None, None, timings, t_count, None, dc.hs, dc.ws, class_ids)
        return pending if deferred else pending.result()
    nd_a = i32_array(nds)
    with torch.cuda.device(dev):
        rle_scratch = _cached("det_rle_scratch", dev, lib.irn_detect_instance_batch_rle_scratch_bytes(n, dc.hs_a, dc.ws_a, nd_a),
                              torch.uint8)
        # score fp32 [G] | channel int32 [G] | area int32 [G] | n_runs int32 [G] | bbox int32 [G][4]
        head_dev = _cached("det_rle_head", dev, 32 * G, torch.uint8)
        base = head_dev.data_ptr()
        check(lib.irn_detect_instance_batch_rle_count(
            n, dc.sc_p, dc.am_p, dc.cs_a, dc.hs_a, dc.ws_a, nd_a, (C.c_double * n)(*[float(v) for v in max_fragment_sizes]),
            base, base + 4 * G, base + 8 * G, base + 12 * G, base + 16 * G, dc.scratch.data_ptr(), rle_scratch.data_ptr(),
            _stream()))
        head_host = torch.empty(32 * G, dtype=torch.uint8, pin_memory=True)
        read_back(head_dev[:32 * G], head_host, side=False).synchronize()          # host round trip 2
        raw = head_host.numpy()
        head = (raw[:4 * G].view(np.float32), raw[4 * G:8 * G].view(np.int32), raw[8 * G:12 * G].view(np.int32),
                raw[12 * G:16 * G].view(np.int32), raw[16 * G:].view(np.int32).reshape(G, 4))
        runs, g = [], 0
        for nd in nds:
            runs.append(int(head[3][g:g + nd].sum(dtype=np.int64)))
            g += nd
        total = sum(runs)
        ws_bytes = lib.irn_detect_instance_batch_rle_sort_bytes(total, G)
        if ws_bytes == 0:
            check(1)
        sort_ws = _cached("det_rle_sort", dev, ws_bytes, torch.uint8)
        counts_dev = (torch.empty(4 * total, dtype=torch.uint8, device=dev) if deferred
                      else _cached("det_rle_counts", dev, 4 * total, torch.uint8))
        check(lib.irn_detect_instance_batch_rle_emit(n, dc.hs_a, dc.ws_a, nd_a, (C.c_int64 * n)(*runs), counts_dev.data_ptr(),
                                                     rle_scratch.data_ptr(), sort_ws.data_ptr(), ws_bytes, _stream()))
        host = torch.empty(4 * total, dtype=torch.uint8, pin_memory=True)
        done = read_back(counts_dev[:4 * total], host, side=deferred)
    if timings is not None:
        timings["bytes"] = timings.get("bytes", 0) + 4 * n + 32 * G + 4 * total
    pending = PendingRleDetections(nds, host, done, timings, t_count, head, dc.hs, dc.ws, class_ids)
    return pending if deferred else pending.result()


class PendingOverlaps(_PendingBatch):
    """`detection_overlap_batch(..., deferred=True)`: the packed counts of a batch may still be crossing to the host on the
    copy stream; `result()` waits for them and returns the list `detection_overlap_batch` returns (an image without a
    detection has a record with N = 0, not an error)."""

    def __init__(self, nds, host, done, gs, class_ids):
        super().__init__(nds, host, done, None, 0.0)
        self._gs, self._class_ids = gs, class_ids

    def result(self):
        if self._out is not None:
            return self._out
        nds, gs = self._nds, self._gs
        G, NG, NI = sum(nds), sum(gs), sum(nd * g for nd, g in zip(nds, gs))
        raw = np.zeros(0, np.uint8)
        if self._host is not None:
            self._done.synchronize()                                               # the batch's last host round trip
            raw = self._host.numpy().copy()          # a few bytes per detection: the page-locked buffer goes back at once
        # inter int64 [NI] | area_gt int64 [NG] | area_pred int64 [G] | score fp32 [G] | channel int32 [G]
        i64 = raw[:8 * (NI + NG + G)].view(np.int64)
        score = raw[8 * (NI + NG + G):8 * (NI + NG + G) + 4 * G].view(np.float32)
        chan = raw[8 * (NI + NG + G) + 4 * G:8 * (NI + NG + G) + 8 * G].view(np.int32)
        out, d, a, x = [], 0, 0, 0
        for i, (nd, g) in enumerate(zip(nds, gs)):
            out.append({"pred_class": np.asarray(self._class_ids[i])[chan[d:d + nd]], "pred_score": score[d:d + nd],
                        "inter": i64[x:x + nd * g].reshape(nd, g), "area_pred": i64[NI + NG + d:NI + NG + d + nd],
                        "area_gt": i64[NI + a:NI + a + g]})
            d, a, x = d + nd, a + g, x + nd * g
        self._out = out
        return out


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
        return PendingOverlaps([], None, None, [], []) if deferred else []
    dev = rw_ups[0].device
    gs = [int(g) for g in n_insts]
    insts = []
    for i in range(n):
        _need_cuda(inst_maps[i], "inst_map")
        m = _u8_map(inst_maps[i], dev, "inst_map")
        if tuple(m.shape) != tuple(argmaxes[i].shape):
            raise ValueError("detection_overlap_batch: instance map %d is %s for a map of %s" % (i, tuple(m.shape), tuple(argmaxes[i].shape)))
        if not 0 <= gs[i] <= 255:
            raise ValueError("detection_overlap_batch: image %d has %d GT instances (0..255)" % (i, gs[i]))
        insts.append(m)
    bad = _accumulator(bad, (1,), dev, "bad")
    dc = _detect_batch_count(rw_ups, argmaxes, n_channels)                         # host round trip 1
    nds = dc.nds
    G, NG, NI = sum(nds), sum(gs), sum(nd * g for nd, g in zip(nds, gs))
    total = 8 * (NI + NG + G) + 8 * G
    host = done = None
    with torch.cuda.device(dev):
        # inter int64 [NI] | area_gt int64 [NG] | area_pred int64 [G] | score fp32 [G] | channel int32 [G]; the staging
        # buffer is the cached one when the call waits for its transfer, one of the batch's own when it is left in flight
        packed = (torch.empty(total + 8, dtype=torch.uint8, device=dev) if deferred
                  else _cached("det_ovl_out", dev, total + 8, torch.uint8))
        base = (packed.data_ptr() + 7) // 8 * 8
        shift = base - packed.data_ptr()
        at = [base, base + 8 * NI, base + 8 * (NI + NG), base + 8 * (NI + NG + G), base + 8 * (NI + NG + G) + 4 * G]
        check(lib.irn_detect_instance_batch_overlap(
            n, dc.sc_p, dc.am_p, dc.cs_a, dc.hs_a, dc.ws_a, i32_array(nds), (C.c_double * n)(*[float(v) for v in max_fragment_sizes]),
            ptr_array([m.data_ptr() for m in insts]), i32_array(gs), at[3] if G else None, at[4] if G else None,
            at[2] if G else None, at[0] if NI else None, at[1] if NG else None, bad.data_ptr(), dc.scratch.data_ptr(), _stream()))
        if total:
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            done = read_back(packed[shift:shift + total], host, side=deferred)     # host round trip 2
    pending = PendingOverlaps(nds, host, done, gs, class_ids)
    return pending if deferred else pending.result()


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


_CACHE = {}


def _cached(tag, dev, nbytes, dtype):
    """Grow-only scratch buffers (device) / pinned staging (dev == "pinned"), one per tag and device."""
    key = (tag, str(dev))
    buf = _CACHE.get(key)
    if buf is None or buf.numel() < nbytes:
        n = int(nbytes * 1.25) + 256
        buf = torch.empty(n, dtype=dtype, pin_memory=True) if dev == "pinned" else torch.empty(n, dtype=dtype, device=dev)
        _CACHE[key] = buf
    return buf


# --------------------------------------------------------------------------------------------------------------------
# dense CRF (misc/imutils.py:156-170 crf_inference_label, step/cam_to_ir_label.py:22-39): include/irn_hip.h irn_crf_*
# --------------------------------------------------------------------------------------------------------------------
CRF_T, CRF_GT_PROB = 10, 0.7          # the reference's defaults (misc/imutils.py:156)
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


# --------------------------------------------------------------------------------------------------------------------
# evaluation counts (step/eval_cam.py, step/eval_sem_seg.py, step/eval_ins_seg.py, step/tune_sem_seg.py): include/irn_hip.h
# irn_cam_confusion, irn_label_confusion, irn_mask_overlap, irn_label_sweep_confusion.  Accumulators are int64 GPU tensors that every
# call adds into; `bad` (int64 [1]) counts values outside the documented ranges and the caller raises when it is non-zero.
# --------------------------------------------------------------------------------------------------------------------
EVAL_CLASSES = 21                     # background + 20 VOC classes
EVAL_MAX_THRES = 256                  # IRN_EVAL_MAX_THRES


def _i64_zeros(shape, dev):
    return torch.zeros(shape, dtype=torch.int64, device=dev)


def _accumulator(t, shape, dev, what):
    if t is None:
        return _i64_zeros(shape, dev)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
            and tuple(t.shape) == tuple(shape) and t.device == dev):
        raise ValueError("%s must be a contiguous int64 GPU tensor of shape %s on %s" % (what, tuple(shape), dev))
    return t


def _u8_map(t, dev, what):
    if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.dtype in (torch.uint8, torch.bool)):
        raise ValueError("%s must be a uint8 [H,W] tensor" % what)
    return t.to(dev).view(torch.uint8).contiguous() if t.dtype == torch.bool else t.to(dev).contiguous()


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


def cam_confusion(high_res, keys, gt, thres, hist=None, bad=None):
    """step/eval_cam.py:14-19 + the confusion count for one image at every threshold of `thres` in one pass.

    high_res: GPU fp32 [K,H,W] (K >= 0), keys: 0-based classes [K], gt: uint8 [H,W] (255 = void), thres: GPU fp32 [T] from
    `eval_thresholds` (or anything it takes).  Adds into hist int64 [22,21,T+1] (row 21 = void GT, include/irn_hip.h) and
    bad int64 [1]; returns (hist, bad).  `cam_confusion_matrices(hist)` turns the histogram into the T matrices."""
    _need_cuda(high_res, "high_res")
    dev = high_res.device
    g = _u8_map(gt, dev, "gt")
    h, w = g.shape
    cams = high_res.to(torch.float32).contiguous()
    k = int(cams.shape[0]) if cams.dim() == 3 else -1
    if k < 0 or (k and tuple(cams.shape[1:]) != (h, w)):
        raise ValueError("cam_confusion: high_res %s for a GT of %dx%d" % (tuple(cams.shape), h, w))
    if k > EVAL_CLASSES - 1:
        raise ValueError("cam_confusion: %d CAM planes (at most %d)" % (k, EVAL_CLASSES - 1))
    ks = torch.as_tensor(keys).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if ks.numel() != k:
        raise ValueError("cam_confusion: %d keys for %d CAM planes" % (ks.numel(), k))
    th, t = _thres_tensor(thres, dev)
    hist = _accumulator(hist, (EVAL_CLASSES + 1, EVAL_CLASSES, t + 1), dev, "hist")
    bad = _accumulator(bad, (1,), dev, "bad")
    with torch.cuda.device(dev):
        check(lib.irn_cam_confusion(cams.data_ptr() if k else None, ks.data_ptr() if k else None, k, g.data_ptr(), h, w,
                                    th.data_ptr(), t, hist.data_ptr(), bad.data_ptr(), _stream()))
    return hist, bad


def cam_confusion_matrices(hist):
    """hist int64 [22,21,T+1] of `cam_confusion` -> (conf int64 [T,21,21] (row = GT, column = prediction), void int64
    [T,21] (predictions at GT-255 pixels)), on the GPU."""
    _need_cuda(hist, "hist")
    t = int(hist.shape[2]) - 1
    hist = _accumulator(hist, (EVAL_CLASSES + 1, EVAL_CLASSES, t + 1), hist.device, "hist")
    conf = _i64_zeros((t, EVAL_CLASSES, EVAL_CLASSES), hist.device)
    void = _i64_zeros((t, EVAL_CLASSES), hist.device)
    with torch.cuda.device(hist.device):
        check(lib.irn_cam_confusion_reduce(hist.data_ptr(), t, conf.data_ptr(), void.data_ptr(), _stream()))
    return conf, void


def label_sweep_confusion(rws, out_sizes, keys, gts, thres, hist=None, bad=None):
    """`label_epilogue` + `label_confusion` at every background threshold of `thres` in one pass, for a batch (no label
    map and no upsampled tensor is written), by the epilogue's own score functions and `cam_confusion`'s counting code.

    rws, out_sizes, keys: as for `label_epilogue` (at most 20 channels per image); gts: a list of uint8 [H,W] GPU tensors
    (255 = void), or ONE flat uint8 GPU buffer that holds the maps of `out_sizes` back to back; thres: GPU fp32 [T] from
    `eval_thresholds` (or anything it takes).  Adds into hist int64 [22,21,T+1] — the layout of `cam_confusion`, so
    `cam_confusion_matrices(hist)` gives the T matrices `label_confusion` counts on the labels of each threshold — and
    bad int64 [1]; returns (hist, bad).  Everything is checked before the launch: a refusal leaves hist / bad untouched."""
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
        if not 1 <= r.shape[0] <= EVAL_CLASSES - 1:
            raise ValueError("label_sweep_confusion: image %d has %d channels (1..%d)" % (i, r.shape[0], EVAL_CLASSES - 1))
        if not (1 <= sizes[i][0] <= 4 * r.shape[1] and 1 <= sizes[i][1] <= 4 * r.shape[2]):
            raise ValueError("label_sweep_confusion: image %d: output %s from a %dx%d map" % (i, sizes[i], r.shape[1], r.shape[2]))
        if k.numel() != r.shape[0]:
            raise ValueError("label_sweep_confusion: image %d: %d keys for %d channels" % (i, k.numel(), r.shape[0]))
    th, t = _thres_tensor(thres, dev)
    if not 1 <= t <= EVAL_MAX_THRES:
        raise ValueError("label_sweep_confusion: %d thresholds (1..%d)" % (t, EVAL_MAX_THRES))
    hist = _accumulator(hist, (EVAL_CLASSES + 1, EVAL_CLASSES, t + 1), dev, "hist")
    bad = _accumulator(bad, (1,), dev, "bad")
    scratch = torch.empty(max(n, 64), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.irn_label_sweep_confusion(
            n, ptr_array([r.data_ptr() for r in rs]), i32_array([r.shape[0] for r in rs]), i32_array([r.shape[1] for r in rs]),
            i32_array([r.shape[2] for r in rs]), i32_array([s[0] for s in sizes]), i32_array([s[1] for s in sizes]),
            ptr_array([k.data_ptr() for k in ks]), ptr_array(gt_ptrs), th.data_ptr(), t, hist.data_ptr(), bad.data_ptr(),
            scratch.data_ptr(), _stream()))
    return hist, bad


def label_confusion(pred, gt, conf=None, bad=None, pred_255_as=0, void=None):
    """step/eval_sem_seg.py:14-17 for one image: pred, gt uint8 [H,W] GPU tensors (pred 255 reads as `pred_255_as`; None =
    out of range).  Adds into conf int64 [21,21], void int64 [21] (predictions at GT-255 pixels) and bad int64 [1];
    returns (conf, void, bad)."""
    _need_cuda(pred, "pred")
    dev = pred.device
    p = _u8_map(pred, dev, "pred")
    g = _u8_map(gt, dev, "gt")
    if p.shape != g.shape:
        raise ValueError("label_confusion: prediction %s for a GT of %s" % (tuple(p.shape), tuple(g.shape)))
    conf = _accumulator(conf, (EVAL_CLASSES, EVAL_CLASSES), dev, "conf")
    void = _accumulator(void, (EVAL_CLASSES,), dev, "void")
    bad = _accumulator(bad, (1,), dev, "bad")
    h, w = g.shape
    with torch.cuda.device(dev):
        check(lib.irn_label_confusion(p.data_ptr(), g.data_ptr(), h, w, -1 if pred_255_as is None else int(pred_255_as),
                                      conf.data_ptr(), void.data_ptr(), bad.data_ptr(), _stream()))
    return conf, void, bad


def mask_overlap(masks, inst_map, n_inst, bad=None):
    """The counts behind chainercv's mask_iou for one image: masks bool/uint8 [N,H,W] and inst_map uint8 [H,W] (0 = no
    instance, 1..n_inst) on the GPU.  Returns (inter int64 [N,G], area_pred int64 [N], area_gt int64 [G]) on the GPU, with
    IoU = inter / (area_pred + area_gt - inter); values of inst_map above n_inst are counted in bad int64 [1]."""
    _need_cuda(inst_map, "inst_map")
    dev = inst_map.device
    inst = _u8_map(inst_map, dev, "inst_map")
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
    bad = _accumulator(bad, (1,), dev, "bad")
    with torch.cuda.device(dev):
        check(lib.irn_mask_overlap(m.data_ptr() if n else None, n, inst.data_ptr(), g, h, w,
                                   inter.data_ptr() if n and g else None, area_pred.data_ptr() if n else None,
                                   area_gt.data_ptr() if g else None, bad.data_ptr(), _stream()))
    return inter, area_pred, area_gt


# --------------------------------------------------------------------------------------------------------------------
# COCO mask encoding (step/make_cocoann.py): include/irn_hip.h irn_mask_rle_count / _emit.  The run lengths come from the
# GPU; pycocotools' string form of them (rleToString / rleFrString) is a few thousand counts per image and is made on the
# host, vectorised over the counts of a mask.
# --------------------------------------------------------------------------------------------------------------------
def mask_rle(masks):
    """pycocotools' rleEncode + rleArea + rleToBbox for masks bool / uint8 [N,H,W] on the GPU (nonzero = in the mask).

    Returns numpy arrays on the host: counts uint32 [total] (the run lengths of every mask in column-major pixel order,
    mask i at counts[offsets[i]:offsets[i+1]], in page-locked memory of their own), offsets int64 [N+1], area int64 [N]
    and bbox int32 [N,4] = [x0, y0, width, height].  Two synchronisations: one for the run counts (with area and bbox in
    the same transfer), one for the packed counts."""
    _need_cuda(masks, "masks")
    if not (masks.dim() == 3 and masks.dtype in (torch.uint8, torch.bool)):
        raise ValueError("mask_rle: masks must be a bool / uint8 [N,H,W] tensor, got %s %s" % (masks.dtype, tuple(masks.shape)))
    dev = masks.device
    m = (masks.view(torch.uint8) if masks.dtype == torch.bool else masks).contiguous()
    n, h, w = (int(v) for v in m.shape)
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros((0, 4), np.int32)
    nbytes = lib.irn_mask_rle_scratch_bytes(n, h, w)
    if nbytes == 0:
        check(1)
    scratch = _cached("rle_scratch", dev, nbytes, torch.uint8)
    # one device block for everything the first transfer brings back: area int64 [n] | bbox int32 [n][4] | n_runs int32 [n]
    head = _cached("rle_head", dev, 28 * n + 8 * (n + 2), torch.uint8)
    host = _cached("rle_head", "pinned", 28 * n + 8 * (n + 2), torch.uint8)
    p_area = head.data_ptr()
    p_bbox, p_runs, p_off = p_area + 8 * n, p_area + 24 * n, p_area + 28 * n + (-28 * n) % 8
    with torch.cuda.device(dev):
        check(lib.irn_mask_rle_count(m.data_ptr(), n, h, w, p_runs, p_area, p_bbox, scratch.data_ptr(), _stream()))
        host[:28 * n].copy_(head[:28 * n], non_blocking=True)
        torch.cuda.current_stream().synchronize()                              # host round trip 1
        raw = host[:28 * n].numpy()
        area, bbox = raw[:8 * n].view(np.int64).copy(), raw[8 * n:24 * n].view(np.int32).reshape(n, 4).copy()
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(raw[24 * n:28 * n].view(np.int32), out=offsets[1:])
        total = int(offsets[n])
        o = p_off - p_area
        host[o:o + 8 * (n + 1)].view(torch.int64).copy_(torch.from_numpy(offsets))
        head[o:o + 8 * (n + 1)].copy_(host[o:o + 8 * (n + 1)], non_blocking=True)
        counts_dev = _cached("rle_counts", dev, 4 * total, torch.uint8)
        check(lib.irn_mask_rle_emit(m.data_ptr(), n, h, w, p_off, counts_dev.data_ptr(), scratch.data_ptr(), _stream()))
        # page-locked memory of the call's own: the counts are handed out as a view of it (torch's caching host allocator
        # takes it back when the last view is dropped)
        out = torch.empty(4 * total, dtype=torch.uint8, pin_memory=True)
        out.copy_(counts_dev[:4 * total], non_blocking=True)
        torch.cuda.current_stream().synchronize()                              # host round trip 2
    return out.numpy().view(np.uint32), offsets, area, bbox


def rle_to_string(counts):
    """pycocotools' rleToString: the run lengths of one mask as COCO's compressed ASCII string (characters '0'..'o').
    Count i is stored as counts[i] - counts[i-2] for i > 2, in 5-bit groups, least significant first, bit 5 = more follow."""
    c = np.asarray(counts).astype(np.int64).reshape(-1)
    x = c.copy()
    x[3:] -= c[1:-2]
    groups = 7                                             # |x| < 2^32: 33 bits with the sign, 7 groups of 5
    shifted = x[:, None] >> (5 * np.arange(groups + 1, dtype=np.int64))[None, :]       # arithmetic shift
    chunk = shifted[:, :groups] & 31
    rest = shifted[:, 1:]
    more = np.where(chunk & 16, rest != -1, rest != 0)
    emitted = np.ones_like(more)
    emitted[:, 1:] = np.logical_and.accumulate(more[:, :-1], axis=1)
    chars = (chunk | (more.astype(np.int64) << 5)) + 48
    return chars[emitted].astype(np.uint8).tobytes().decode("ascii")


def rle_from_string(s):
    """pycocotools' rleFrString: COCO's compressed string (str or bytes) back to the run lengths, uint32."""
    b = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), np.uint8).astype(np.int64) - 48
    if b.size == 0:
        return np.zeros(0, np.uint32)
    if ((b < 0) | (b > 63)).any() or b[-1] & 32:
        raise ValueError("rle_from_string: not a COCO run-length string")
    last = (b & 32) == 0                                   # the last group of every count
    start = np.flatnonzero(np.concatenate([[True], last[:-1]]))
    k = np.arange(b.size) - np.repeat(start, np.diff(np.append(start, b.size)))       # group number within its count
    x = np.add.reduceat((b & 31) << (5 * k), start)
    ends = np.flatnonzero(last)
    neg = (b[ends] & 16) != 0
    x[neg] |= np.int64(-1) << (5 * (k[ends][neg] + 1))    # sign extension
    x[2::2] = np.cumsum(x[2::2])                           # counts[i] = x[i] + counts[i-2] for i > 2
    x[1::2] = np.cumsum(x[1::2])
    if (x < 0).any() or (x > 0xffffffff).any():
        raise ValueError("rle_from_string: a run length outside 0..2^32-1")
    return x.astype(np.uint32)


def rle_decode(counts, h, w):
    """The mask of pycocotools' rleDecode: bool [h,w] from the run lengths of its column-major pixel order."""
    c = np.asarray(counts).astype(np.int64).reshape(-1)
    if (c < 0).any() or int(c.sum()) != h * w:
        raise ValueError("rle_decode: the counts sum to %d, the mask has %d pixels" % (int(c.sum()), h * w))
    bits = np.repeat(np.arange(c.size) & 1, c).astype(bool)
    return np.ascontiguousarray(bits.reshape(w, h).T)
