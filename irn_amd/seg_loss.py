"""Host side of irn_amd/csrc/seg_loss.hip and seg_fuse.hip: the fused bilinear-upsampling + softmax cross-entropy of
segmentation training, the arg-max of segmentation inference and its multi-scale fusion.  `irn_amd.ops` re-exports the
functions.  GPU tensors in, GPU tensors out; no CPU fallback."""
import torch

from ._lib import _need_cuda, _stream, check, i32_array, lib, ptr_array

MAX_CLASSES = 81                      # IRN_EVAL_MAX_CLASSES: background + 80
SEG_FUSE_MAX_MAPS = 16                # IRN_SEG_FUSE_MAX_MAPS


def _need_logits(who, logits, factor):
    _need_cuda(logits, "%s: logits" % who)
    if logits.dtype != torch.float32 or logits.dim() != 4 or not logits.is_contiguous():
        raise ValueError("%s: logits must be a contiguous fp32 [B, C, h, w] tensor, got %s %s %s"
                         % (who, logits.dtype, tuple(logits.shape), logits.stride()))
    if not (isinstance(factor, int) and not isinstance(factor, bool) and 1 <= factor <= 64):
        raise ValueError("%s: integer factor in 1..64 expected, got %r" % (who, factor))
    if not 2 <= logits.shape[1] <= MAX_CLASSES:
        raise ValueError("%s: %d channels outside 2..%d" % (who, logits.shape[1], MAX_CLASSES))


def _need_label(who, logits, label, factor):
    _need_cuda(label, "%s: label" % who)
    if label.dtype != torch.uint8 or label.dim() != 3 or not label.is_contiguous() or label.device != logits.device:
        raise ValueError("%s: label must be a contiguous uint8 [B, H, W] tensor on %s, got %s %s"
                         % (who, logits.device, label.dtype, tuple(label.shape)))
    b, _, h, w = logits.shape
    if label.shape[0] != b or not (1 <= label.shape[1] <= h * factor and 1 <= label.shape[2] <= w * factor):
        raise ValueError("%s: label %s does not fit logits %s upsampled by %d" % (who, tuple(label.shape), tuple(logits.shape), factor))


class _SegLossSums(torch.autograd.Function):
    """irn_seg_loss_forward with irn_seg_loss_backward (a gather: no atomics, the same bits every time) as its vector-Jacobian
    product.  Saves the logits, the labels and the per-pixel log-sum-exp (fp64 [B, H, W]); no [B, C, H, W] tensor exists."""

    @staticmethod
    def forward(ctx, logits, label, factor):
        b, c, h, w = logits.shape
        hh, ww = int(label.shape[1]), int(label.shape[2])
        geom = (b, c, h, w, factor, hh, ww)
        need = lib.irn_seg_loss_workspace_bytes(*geom)
        if need == 0:
            raise ValueError("seg_loss_sums: logits %s, factor %d, label %s is not a shape the kernel takes"
                             % (tuple(logits.shape), factor, tuple(label.shape)))
        dev = logits.device
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        sums = torch.empty(b, dtype=torch.float64, device=dev)
        counts = torch.empty(b, dtype=torch.int64, device=dev)
        lse = torch.empty((b, hh, ww), dtype=torch.float64, device=dev) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(dev):
            check(lib.irn_seg_loss_forward(logits.data_ptr(), label.data_ptr(), *geom, sums.data_ptr(), counts.data_ptr(),
                                           None if lse is None else lse.data_ptr(), ws.data_ptr(), need, _stream()))
        if lse is not None:
            ctx.save_for_backward(logits, label, lse)
        ctx.geom, ctx.ws = geom, ws
        ctx.mark_non_differentiable(counts)
        return sums, counts

    @staticmethod
    def backward(ctx, grad_sums, _grad_counts):
        logits, label, lse = ctx.saved_tensors
        coef = grad_sums.to(torch.float32).contiguous()          # stays on the device: nothing synchronises
        grad = torch.empty_like(logits)
        with torch.cuda.device(logits.device):
            check(lib.irn_seg_loss_backward(logits.data_ptr(), label.data_ptr(), lse.data_ptr(), coef.data_ptr(), *ctx.geom,
                                            grad.data_ptr(), ctx.ws.data_ptr(), ctx.ws.numel(), _stream()))
        return grad, None, None


def seg_loss_sums(logits, label, factor):
    """Per image, the sum over the valid pixels of the softmax cross-entropy of the logits upsampled bilinearly by `factor`
    (align_corners = False, the arithmetic of `upsample_bilinear`) against `label`, and the number of valid pixels: what
    `F.cross_entropy(F.interpolate(logits, scale_factor=factor, mode='bilinear')[..., :H, :W], label, ignore_index=255,
    reduction='sum')` gives per image, in one pass without the upsampled tensor (include/irn_hip.h, irn_seg_loss_forward).

    ``logits``: GPU fp32 [B, C, h, w], contiguous, C in 2..81; ``label``: GPU uint8 [B, H, W], H <= h * factor,
    W <= w * factor (the top-left window of the upsampling), a byte >= C is ignored.  Returns ``(sums, counts)``: fp64 [B] and
    int64 [B] on the device.  Differentiable w.r.t. ``logits``; forward and backward are bit-reproducible and an image's
    results do not depend on the images batched with it."""
    _need_logits("seg_loss_sums", logits, factor)
    _need_label("seg_loss_sums", logits, label, factor)
    return _SegLossSums.apply(logits, label, factor)


def seg_cross_entropy(logits, label, factor):
    """Mean cross-entropy over the valid pixels of the batch: `seg_loss_sums(...)` as sums.sum() / counts.sum().clamp(min=1),
    an fp64 device scalar.  A batch without a valid pixel gives 0 with zero gradients, not NaN."""
    sums, counts = seg_loss_sums(logits, label, factor)
    return sums.sum() / counts.sum().clamp(min=1)


def seg_argmax(logits, factor, out_hw):
    """torch.argmax(upsample_bilinear(logits, factor)[..., :H, :W], 1) as uint8 [B, H, W] without the upsampled tensor
    (irn_seg_argmax): the first channel that attains the maximum, a NaN counting as the maximum.  ``out_hw`` = (H, W)."""
    _need_logits("seg_argmax", logits, factor)
    b, c, h, w = logits.shape
    hh, ww = int(out_hw[0]), int(out_hw[1])
    if not (1 <= hh <= h * factor and 1 <= ww <= w * factor):
        raise ValueError("seg_argmax: out_hw %s outside logits %s upsampled by %d" % ((hh, ww), tuple(logits.shape), factor))
    out = torch.empty((b, hh, ww), dtype=torch.uint8, device=logits.device)
    with torch.cuda.device(logits.device):
        check(lib.irn_seg_argmax(logits.data_ptr(), b, c, h, w, factor, hh, ww, out.data_ptr(), _stream()))
    return out


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def seg_fuse(maps, sizes, stride, out_hw, want_label=True, want_prob=False):
    """Multi-scale inference of one image in one launch (irn_seg_fuse): every map's logits upsampled bilinearly
    to ``out_hw`` = (H, W), the softmax of each, their mean P and its arg-max, without any [C, H, W] tensor but the one asked for.

    ``maps``: list of 1..16 GPU fp32 [C, h, w] tensors, contiguous, C in 2..81, one per scale; ``sizes``: list of (Hs, Ws),
    the size of the rescaled image map m was computed from, with Hs <= h * stride and Hs <= stride * H (likewise the widths):
    map m is read at ratio Hs / (stride * H).  Returns ``(label, prob)``: uint8 [H, W] = the first class that attains the
    maximum of P (a NaN counts as the maximum) and fp32 [C, H, W] = P, each None unless asked for.  Bit-reproducible; label is
    the arg-max of the very P that prob holds."""
    who = "seg_fuse"
    if not isinstance(maps, (list, tuple)) or not 1 <= len(maps) <= SEG_FUSE_MAX_MAPS:
        raise ValueError("%s: maps must be a list of 1..%d tensors" % (who, SEG_FUSE_MAX_MAPS))
    if not isinstance(sizes, (list, tuple)) or len(sizes) != len(maps):
        raise ValueError("%s: sizes must be a list of one (Hs, Ws) per map, %d maps" % (who, len(maps)))
    if not (_is_int(stride) and 1 <= stride <= 64):
        raise ValueError("%s: integer stride in 1..64 expected, got %r" % (who, stride))
    if not (want_label or want_prob):
        raise ValueError("%s: neither the label nor the probabilities are asked for" % who)
    try:
        hh, ww = int(out_hw[0]), int(out_hw[1])
        sizes = [(int(s[0]), int(s[1])) for s in sizes]
    except (TypeError, ValueError, IndexError):
        raise ValueError("%s: out_hw and every entry of sizes must be a pair of integers, got %r and %r" % (who, out_hw, sizes))
    if not (1 <= hh <= 32768 and 1 <= ww <= 32768):
        raise ValueError("%s: out_hw %s outside 1..32768" % (who, (hh, ww)))
    for m, t in enumerate(maps):
        _need_cuda(t, "%s: maps[%d]" % (who, m))
        if t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous():
            raise ValueError("%s: maps[%d] must be a contiguous fp32 [C, h, w] tensor, got %s %s %s"
                             % (who, m, t.dtype, tuple(t.shape), t.stride()))
        if t.device != maps[0].device or t.shape[0] != maps[0].shape[0]:
            raise ValueError("%s: maps[%d] has %d channels on %s, maps[0] %d on %s"
                             % (who, m, t.shape[0], t.device, maps[0].shape[0], maps[0].device))
        hs, ws = sizes[m]
        if not (1 <= hs <= min(t.shape[1], hh) * stride and 1 <= ws <= min(t.shape[2], ww) * stride):
            raise ValueError("%s: sizes[%d] = %s does not fit a map of %s and an output of %s at stride %d"
                             % (who, m, (hs, ws), tuple(t.shape[1:]), (hh, ww), stride))
    c = int(maps[0].shape[0])
    if not 2 <= c <= MAX_CLASSES:
        raise ValueError("%s: %d channels outside 2..%d" % (who, c, MAX_CLASSES))
    dev = maps[0].device
    label = torch.empty((hh, ww), dtype=torch.uint8, device=dev) if want_label else None
    prob = torch.empty((c, hh, ww), dtype=torch.float32, device=dev) if want_prob else None
    with torch.cuda.device(dev):
        check(lib.irn_seg_fuse(ptr_array([t.data_ptr() for t in maps]), i32_array([t.shape[1] for t in maps]),
                               i32_array([t.shape[2] for t in maps]), i32_array([s[0] for s in sizes]),
                               i32_array([s[1] for s in sizes]), len(maps), c, stride, hh, ww,
                               None if label is None else label.data_ptr(), None if prob is None else prob.data_ptr(), _stream()))
    return label, prob
