"""Host side of irn_amd/csrc/bn_act.hip: the trunk's elementwise passes — inference batch norm (+ residual) (+ ReLU) in
place (`bn_act_`) and as a differentiable pass (`bn_act`), the stem's batch norm + ReLU + max pool, and the IRNet heads'
bilinear upsampling.  `irn_amd.ops` re-exports the functions.  GPU tensors in, GPU tensors out; no CPU fallback."""
import torch

from ._host import need_f32_contig
from ._lib import _need_cuda, _need_vec, _stream, check, lib


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
    plane = x[0, 0].numel() if n_img else 0
    rs, rb = (None, None) if residual_affine is None else (residual_affine[0].data_ptr(), residual_affine[1].data_ptr())
    # the entry points take at most 2^31 - 1 elements: larger batches go image group by image group
    per = max(1, (2 ** 31 - 1) // max(1, n_ch * plane))
    with torch.cuda.device(x.device):
        for i in range(0, n_img, per):
            xi = x[i:i + per]
            ri = None if residual is None else residual[i:i + per].data_ptr()
            if nhwc:
                check(lib.irn_bn_act_nhwc(xi.data_ptr(), ri, scale.data_ptr(), shift.data_ptr(), rs, rb,
                                          int(xi.shape[0]) * plane, n_ch, 1 if relu else 0, _stream()))
            else:
                check(lib.irn_bn_act(xi.data_ptr(), ri, scale.data_ptr(), shift.data_ptr(), rs, rb,
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


def bn_act_backward(grad_out, out, x, res, scale, res_scale, relu, want_x, want_res, want_sums):
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
            gx, gr, sums = bn_act_backward(grad_out, out, x, residual, scale, rs, ctx.relu, want_x, want_res, want_sums)
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


def stem_pool(x, scale, shift):
    """Batch norm + ReLU + 3x3 / stride 2 / pad 1 max pool of the trunk's stem in one pass (irn_stem_pool; reference
    net/resnet50.py:94-97).  x: GPU fp32 [N, C, H, W] (conv1's output, left untouched) -> [N, C, (H-1)//2+1, (W-1)//2+1]."""
    need_f32_contig(x, "stem_pool: x", 4)
    n, c, h, w = (int(v) for v in x.shape)
    _need_vec(scale, "stem_pool: scale", c, x.device)
    _need_vec(shift, "stem_pool: shift", c, x.device)
    out = torch.empty((n, c, (h - 1) // 2 + 1 if h else 0, (w - 1) // 2 + 1 if w else 0), dtype=torch.float32, device=x.device)
    if out.numel():
        with torch.cuda.device(x.device):
            check(lib.irn_stem_pool(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), n, c, h, w, out.data_ptr(), _stream()))
    return out


def _upsample_bilinear_forward(x, factor, relu):
    h, w = int(x.shape[-2]), int(x.shape[-1])
    out = torch.empty(tuple(x.shape[:-2]) + (h * factor, w * factor), dtype=torch.float32, device=x.device)
    if out.numel():
        with torch.cuda.device(x.device):
            check(lib.irn_upsample_bilinear(x.data_ptr(), x.numel() // (h * w), h, w, factor, 1 if relu else 0, out.data_ptr(),
                                            _stream()))
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
    need_f32_contig(x, "upsample_bilinear: x", 2)
    if int(factor) != factor or not 1 <= factor <= 64:
        raise ValueError("upsample_bilinear: integer factor in 1..64 expected, got %r" % (factor,))
    factor = int(factor)
    if x.requires_grad and torch.is_grad_enabled():
        return _UpsampleBilinear.apply(x, factor, bool(relu))
    return _upsample_bilinear_forward(x, factor, relu)
