"""The backward of the one-pass bilinear upsampling (irn_upsample_bilinear_backward, `ops.upsample_bilinear` under autograd)
on the GPU.

Tolerance of the values.  The reference is `F.interpolate(mode="bilinear", align_corners=False)` (+ ReLU) in fp64 on the CPU
with a random `grad_out` sent back through it.  ATen's own fp32 GPU backward is measured against it in the same run; the
gather is allowed 4x that distance, since only the order of the additions differs, with a floor of one fp32 ulp of the
largest gradient magnitude (where ATen happens to be exact).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PLANES = ((3, 1, 1), (2, 3, 5), (4, 16, 16), (1, 7, 64))       # planes x h x w: one cell (clamped both ways), odd sizes, several rows of threads, a full wave row
CASES = [(p, f, r) for p in PLANES for f in (2, 4) for r in (0, 1)]
IDS = ["%dx%dx%d_f%d_relu%d" % (p + (f, r)) for p, f, r in CASES]


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(plane, factor, relu):
    """x, grad_out (CPU fp32) and the fp64 gradient, computed once."""
    n, h, w = plane
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w + factor)
    x = torch.randn(1, n, h, w, generator=g)
    grad_out = torch.randn(1, n, h * factor, w * factor, generator=g)
    x64 = x.double().requires_grad_(True)
    y = F.interpolate(x64, scale_factor=factor, mode="bilinear", align_corners=False)
    (torch.relu(y) if relu else y).backward(grad_out.double())
    return x, grad_out, x64.grad


def _entry(grad_out, out, plane, factor, relu):
    """The C entry on an output filled with NaN beforehand."""
    from irn_amd._lib import _stream, check, lib
    n, h, w = plane
    grad_in = torch.full((1, n, h, w), float("nan"), device=_dev())
    check(lib.irn_upsample_bilinear_backward(grad_out.data_ptr(), out.data_ptr() if relu else None, n, h, w, factor, relu,
                                             grad_in.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return grad_in


@pytest.mark.parametrize("plane,factor,relu", CASES, ids=IDS)
def test_values_against_fp64_with_atens_own_distance_as_the_bar(plane, factor, relu):
    from irn_amd import ops
    x, grad_out, want = _case(plane, factor, relu)
    xa = x.to(_dev()).requires_grad_(True)
    y = F.interpolate(xa, scale_factor=factor, mode="bilinear", align_corners=False)
    (torch.relu(y) if relu else y).backward(grad_out.to(_dev()))
    aten = float((xa.grad.cpu().double() - want).abs().max())
    xo = x.to(_dev()).requires_grad_(True)
    ops.upsample_bilinear(xo, factor, relu=bool(relu)).backward(grad_out.to(_dev()))
    got = float((xo.grad.cpu().double() - want).abs().max())
    ulp = float(np.spacing(np.float32(want.abs().max())))
    print("\n%s x%d relu=%d: gather %.3e, ATen %.3e, one ulp of the largest gradient %.3e" % (plane, factor, relu, got, aten, ulp))
    assert xo.grad.shape == x.shape and torch.isfinite(xo.grad).all()
    assert got <= max(4 * aten, ulp), "max-abs error %.3e, bound %.3e" % (got, max(4 * aten, ulp))


@pytest.mark.parametrize("plane,factor,relu", CASES, ids=IDS)
def test_five_calls_give_the_same_bits_and_write_every_cell(plane, factor, relu):
    from irn_amd import ops
    x, grad_out, _ = _case(plane, factor, relu)
    out = ops.upsample_bilinear(x.to(_dev()), factor, relu=bool(relu))
    g = grad_out.to(_dev())
    first = _entry(g, out, plane, factor, relu)
    assert not torch.isnan(first).any(), "a cell was left unwritten"
    for _ in range(4):
        assert torch.equal(_entry(g, out, plane, factor, relu), first)
    # and the operator's backward is that entry
    xo = x.to(_dev()).requires_grad_(True)
    ops.upsample_bilinear(xo, factor, relu=bool(relu)).backward(g)
    assert torch.equal(xo.grad, first)


@pytest.mark.parametrize("plane,factor,relu", CASES, ids=IDS)
def test_forward_under_autograd_equals_the_forward_without(plane, factor, relu):
    from irn_amd import ops
    x = _case(plane, factor, relu)[0].to(_dev())
    plain = ops.upsample_bilinear(x, factor, relu=bool(relu))
    with torch.no_grad():
        no_grad = ops.upsample_bilinear(x.clone().requires_grad_(True), factor, relu=bool(relu))
    tracked = ops.upsample_bilinear(x.clone().requires_grad_(True), factor, relu=bool(relu))
    assert not plain.requires_grad and not no_grad.requires_grad and tracked.requires_grad
    assert torch.equal(tracked.detach(), plain) and torch.equal(no_grad, plain)
