"""The differentiable fused tail of the trunk (irn_bn_fold, irn_bn_act_forward, irn_bn_act_backward; ops.bn_act) on the GPU:
the fold against `FrozenBatchNorm._fold64().float()`, the forward against the in-place inference kernel, the backward against
the fp64 restatement in tests/_bn_act_train_ref.py with the mask taken from the kernel's own forward output — so that every
comparison is exact (products) or bounded by the rounding of a double sum, never by where a ReLU happened to cut."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_act_train_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 1e-5

# the shapes of tests/test_gpu_bn_act.py (planes that are / are not a multiple of four long, pieces straddling planes, planes
# shorter than a piece, one channel, many channels) and two from the backward's constants (a share = 4096 elements):
#   (5, 3, 40, 40)   1600-element planes: two whole planes per share, a channel's sum spans three workgroups, the last with
#                    one plane only (less than a full share)
#   (2, 3, 65, 67)   4355-element planes (odd: every plane starts at another offset in its 16-byte piece): two chunks per
#                    plane, the second 259 elements long
SHAPES = [(2, 8, 16, 16), (3, 5, 7, 9), (2, 3, 1, 5), (4, 6, 1, 1), (1, 1, 3, 1), (1, 7, 1, 3), (2, 64, 33, 47), (1, 2048, 2, 3),
          (16, 3, 5, 5), (1, 1, 1, 1027), (2, 1, 31, 2), (5, 3, 40, 40), (2, 3, 65, 67)]
MODES = ["plain", "residual", "residual_bn"]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def _case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    t = {"x": torch.randn(shape, generator=g), "res": torch.randn(shape, generator=g), "grad_out": torch.randn(shape, generator=g)}
    for p in ("", "r_"):
        t[p + "weight"] = torch.rand(c, generator=g) * 2.5 - 1.0               # negative scales too
        t[p + "bias"] = torch.randn(c, generator=g)
        t[p + "mean"] = torch.randn(c, generator=g)
        t[p + "var"] = torch.rand(c, generator=g) * 2 + 0.05
    return {k: v.to(_dev()) for k, v in t.items()}


def _forward(t, mode, relu):
    from irn_amd import ops
    res = None if mode == "plain" else t["res"]
    rbn = (t["r_weight"], t["r_bias"], t["r_mean"], t["r_var"], EPS) if mode == "residual_bn" else None
    with torch.no_grad():
        return ops.bn_act(t["x"], t["weight"], t["bias"], t["mean"], t["var"], EPS, res, relu, rbn)


def _fsum_channels(terms):
    """Exact (correctly rounded) per-channel sums of a float64 [N, C, ...] array, and the sums of magnitudes."""
    c = terms.shape[1]
    rows = np.moveaxis(terms, 1, 0).reshape(c, -1)
    return np.array([math.fsum(r) for r in rows]), np.abs(rows).sum(axis=1)


def test_fold_equals_fold64_rounded_bit_for_bit():
    from irn_amd import ops
    from irn_amd.net import resnet50 as R
    g = torch.Generator().manual_seed(21)
    c = 1031
    bn = R.FrozenBatchNorm(c)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(c, generator=g))
        bn.bias.copy_(torch.randn(c, generator=g))
        bn.running_mean.copy_(torch.randn(c, generator=g) * 30)
        bn.running_var.copy_(torch.rand(c, generator=g) * 3)
        bn.running_var[:64] = torch.rand(64, generator=g) * 1e-9                 # eps decides
        bn.running_var[64:128] = torch.rand(64, generator=g) * 1e9 + 1e6          # large variances
        bn.running_var[128] = 0.0
        bn.weight[129] = 0.0
    want = tuple(v.float() for v in bn._fold64())                                 # IEEE double on the CPU
    dev = _dev()
    bnd = bn.to(dev)
    for _ in range(2):
        scale, shift = ops.bn_fold(bnd.weight, bnd.bias, bnd.running_mean, bnd.running_var, bnd.eps)
        assert scale.dtype == torch.float32 and scale.is_contiguous() and shift.is_contiguous()
        assert torch.equal(scale.cpu(), want[0]) and torch.equal(shift.cpu(), want[1])
    on_dev = tuple(v.float() for v in bnd._fold64())
    assert torch.equal(scale, on_dev[0]) and torch.equal(shift, on_dev[1])
    s1, b1 = ops.bn_fold(bnd.weight[:1].clone(), bnd.bias[:1].clone(), bnd.running_mean[:1].clone(), bnd.running_var[:1].clone(), bnd.eps)
    assert torch.equal(s1.cpu(), want[0][:1]) and torch.equal(b1.cpu(), want[1][:1])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("relu", [False, True])
def test_forward_equals_the_inplace_kernel_and_backward_equals_the_restatement(shape, mode, relu):
    from irn_amd import ops
    t = _case(shape, 5 + shape[1] + len(mode))
    x0 = t["x"].clone()
    out = _forward(t, mode, relu)
    assert torch.equal(t["x"], x0) and out.data_ptr() != t["x"].data_ptr()       # out of place
    scale, shift = ops.bn_fold(t["weight"], t["bias"], t["mean"], t["var"], EPS)
    rs, rb = ops.bn_fold(t["r_weight"], t["r_bias"], t["r_mean"], t["r_var"], EPS)
    want = ops.bn_act_(t["x"].clone(), scale, shift, None if mode == "plain" else t["res"], relu, (rs, rb) if mode == "residual_bn" else None)
    assert torch.equal(out, want)

    # backward, every combination of requested outputs; the mask is the kernel's own output
    res_bn = mode == "residual_bn"
    g = t["grad_out"].cpu().numpy()
    mask = B.relu_mask(out.cpu().numpy()) if relu else np.ones(shape, dtype=bool)
    gx64, gr64 = B.grads(g, mask, scale.cpu().numpy(), rs.cpu().numpy() if res_bn else None)
    dz = np.where(mask, g.astype(np.float64), 0.0)
    terms = [dz, dz * t["x"].cpu().numpy().astype(np.float64)] + ([dz * t["res"].cpu().numpy().astype(np.float64)] if res_bn else [])
    exact = [_fsum_channels(v) for v in terms]
    n = shape[0] * int(np.prod(shape[2:]))
    combos = [c for c in itertools.product([False, True], repeat=3) if any(c) and (mode != "plain" or not c[1])]
    for want_x, want_res, want_sums in combos:
        gx, gr, sums = ops.bn_act_backward(t["grad_out"], out, t["x"], t["res"] if res_bn else None, scale, rs if res_bn else None,
                                            relu, want_x, want_res, want_sums)
        assert (gx is not None) == want_x and (gr is not None) == want_res and (sums is not None) == want_sums
        if want_x:
            assert np.array_equal(gx.cpu().numpy(), gx64.astype(np.float32), equal_nan=True)          # one rounding of the exact product
        if want_res:
            assert np.array_equal(gr.cpu().numpy(), gr64.astype(np.float32), equal_nan=True)
        if want_sums:
            assert sums.dtype == torch.float64 and tuple(sums.shape) == (len(terms), shape[1])
            got = sums.cpu().numpy()
            for q, (s, mag) in enumerate(exact):
                # products of two floats are exact in double: the whole error is that of the summation, in any order
                assert (np.abs(got[q] - s) <= n * 2.0 ** -53 * mag).all(), (q, float(np.abs(got[q] - s).max()))


@pytest.mark.parametrize("shape", [(5, 3, 40, 40), (2, 3, 65, 67), (3, 5, 7, 9)])
def test_five_calls_give_identical_bits(shape):
    from irn_amd import ops
    t = _case(shape, 77)
    out = _forward(t, "residual_bn", True)
    scale, _ = ops.bn_fold(t["weight"], t["bias"], t["mean"], t["var"], EPS)
    rs, _ = ops.bn_fold(t["r_weight"], t["r_bias"], t["r_mean"], t["r_var"], EPS)
    first = None
    for _ in range(5):
        got = ops.bn_act_backward(t["grad_out"], out, t["x"], t["res"], scale, rs, True, True, True, True)
        got = [v.clone() for v in got]
        if first is None:
            first = got
        assert all(torch.equal(a, b) for a, b in zip(first, got))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("relu", [False, True])
def test_autograd_function_honours_needs_input_grad(mode, relu):
    """ops.bn_act under autograd: gradients for exactly the inputs that ask for one, equal to what the kernel and
    `bn_param_grads` give when called by hand."""
    from irn_amd import ops
    shape = (3, 6, 9, 7)
    base = _case(shape, 13)
    res_bn = mode == "residual_bn"
    keys = ["x", "weight", "bias"] + (["res"] if mode != "plain" else []) + (["r_weight", "r_bias"] if res_bn else [])
    full = None
    for wanted in [tuple(keys)] + [(k,) for k in keys]:
        t = {k: v.clone().requires_grad_(k in wanted) for k, v in base.items()}
        rbn = (t["r_weight"], t["r_bias"], t["r_mean"], t["r_var"], EPS) if res_bn else None
        out = ops.bn_act(t["x"], t["weight"], t["bias"], t["mean"], t["var"], EPS, None if mode == "plain" else t["res"], relu, rbn)
        assert out.requires_grad and type(out.grad_fn).__name__.startswith("_BnAct")
        out.backward(base["grad_out"])
        grads = {k: t[k].grad for k in base}
        assert all((grads[k] is not None) == (k in wanted) for k in base), (wanted, [k for k in base if grads[k] is not None])
        if full is None:
            full = grads
            scale, _ = ops.bn_fold(base["weight"], base["bias"], base["mean"], base["var"], EPS)
            rs = ops.bn_fold(base["r_weight"], base["r_bias"], base["r_mean"], base["r_var"], EPS)[0] if res_bn else None
            gx, gr, sums = ops.bn_act_backward(base["grad_out"], out.detach(), base["x"], base["res"] if res_bn else None, scale, rs,
                                                relu, True, mode != "plain", True)
            gw, gb = ops.bn_param_grads(sums[0], sums[1], base["mean"], base["var"], EPS)
            assert torch.equal(grads["x"], gx) and torch.equal(grads["weight"], gw) and torch.equal(grads["bias"], gb)
            if mode != "plain":
                assert torch.equal(grads["res"], gr)
            if res_bn:
                gw, gb = ops.bn_param_grads(sums[0], sums[2], base["r_mean"], base["r_var"], EPS)
                assert torch.equal(grads["r_weight"], gw) and torch.equal(grads["r_bias"], gb)
            # and against the composed ops in fp32 on the device: the same gradients up to fp32 rounding of long sums
            c = {k: v.clone().requires_grad_(k in wanted) for k, v in base.items()}
            y = F.batch_norm(c["x"], c["mean"], c["var"], c["weight"], c["bias"], False, 0.0, EPS)
            if mode == "residual":
                y = y + c["res"]
            elif res_bn:
                y = y + F.batch_norm(c["res"], c["r_mean"], c["r_var"], c["r_weight"], c["r_bias"], False, 0.0, EPS)
            y = F.relu(y) if relu else y
            assert float((y - out).detach().abs().max()) <= 4e-6 * max(1.0, float(y.detach().abs().max()))
        else:
            assert all(torch.equal(grads[k], full[k]) for k in wanted)           # asking for less changes no bit of the rest


def test_nan_and_signed_zero_as_in_torchs_relu_backward():
    from irn_amd import ops
    dev = _dev()
    vals = [float("nan"), -1.0, 2.0, float("inf"), -float("inf"), 0.0, -0.0, 1.0, 3.0]
    x = torch.tensor(vals, device=dev).view(1, 1, 9).requires_grad_(True)
    one, zero = torch.ones(1, device=dev), torch.zeros(1, device=dev)
    grad_out = torch.tensor([1.0, float("nan"), 1.0, 1.0, 1.0, 1.0, 1.0, float("nan"), float("inf")], device=dev).view(1, 1, 9)
    var = torch.ones(1, device=dev) - EPS
    assert float(ops.bn_fold(one, zero, zero, var, EPS)[0]) == 1.0               # the layer is the identity: scale 1, shift 0
    ops.bn_act(x, one, zero, zero, var, EPS, relu=True).backward(grad_out)
    xt = x.detach().clone().requires_grad_(True)
    torch.relu(xt).backward(grad_out)
    assert torch.equal(torch.isnan(x.grad), torch.isnan(xt.grad))
    assert torch.equal(torch.nan_to_num(x.grad, nan=7.0), torch.nan_to_num(xt.grad, nan=7.0))
    assert x.grad.view(-1)[0] == 1.0 and x.grad.view(-1)[1] == 0.0                # a NaN output passes; a masked NaN gradient is 0


def test_bad_arguments_raise():
    from irn_amd import ops
    dev = _dev()
    x = torch.zeros(2, 4, 3, 3, device=dev)
    v = torch.ones(4, device=dev)
    ok = (v, v, v, v, EPS)
    with pytest.raises(ValueError):
        ops.bn_act(x.cpu(), *ok)
    with pytest.raises(ValueError):
        ops.bn_act(x.permute(0, 1, 3, 2)[:, :, :, :2], *ok)                      # not contiguous
    with pytest.raises(ValueError):
        ops.bn_act(x.contiguous(memory_format=torch.channels_last), *ok)         # the training trunk is NCHW
    with pytest.raises(ValueError):
        ops.bn_act(x.double(), *ok)
    off = torch.zeros(2 * 4 * 3 * 3 + 1, device=dev)[1:].view(2, 4, 3, 3)
    assert off.data_ptr() % 16 == 4
    with pytest.raises(ValueError):
        ops.bn_act(off, *ok)                                                      # not 16-byte aligned
    with pytest.raises(ValueError):
        ops.bn_act(x, *ok, residual=off)
    with pytest.raises(ValueError):
        ops.bn_act(x, torch.ones(3, device=dev), v, v, v, EPS)
    with pytest.raises(ValueError):
        ops.bn_act(x, v, v, v.cpu(), v, EPS)
    with pytest.raises(ValueError):
        ops.bn_act(x, *ok, residual=torch.zeros(2, 4, 3, 2, device=dev))
    with pytest.raises(ValueError):
        ops.bn_act(x, *ok, residual_bn=ok)                                        # no residual
    with pytest.raises(ValueError):
        ops.bn_act(x, *ok, residual=x.clone(), residual_bn=(v, v, v, torch.ones(5, device=dev), EPS))
    with pytest.raises(ValueError):
        ops.bn_fold(v, v, v, torch.ones(5, device=dev), EPS)
    empty = ops.bn_act(torch.zeros(0, 4, 3, 3, device=dev, requires_grad=True), v.clone().requires_grad_(True), v, v, v, EPS)
    assert empty.shape == (0, 4, 3, 3)
    empty.sum().backward()


def test_apply_routes_through_the_fused_tail_only_when_the_switch_is_on(monkeypatch):
    from irn_amd.net import resnet50 as R
    dev = _dev()
    torch.manual_seed(3)
    unit = R.Bottleneck(16, 8, stride=2, project=True).to(dev).train()
    with torch.no_grad():
        for m in unit.modules():
            if isinstance(m, R.FrozenBatchNorm):
                m.running_mean.normal_()
                m.running_var.uniform_(0.3, 2.0)
                m.weight.uniform_(-1.0, 1.5)
                m.bias.normal_()
    x = torch.randn(3, 16, 19, 23, device=dev)
    g = torch.randn(3, 32, 10, 12, device=dev)

    def run(fused):
        monkeypatch.setattr(R, "TRAIN_FUSED_TAIL", fused)
        unit.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        y = unit(xi)
        y.backward(g)
        return y, xi.grad, {k: p.grad.clone() for k, p in unit.named_parameters()}

    y0, gx0, p0 = run(False)
    assert type(y0.grad_fn).__name__ == "ReluBackward0"
    y1, gx1, p1 = run(True)
    assert type(y1.grad_fn).__name__.startswith("_BnAct")
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    assert rel(y1, y0) < 1e-6 and rel(gx1, gx0) < 1e-5
    assert p0.keys() == p1.keys() and all(rel(p1[k], p0[k]) < 1e-5 for k in p0), {k: rel(p1[k], p0[k]) for k in p0}
    # no_grad: the inference path, whatever the switch says; an offset view: the composed ops
    monkeypatch.setattr(R, "TRAIN_FUSED_TAIL", True)
    bn = unit.bn3
    off = torch.zeros(3 * 32 * 4 * 5 + 1, device=dev)[1:].view(3, 32, 4, 5).requires_grad_(True)
    assert type(bn.apply_(off, relu=True).grad_fn).__name__ == "ReluBackward0"
    with torch.no_grad():
        z = torch.randn(3, 32, 4, 5, device=dev)
        assert bn.apply_(z, relu=True).data_ptr() == z.data_ptr()
