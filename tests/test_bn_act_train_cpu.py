"""The host half of the fused training tail (ops.bn_act) without a GPU: the parameter gradients `ops.bn_param_grads` forms
from the channel sums of `irn_bn_act_backward` — grad_weight = (S1 - mean * S0) / sqrt(var + eps), grad_bias = S0 — against
fp64 autograd of the composed ops (F.batch_norm(training=False) -> add -> ReLU with the mask held fixed), the new entry
points' argument checks, the new flags and the module switch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_act_train_ref as B  # noqa: E402

EPS = 1e-5


def _case(shape, seed, mean_scale=1.0, var_lo=0.05, var_hi=3.0):
    """fp32-representable inputs (so that fp64 autograd and the function under test see the same numbers)."""
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    t = {"mean": torch.randn(c, generator=g) * mean_scale, "var": torch.rand(c, generator=g) * (var_hi - var_lo) + var_lo,
         "weight": torch.randn(c, generator=g), "bias": torch.randn(c, generator=g),
         "r_mean": torch.randn(c, generator=g) * mean_scale, "r_var": torch.rand(c, generator=g) * (var_hi - var_lo) + var_lo,
         "r_weight": torch.randn(c, generator=g), "r_bias": torch.randn(c, generator=g)}
    view = (1, -1) + (1,) * (len(shape) - 2)
    t["x"] = torch.randn(shape, generator=g) * t["var"].sqrt().view(view) + t["mean"].view(view)
    t["res"] = torch.randn(shape, generator=g) * t["r_var"].sqrt().view(view) + t["r_mean"].view(view)
    t["grad_out"] = torch.randn(shape, generator=g)
    return t


CASES = {
    "plain": dict(shape=(3, 5, 7, 9), seed=1),
    "var_near_zero": dict(shape=(2, 6, 5, 5), seed=2, var_lo=1e-12, var_hi=1e-9),           # eps dominates: 1 / sqrt(..) ~ 316
    "large_mean": dict(shape=(2, 4, 11, 3), seed=3, mean_scale=1e4),                        # S1 - mean * S0 cancels ~4 digits
    "large_mean_small_var": dict(shape=(4, 3, 6, 6), seed=4, mean_scale=3e3, var_lo=1e-6, var_hi=1e-4),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("mode", ["plain", "residual", "residual_bn"])
def test_parameter_gradients_equal_fp64_autograd_of_the_composed_ops(case, mode):
    """Bound: the function works in double from double sums and rounds ONCE to fp32, so against the fp64 value it is off by
    the rounding of that cast, |want| * 2^-24, plus what two fp64 evaluations of the same sum in different orders may differ
    by: n * 2^-52 * sum |terms|, with the terms of S1 - mean * S0 scaled by 1 / sqrt(var + eps)."""
    from irn_amd import ops
    t = _case(**CASES[case])
    d = {k: v.double() for k, v in t.items()}
    for k in ("weight", "bias", "r_weight", "r_bias"):
        d[k].requires_grad_(True)
    y = F.batch_norm(d["x"], d["mean"], d["var"], d["weight"], d["bias"], False, 0.0, EPS)
    if mode == "residual":
        y = y + d["res"]
    elif mode == "residual_bn":
        y = y + F.batch_norm(d["res"], d["r_mean"], d["r_var"], d["r_weight"], d["r_bias"], False, 0.0, EPS)
    mask = (y.detach() > 0)
    (y * mask).backward(d["grad_out"])                                           # ReLU with the mask held fixed

    (s0, s1, s2), (m0, m1, m2) = B.sums(t["grad_out"].numpy(), mask.numpy(), t["x"].numpy(), t["res"].numpy() if mode == "residual_bn" else None)
    n = t["x"].numel() // t["x"].shape[1]
    layers = [("weight", "bias", s1, m1, "mean", "var")]
    if mode == "residual_bn":
        layers.append(("r_weight", "r_bias", s2, m2, "r_mean", "r_var"))
    for wk, bk, s_x, m_x, mk, vk in layers:
        gw, gb = ops.bn_param_grads(torch.from_numpy(s0), torch.from_numpy(s_x), t[mk], t[vk], EPS)
        assert gw.dtype == torch.float32 and gb.dtype == torch.float32
        want_w, want_b = d[wk].grad.numpy(), d[bk].grad.numpy()
        inv = 1.0 / np.sqrt(t[vk].double().numpy() + EPS)
        tol_w = np.abs(want_w) * 2.0 ** -24 + 2 * n * 2.0 ** -52 * (m_x + np.abs(t[mk].double().numpy()) * m0) * inv
        tol_b = np.abs(want_b) * 2.0 ** -24 + 2 * n * 2.0 ** -52 * m0
        err_w, err_b = np.abs(gw.double().numpy() - want_w), np.abs(gb.double().numpy() - want_b)
        print("\n%s / %s %s: worst grad_weight error / bound %.3f, grad_bias %.3f" % (case, mode, wk, float((err_w / (tol_w + 1e-300)).max()),
                                                                                      float((err_b / (tol_b + 1e-300)).max())))
        assert (err_w <= tol_w).all() and (err_b <= tol_b).all()
        # and the restatement says the same
        ref_w, ref_b = B.param_grads(s0, s_x, t[mk].numpy(), t[vk].numpy(), EPS)
        assert np.array_equal(gw.numpy(), ref_w.astype(np.float32)) and np.array_equal(gb.numpy(), ref_b.astype(np.float32))


def test_restated_input_gradients_equal_fp64_autograd():
    """grad_x = dz * scale and grad_res = dz * res_scale of the restatement against autograd, to fp64 rounding."""
    t = _case((2, 5, 4, 6), 9)
    d = {k: v.double() for k, v in t.items()}
    d["x"].requires_grad_(True)
    d["res"].requires_grad_(True)
    y = (F.batch_norm(d["x"], d["mean"], d["var"], d["weight"], d["bias"], False, 0.0, EPS)
         + F.batch_norm(d["res"], d["r_mean"], d["r_var"], d["r_weight"], d["r_bias"], False, 0.0, EPS))
    mask = y.detach() > 0
    (y * mask).backward(d["grad_out"])
    scale = (d["weight"] / torch.sqrt(d["var"] + EPS)).detach().numpy()
    r_scale = (d["r_weight"] / torch.sqrt(d["r_var"] + EPS)).detach().numpy()
    gx, gr = B.grads(t["grad_out"].numpy(), mask.numpy(), scale, r_scale)
    np.testing.assert_allclose(gx, d["x"].grad.numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(gr, d["res"].grad.numpy(), rtol=1e-14, atol=0)
    assert np.array_equal(B.relu_mask(np.array([1.0, 0.0, -0.0, -1.0, np.nan])), [True, False, False, False, True])


def test_argument_validation_of_the_training_tail_entry_points():
    from irn_amd import _lib
    L = _lib.lib
    one = C.c_void_p(64)                                                       # never dereferenced on these paths
    assert L.irn_bn_fold(None, one, one, one, 1e-5, 4, one, one, None) == 1 and b"irn_bn_fold" in L.irn_last_error()
    assert L.irn_bn_fold(one, one, one, one, 1e-5, 0, one, one, None) == 1
    assert L.irn_bn_act_forward(one, None, one, one, None, None, None, 1, 4, 16, 1, None) == 1 and b"irn_bn_act_forward" in L.irn_last_error()
    assert L.irn_bn_act_forward(one, None, one, one, None, None, C.c_void_p(4164), 1, 4, 16, 1, None) == 1   # out not 16-byte aligned
    assert L.irn_bn_act_forward(one, None, one, one, None, None, C.c_void_p(128), 1, 4, 16, 1, None) == 1 and b"overlaps" in L.irn_last_error()
    assert L.irn_bn_act_forward(one, None, one, one, one, one, C.c_void_p(4160), 1, 4, 16, 1, None) == 1     # residual constants, no residual
    assert L.irn_bn_act_forward(one, None, one, one, None, None, C.c_void_p(1 << 40), 1 << 20, 2048, 4096, 1, None) == 1 and b"2^31" in L.irn_last_error()
    assert L.irn_bn_act_forward(one, None, one, one, None, None, C.c_void_p(4160), 0, 4, 16, 1, None) == 0   # empty batch
    assert L.irn_bn_act_backward(None, one, one, None, one, None, one, None, one, 1, 4, 16, 1, one, 1 << 20, None) == 1
    assert b"irn_bn_act_backward" in L.irn_last_error()
    assert L.irn_bn_act_backward(one, None, one, None, one, None, one, None, None, 1, 4, 16, 1, None, 0, None) == 1 and b"mask" in L.irn_last_error()
    assert L.irn_bn_act_backward(one, one, one, None, None, None, one, None, None, 1, 4, 16, 1, None, 0, None) == 1 and b"scale" in L.irn_last_error()
    assert L.irn_bn_act_backward(one, one, None, None, one, None, None, None, one, 1, 4, 16, 1, one, 1 << 20, None) == 1   # sums without x
    assert L.irn_bn_act_backward(one, one, one, None, one, one, None, None, one, 1, 4, 16, 1, one, 1 << 20, None) == 1     # S2 without res
    assert L.irn_bn_act_backward(one, one, one, None, one, None, None, None, one, 1, 4, 16, 1, one, 8, None) == 1 and b"workspace" in L.irn_last_error()
    assert L.irn_bn_act_backward(one, one, one, None, one, None, C.c_void_p(68), None, None, 1, 4, 16, 1, None, 0, None) == 1   # alignment
    assert L.irn_bn_act_backward(one, one, one, None, one, None, one, None, None, 1 << 20, 2048, 4096, 1, None, 0, None) == 1 and b"2^31" in L.irn_last_error()
    assert L.irn_bn_act_backward(one, one, one, None, one, None, None, None, None, 1, 4, 16, 1, None, 0, None) == 0        # nothing asked for
    # the workspace: three sums x channels x shares of 4096 elements, 8 bytes each
    assert L.irn_bn_act_backward_workspace_bytes(16, 256, 32 * 32) == 3 * 256 * 4 * 8         # four 1024-element planes per share
    assert L.irn_bn_act_backward_workspace_bytes(16, 256, 64 * 64) == 3 * 256 * 16 * 8
    assert L.irn_bn_act_backward_workspace_bytes(2, 2, 70 * 70) == 3 * 2 * 4 * 8              # two chunks per plane
    assert L.irn_bn_act_backward_workspace_bytes(5, 3, 40 * 40) == 3 * 3 * 3 * 8              # 2 + 2 + 1 images
    assert L.irn_bn_act_backward_workspace_bytes(0, 4, 16) == 0 and L.irn_bn_act_backward_workspace_bytes(1 << 20, 2048, 4096) == 0


def test_bn_act_refuses_cpu_tensors():
    from irn_amd import ops
    x = torch.zeros(2, 4, 3, 3)
    v = torch.ones(4)
    with pytest.raises(ValueError):
        ops.bn_act(x, v, v, v, v, 1e-5)
    with pytest.raises(ValueError):
        ops.bn_fold(v, v, v, v, 1e-5)


def test_flags_and_the_module_switch():
    import run_train
    import run_train_cam
    from irn_amd.net import resnet50 as R
    assert R.TRAIN_FUSED_TAIL is False
    base = ["--voc12_root", "VOC2012"]
    a = run_train.build_parser().parse_args(base)
    assert a.irn_trunk == "autograd"
    assert run_train.build_parser().parse_args(base + ["--irn_trunk", "inference"]).irn_trunk == "inference"
    with pytest.raises(SystemExit):
        run_train.build_parser().parse_args(base + ["--irn_trunk", "fast"])
    assert "2 rows" in run_train.build_parser().format_help()                  # the untuned-crop caveat is in the help text
    c = run_train_cam.build_parser().parse_args(base)
    assert c.cam_fused_tail == 0 and run_train_cam.build_parser().parse_args(base + ["--cam_fused_tail", "1"]).cam_fused_tail == 1
    # with the switch on, the CPU (and any tensor the kernel cannot take) still runs the composed ops
    bn = R.FrozenBatchNorm(4)
    x = torch.randn(2, 4, 3, 3, requires_grad=True)
    want = F.relu(bn(x))
    R.TRAIN_FUSED_TAIL = True
    try:
        got = bn.apply_(x, relu=True)
    finally:
        R.TRAIN_FUSED_TAIL = False
    assert torch.equal(got, want) and got.requires_grad


def test_irn_forward_is_trunk_then_heads_and_forward_train_matches_it_on_the_cpu():
    """`Net.forward` split into `trunk` and `heads`; `forward_train` (trunk under no_grad) gives the same outputs and the
    same head gradients on the CPU, where there is one code path, and no trunk parameter gets a gradient."""
    from irn_amd.net import weights
    from irn_amd.net.resnet50_irn import Net
    model = Net()
    model.load_state_dict(weights.random_irn_state(), strict=False)
    model.train()
    x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    outs = {}
    for name in ("forward", "forward_train"):
        model.zero_grad(set_to_none=True)
        edge, dp = getattr(model, name)(x)
        assert edge.grad_fn is not None and dp.grad_fn is not None
        (edge.sum() + dp.sum()).backward()
        outs[name] = (edge.detach(), dp.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        assert outs[name][2] and all(k.startswith(("fc_edge", "fc_dp")) for k in outs[name][2])
    a, b = outs["forward"], outs["forward_train"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].keys() == b[2].keys()
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    f = model.trunk(x)
    assert len(f) == 6 and f[5] is False and not any(t.requires_grad for t in f[:5])
