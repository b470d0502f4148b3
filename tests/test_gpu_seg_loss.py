"""The fused upsample / softmax cross-entropy (irn_amd/csrc/seg_loss.hip, `ops.seg_loss_sums`, `ops.seg_cross_entropy`,
`ops.seg_argmax`) on the GPU against tests/_seg_loss_ref.py: counts exactly; sums and gradients as close to the fp64
restatement as the composed fp32 path on the same device, within a factor of 4; void-only images; logits of +-1e4 and NaN;
identical bits call after call, alone and inside a batch; every gradient element written; the arg-max bit-equal to
torch.argmax of `ops.upsample_bilinear`; and the second call queued behind a lagging device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lag as L  # noqa: E402
import _seg_loss_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR = 4.0               # fused error <= FACTOR * composed error (the factor of --cam_fused_tail's test)
IDS = ["%dx%dx%dx%d_f%d_%dx%d" % s for s in R.SHAPES]
_CASES = {}


def _dev():
    return torch.device("cuda", 0)


def _case(i):
    """The inputs of shape i, the fp64 restatement and the composed fp32 path on the device: computed once, never changed."""
    if i not in _CASES:
        shape = R.SHAPES[i]
        x, label, coef = R.make_case(shape, seed=100 + i)
        f = shape[4]
        _CASES[i] = {"shape": shape, "x": x, "label": label, "coef": coef, "f": f,
                     "ref": R.sums_counts_grad(x, label, f, coef),
                     "composed": R.sums_counts_grad(x, label, f, coef, torch.float32, _dev())}
    return _CASES[i]


def _fused(x, label, f, coef=None):
    """-> (sums, counts, grad) of the fused path, on the host."""
    from irn_amd import ops
    xs = x.to(_dev()).requires_grad_(True)
    sums, counts = ops.seg_loss_sums(xs, label.to(_dev()), f)
    cf = torch.ones_like(sums) if coef is None else coef.to(_dev(), torch.float64)
    (sums * cf).sum().backward()
    return sums.detach().cpu(), counts.cpu(), xs.grad.cpu()


def _rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def _rel_each(a, ref):
    return [abs(float(p) - float(q)) / abs(float(q)) for p, q in zip(a.double(), ref.double())]


def measure(i):
    """{'shape', 'grad': (fused, composed), 'sums': [(fused, composed) per image]}: relative errors against fp64."""
    c = _case(i)
    rs, _, rg = c["ref"]
    cs, _, cg = c["composed"]
    fs, _, fg = _fused(c["x"], c["label"], c["f"], c["coef"])
    return {"shape": list(c["shape"]), "grad": (_rel_l2(fg, rg), _rel_l2(cg, rg)),
            "sums": list(zip(_rel_each(fs, rs), _rel_each(cs, rs)))}


@pytest.mark.parametrize("i", range(len(R.SHAPES)), ids=IDS)
def test_counts_exact_sums_and_gradients_within_4x_of_the_composed_error(i):
    c = _case(i)
    _, counts, _ = _fused(c["x"], c["label"], c["f"], c["coef"])
    assert torch.equal(counts, c["ref"][1])
    m = measure(i)
    print("\n%s: gradient rel. L2 error against fp64: fused %.3e, composed %.3e" % ((IDS[i],) + m["grad"]))
    for b, (ef, ec) in enumerate(m["sums"]):
        print("%s: sums[%d] |d|/|ref|: fused %.3e, composed %.3e" % (IDS[i], b, ef, ec))
    assert m["grad"][1] > 0, "the composed gradient is exact here: the input measures nothing"
    assert m["grad"][0] <= FACTOR * m["grad"][1]
    for b, (ef, ec) in enumerate(m["sums"]):
        assert ec > 0, "the composed sum of image %d is exact here: the input measures nothing" % b
        assert ef <= FACTOR * ec, "sums[%d]: fused %.3e against composed %.3e" % (b, ef, ec)


def test_all_void_gives_zero_counts_zero_sums_and_exactly_zero_gradients():
    from irn_amd import ops
    x, _, _ = R.make_case(R.SHAPES[1], seed=7)
    label = torch.full((2, 24, 40), 255, dtype=torch.uint8)
    sums, counts, grad = _fused(x, label, 8)
    assert counts.tolist() == [0, 0] and sums.tolist() == [0.0, 0.0]
    assert torch.equal(grad, torch.zeros_like(grad))
    xs = x.to(_dev()).requires_grad_(True)
    loss = ops.seg_cross_entropy(xs, label.to(_dev()), 8)
    loss.backward()
    assert float(loss.detach()) == 0.0 and torch.equal(xs.grad.cpu(), torch.zeros_like(x))


def test_one_void_image_of_two():
    x, label, coef = R.make_case(R.SHAPES[1], seed=8)
    label[1] = 255
    _, rc, _ = R.sums_counts_grad(x, label, 8, coef)
    sums, counts, grad = _fused(x, label, 8, coef)
    assert torch.equal(counts, rc) and counts[1] == 0 and counts[0] > 0
    assert float(sums[1]) == 0.0 and torch.equal(grad[1], torch.zeros_like(grad[1]))
    assert torch.isfinite(sums[0]) and float(sums[0]) > 0 and torch.isfinite(grad[0]).all() and grad[0].abs().max() > 0
    alone = _fused(x[:1], label[:1], 8, coef[:1])
    assert torch.equal(alone[0][0], sums[0]) and torch.equal(alone[2][0], grad[0])


def test_logits_of_1e4_stay_finite_and_within_the_rule():
    shape = R.SHAPES[1]
    x, label, coef = R.make_case(shape, seed=9)
    x = torch.where(x > 0, torch.full_like(x, 1e4), torch.full_like(x, -1e4))
    rs, rc, rg = R.sums_counts_grad(x, label, 8, coef)
    cs, _, cg = R.sums_counts_grad(x, label, 8, coef, torch.float32, _dev())
    fs, fc, fg = _fused(x, label, 8, coef)
    assert torch.isfinite(fs).all() and torch.isfinite(fg).all() and torch.equal(fc, rc)
    eg, ecg = _rel_l2(fg, rg), _rel_l2(cg, rg)
    print("\n+-1e4: gradient: fused %.3e, composed %.3e" % (eg, ecg))
    assert eg <= FACTOR * ecg
    for b, (ef, ec) in enumerate(zip(_rel_each(fs, rs), _rel_each(cs, rs))):
        print("+-1e4: sums[%d]: fused %.3e, composed %.3e" % (b, ef, ec))
        assert ef <= FACTOR * ec


def test_a_nan_logit_gives_a_nan_sum_for_its_image_only():
    x, label, _ = R.make_case(R.SHAPES[1], seed=10)
    label = torch.randint(0, 21, label.shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    clean = _fused(x, label, 8)
    x[1, 4, 1, 2] = float("nan")
    sums, counts, grad = _fused(x, label, 8)
    assert torch.isnan(sums[1]) and torch.equal(sums[0], clean[0][0]) and torch.equal(counts, clean[1])
    assert torch.equal(grad[0], clean[2][0]) and torch.isnan(grad[1]).any()


@pytest.mark.parametrize("i", [1, 3], ids=[IDS[1], IDS[3]])
def test_five_calls_give_identical_bits(i):
    c = _case(i)
    first = _fused(c["x"], c["label"], c["f"], c["coef"])
    for _ in range(4):
        again = _fused(c["x"], c["label"], c["f"], c["coef"])
        assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_an_image_alone_and_inside_a_batch_of_three_has_the_same_bits():
    c = _case(3)
    assert c["shape"][0] == 3
    whole = _fused(c["x"], c["label"], c["f"], c["coef"])
    for b in range(3):
        alone = _fused(c["x"][b:b + 1], c["label"][b:b + 1], c["f"], c["coef"][b:b + 1])
        assert torch.equal(alone[0][0], whole[0][b]) and torch.equal(alone[1][0], whole[1][b])
        assert torch.equal(alone[2][0], whole[2][b])


@pytest.mark.parametrize("i", [0, 2, 3, 6], ids=[IDS[0], IDS[2], IDS[3], IDS[6]])
def test_the_backward_writes_every_element(i):
    """irn_seg_loss_backward into a buffer prefilled with NaN, called at the C tier (the autograd tier allocates its own)."""
    from irn_amd._lib import _stream, check, lib
    c = _case(i)
    B, C, h, w, f, H, W = c["shape"]
    x, label = c["x"].to(_dev()), c["label"].to(_dev())
    need = lib.irn_seg_loss_workspace_bytes(B, C, h, w, f, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())
    sums = torch.empty(B, dtype=torch.float64, device=_dev())
    counts = torch.empty(B, dtype=torch.int64, device=_dev())
    lse = torch.empty(B, H, W, dtype=torch.float64, device=_dev())
    coef = c["coef"].to(_dev())
    grad = torch.full_like(x, float("nan"))
    check(lib.irn_seg_loss_forward(x.data_ptr(), label.data_ptr(), B, C, h, w, f, H, W, sums.data_ptr(), counts.data_ptr(),
                                   lse.data_ptr(), ws.data_ptr(), need, _stream()))
    check(lib.irn_seg_loss_backward(x.data_ptr(), label.data_ptr(), lse.data_ptr(), coef.data_ptr(), B, C, h, w, f, H, W,
                                    grad.data_ptr(), ws.data_ptr(), need, _stream()))
    assert not torch.isnan(grad).any()
    assert torch.equal(grad.cpu(), _fused(c["x"], c["label"], f, c["coef"])[2])


def _argmax_ref(x, f, H, W):
    from irn_amd import ops
    return torch.argmax(ops.upsample_bilinear(x, f)[..., :H, :W], 1)


@pytest.mark.parametrize("i", range(len(R.SHAPES)), ids=IDS)
def test_seg_argmax_is_bit_equal_to_argmax_of_the_upsampled_logits(i):
    from irn_amd import ops
    c = _case(i)
    H, W = c["shape"][5:]
    x = c["x"].to(_dev())
    out = ops.seg_argmax(x, c["f"], (H, W))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (c["shape"][0], H, W)
    assert torch.equal(out.long(), _argmax_ref(x, c["f"], H, W))


def test_seg_argmax_ties_go_to_the_first_channel_and_nan_is_the_maximum():
    from irn_amd import ops
    x = torch.zeros(1, 5, 3, 4)
    x[0, 1], x[0, 3] = 2.0, 2.0              # constant planes: channels 1 and 3 tie everywhere
    x[0, 0, :, :2] = 2.0                     # ... and channel 0 ties with them on the left
    xd = x.to(_dev())
    out = ops.seg_argmax(xd, 8, (24, 32))
    assert torch.equal(out.long(), _argmax_ref(xd, 8, 24, 32))
    assert set(out.unique().tolist()) == {0, 1}
    y = torch.randn(2, 6, 3, 4, generator=torch.Generator().manual_seed(3))
    y[1, 4, 1, 1] = float("nan")
    y[1, 2, 1, 2] = float("nan")
    yd = y.to(_dev())
    out = ops.seg_argmax(yd, 8, (24, 30))
    assert torch.equal(out.long(), _argmax_ref(yd, 8, 24, 30))
    assert (out[1] == 4).any() and (out[1] == 2).any()


def test_second_call_behind_a_lagging_device_gives_the_same_bits():
    """seg_cross_entropy forward and backward twice while the device is still busy with a stall: the second call's workspace,
    sums and log-sum-exp buffers are its own, so both give the bits of a call on an idle device."""
    from irn_amd import ops
    c = _case(3)
    label, x = c["label"].to(_dev()), c["x"].to(_dev())     # (an upload from pageable memory would wait for the stall)

    def once():
        xs = x.clone().requires_grad_(True)
        loss = ops.seg_cross_entropy(xs, label, c["f"])
        loss.backward()
        return loss.detach(), xs.grad

    (idle, host_ms) = L.timed(once)
    torch.cuda.synchronize()
    results, b = L.run_behind([("first", once), ("second", once)], L.stall_ms_for(host_ms), gap_ms=3.0)
    lagged = b.lags["second"].before
    torch.cuda.synchronize()
    b.report("seg_cross_entropy twice")
    assert lagged, "the device had caught up before the second call: the stall was too short to test anything"
    for loss, grad in results:
        assert torch.equal(loss, idle[0]) and torch.equal(grad, idle[1])
