"""The fp16-range flag of the split pass, attributed per sample (irn_split16 with pixels_per_sample, irn_split16_pad with per_sample;
irn_amd/csrc/split16.hip, irn_amd/gemm.py `sample_flags`, net/resnet50.run_rows): bit 0 of flags[s] is set exactly when a value of
sample s — the value that is split, after batch norm and ReLU — is beyond 65504 or NaN; the fp16 output is the bits of the call
without per-sample flags and the process-wide flag stays clear.

  kernel level   5 samples of 3 x 5 pixels: 600 eight-channel pieces at 64 channels = three 256-thread blocks with sample boundaries
                 inside a block; again at 8 channels, where one piece is a whole row.  The dense pass and every (in_padded,
                 out_padded) form of the padded one; an inf in the border of a bordered input flags nothing.
  trunk level    a Bottleneck(256, 64) inside `ops.split_sample_flags`, alone and through `run_rows` in passes of 2 rows: the fill
                 row's word is dropped with its output.
No input here is invalid memory or an invalid call: NaN and inf are data."""
import pytest
import torch

pytestmark = pytest.mark.gpu

INF, NAN, FP16_MAX = float("inf"), float("nan"), 65504.0
N, H, W = 5, 3, 5
FORMS = ["dense", "pad_dense_dense", "pad_dense_bordered", "pad_bordered_dense", "pad_bordered_bordered"]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _nchw(rows, n, h, w):
    return _cl(rows.view(n, h, w, -1).permute(0, 3, 1, 2))


def _global_flag(dev):
    from irn_amd import gemm
    return int(gemm._split_flag(dev).item())


def _bordered(rows, n, h, w, border):
    c = rows.shape[1]
    out = torch.empty(n, h + 2, w + 2, c, dtype=rows.dtype)
    out[:] = border
    out[:, 1:-1, 1:-1] = rows.view(n, h, w, c)
    return out.view(-1, c)


def _run(form, x, c, scale, shift, relu, flags, dev):
    """The split of the rows `x` [N H W, c] in one of the five forms -> its fp16 rows [N H W, 3c] (the interior of a bordered
    output).  A bordered input carries inf in every border row."""
    from irn_amd import ops
    sd, td = (None, None) if scale is None else (scale.to(dev), shift.to(dev))
    if form == "dense":
        return ops.split16(_nchw(x, N, H, W).to(dev), sd, td, relu, flags=flags)
    _, src, dst = form.split("_")
    xin = _bordered(x, N, H, W, INF).to(dev) if src == "bordered" else _nchw(x, N, H, W).to(dev)
    out = None
    if dst == "bordered":
        out = torch.full((N * (H + 2) * (W + 2), 3 * c), 7.0, dtype=torch.float16, device=dev)
    got = ops.split16_pad(xin, (N, c, H, W), sd, td, relu, in_padded=src == "bordered", out=out, flags=flags)
    if dst == "bordered":
        full = got.view(N, H + 2, W + 2, 3 * c)
        border = torch.ones(H + 2, W + 2, dtype=torch.bool, device=dev)
        border[1:-1, 1:-1] = False
        assert not bool((full[:, border] != 0).any()), "border rows are written as zeros"
        return full[:, 1:-1, 1:-1].reshape(-1, 3 * c)
    return got


def _cases(c):
    """(name, rows [N H W, c], scale, shift, relu, expected flags).  Values are otherwise within +-300."""
    gen = torch.Generator().manual_seed(17 + c)
    pps = H * W
    base = (torch.rand(N * pps, c, generator=gen) * 2 - 1) * 300.0
    one = lambda v: torch.full((c,), float(v))
    out = []
    x = base.clone()
    x[4 * pps - 1, c - 1] = 70000.0             # the last channel of the last pixel of sample 3
    x[0, 0] = -70000.0                          # the first element of sample 0
    out.append(("two samples beyond the range", x, None, None, False, [1, 0, 0, 1, 0]))
    x = base.clone()
    x[4 * pps + 7, c // 2] = NAN
    out.append(("a NaN in sample 4", x, None, None, False, [0, 0, 0, 0, 1]))
    x = base.clone()
    x[2 * pps, 0], x[3 * pps - 1, c - 1] = FP16_MAX, -FP16_MAX
    out.append(("65504 itself is inside", x, None, None, False, [0, 0, 0, 0, 0]))
    x = base.clone()
    x[2 * pps + 3, 1] = 1e3                     # 1e3 * 100 = 1e5 after the batch norm
    out.append(("a small input times a large scale", x, one(100.0), one(0.0), True, [0, 0, 1, 0, 0]))
    x = base.clone()
    x[1 * pps + 2, c - 1] = -7e4                # ReLU takes it to 0
    out.append(("a large negative value under ReLU", x, one(1.0), one(0.0), True, [0, 0, 0, 0, 0]))
    x = base.clone()
    x[1 * pps + 2, c - 1] = -7e4                # ... and without ReLU it is split as it is
    out.append(("the same without ReLU", x, one(1.0), one(0.0), False, [0, 1, 0, 0, 0]))
    return out


@pytest.mark.parametrize("c", [64, 8])
@pytest.mark.parametrize("form", FORMS)
def test_flags_name_the_samples_that_left_the_range(form, c):
    from irn_amd import ops
    dev = _dev()
    assert (N * H * W * c // 8 == 600) == (c == 64)
    ops.split_overflowed()
    for name, x, scale, shift, relu, want in _cases(c):
        flags = torch.zeros(N, dtype=torch.int32, device=dev)
        got = _run(form, x, c, scale, shift, relu, flags, dev)
        assert flags.cpu().tolist() == want, (form, c, name)
        assert _global_flag(dev) == 0, ("the process-wide flag stays clear", form, c, name)
        plain = _run(form, x, c, scale, shift, relu, None, dev)
        assert got.dtype == torch.float16 and torch.equal(got.view(torch.int16), plain.view(torch.int16)), (form, c, name)
        assert ops.split_overflowed() == (sum(want) > 0) and _global_flag(dev) == 0, (form, c, name)


def test_flags_keep_their_other_bits_and_are_checked():
    """Bit 0 is OR-ed in: what a word held before stays.  A flag tensor of another length, type or device is refused."""
    from irn_amd import ops
    dev = _dev()
    c = 64
    name, x, scale, shift, relu, want = _cases(c)[0]
    flags = torch.tensor([2, 4, 0, 6, 8], dtype=torch.int32, device=dev)
    _run("dense", x, c, scale, shift, relu, flags, dev)
    assert flags.cpu().tolist() == [3, 4, 0, 7, 8]
    for bad in (torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.int32)):
        with pytest.raises(ValueError, match="flags"):
            _run("dense", x, c, scale, shift, relu, bad, dev)
        with pytest.raises(ValueError, match="flags"):
            _run("pad_dense_dense", x, c, scale, shift, relu, bad, dev)
    assert not ops.split_overflowed()


# ---- trunk level ----
def _unit(c_in, planes, dev):
    from irn_amd.net import resnet50 as r50
    unit = r50.Bottleneck(c_in, planes, stride=1, project=False).to(dev).eval()
    with torch.no_grad():
        for m in unit.modules():
            if isinstance(m, r50.FrozenBatchNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 2.0)
    return unit


def _split_switches(monkeypatch, r50):
    monkeypatch.setattr(r50, "SPLIT_GEMM", True)
    monkeypatch.setattr(r50, "SPLIT_MIN_PLANES", 64)
    monkeypatch.setattr(r50, "SPLIT_MIN_INPUT", 1 << 20)
    monkeypatch.setattr(r50, "SPLIT_MIN_ROWS_3X3", 1)


def test_a_unit_flags_the_sample_that_overflows_also_through_run_rows(monkeypatch):
    from irn_amd import gemm, ops
    from irn_amd.net import resnet50 as r50
    dev = _dev()
    torch.manual_seed(5)
    unit = _unit(256, 64, dev)
    _split_switches(monkeypatch, r50)
    x = torch.relu(torch.randn(3, 256, 6, 5, device=dev))
    with torch.no_grad():
        handed = lambda t: torch.relu(unit.bn2(unit.conv2(torch.relu(unit.bn1(unit.conv1(t)))))).flatten(1).max(dim=1).values    # the composed modules
        for _ in range(20):                             # scale sample 1 until what ITS split pass is handed passes 65504
            if float(handed(x)[1]) > 2 * FP16_MAX:
                break
            x[1] *= 4.0
        top = handed(x).cpu().tolist()
        assert top[1] > 2 * FP16_MAX and top[0] < FP16_MAX / 2 and top[2] < FP16_MAX / 2, top
        xc = _cl(x)
        ops.split_overflowed()
        flags = torch.zeros(3, dtype=torch.int32, device=dev)
        with ops.split_sample_flags(flags):
            y = unit(xc)
        assert "w3_16" in unit.gemm_params() and flags.cpu().tolist() == [0, 1, 0]
        assert gemm._SAMPLE_FLAGS[0] is None and _global_flag(dev) == 0
        assert bool(torch.isfinite(y[0]).all()) and bool(torch.isfinite(y[2]).all())

        # the same rows in passes of 2: [0, 1] and [2, fill].  The fill row (zeros) is turned into an overflowing sample by a
        # row-wise function, so its scratch word IS set — and must go with its output
        monkeypatch.setattr(r50, "pass_rows", lambda t: 2)
        seen = []

        def fn(chunk):
            seen.append(gemm._SAMPLE_FLAGS[0])
            empty = (chunk.flatten(1) == 0).all(dim=1).view(-1, 1, 1, 1)
            return unit(_cl(torch.where(empty, xc[1:2].expand_as(chunk), chunk)))

        flags = torch.zeros(3, dtype=torch.int32, device=dev)
        with ops.split_sample_flags(flags):
            y2 = r50.run_rows(fn, xc)
        assert y2.shape[0] == 3 and flags.numel() == 3 and flags.cpu().tolist() == [0, 1, 0]
        assert len(seen) == 2 and seen[0].data_ptr() == flags.data_ptr() and seen[0].numel() == 2
        assert seen[1].numel() == 2 and seen[1].cpu().tolist() == [0, 1], "the fill row's word was set, in scratch"
        assert not (flags.data_ptr() <= seen[1].data_ptr() < flags.data_ptr() + 12)
        assert bool(torch.isfinite(y2[0]).all()) and bool(torch.isfinite(y2[2]).all())
        assert gemm._SAMPLE_FLAGS[0] is None and _global_flag(dev) == 0 and not ops.split_overflowed()
