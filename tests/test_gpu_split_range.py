"""The split-precision GEMMs at both ends of fp16's range (irn_split16, irn_split16_pad, irn_gemm16_nhwc, irn_conv3x3_split_gemm;
irn_amd/csrc/split16.hip, conv1x1.cpp, irn_amd/gemm.py; reference net/resnet50.py:34-54): activations from 1e-7, where hi and lo'
are both fp16 subnormals, to 65504, where lo' reaches 2^15, one magnitude band per row of the operand (tests/_split_ref.py).

  (a) the split kernel, dense and bordered, equals its host restatement bit for bit at the edges, with and without batch norm;
  (b) the overflow flag follows the value that is split, in the last interior pixel, and ignores the bordered input's border;
  (c) irn_gemm16_nhwc against the exact sum of the products of the fp16 operands it was given: (k + 2) 2^-24 S per element;
  (d) the same for the 3x3 in both forms, on the bordered operand as read back;
  (e) guard rows of the 3x3 operand cannot reach an interior result;
  (f) a unit sets the flag and the step check raises, once.
No input here is invalid memory or an invalid call: NaN and inf are data."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _split_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _nchw(rows, n, h, w):
    """[n h w, c] rows -> the channels-last [n, c, h, w] tensor whose memory they are."""
    return _cl(rows.view(n, h, w, -1).permute(0, 3, 1, 2))


def _rows(t):
    """channels-last [n, c, h, w] -> [n h w, c] on the CPU."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).cpu()


def _flag(dev):
    from irn_amd import gemm
    return int(gemm._split_flag(dev).item())


def _bordered(rows, n, h, w, border):
    """[n h w, c] -> the bordered form [n (h+2)(w+2), c] with `border` (a [c] pattern or a number) in every border row."""
    c = rows.shape[1]
    out = torch.empty(n, h + 2, w + 2, c, dtype=rows.dtype)
    out[:] = border
    out[:, 1:-1, 1:-1] = rows.view(n, h, w, c)
    return out.view(-1, c)


# ---- (a) ----
def _edge_pool(gen):
    nx = float(torch.nextafter(torch.tensor(R.FP16_MAX), torch.tensor(INF)))
    special = [0.0, -0.0, 1e-40, -1e-40, R.FP16_MAX, -R.FP16_MAX, nx, -nx, 65519.0, -65519.0, 65520.0, -65520.0, INF, -INF,
               2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 6.1e-5, 1.2e-4, 2.0 ** -36, 3e-8, 1e-7, 32768.0, NAN]
    bands = torch.cat([R.band_rows(b, 1, 8, gen).view(-1) for b in R.BANDS])
    return torch.cat([torch.tensor(special, dtype=torch.float32), bands])             # 24 + 40 = 64 values


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == torch.float16, what
    assert torch.equal(R.fp16_bits(got), R.fp16_bits(want)), what


@pytest.mark.parametrize("n,c,h,w", [(1, 8, 1, 1), (2, 64, 5, 7), (1, 2048, 2, 3)])
def test_split_kernels_equal_the_host_restatement_bit_for_bit_at_the_edges(n, c, h, w):
    """[hi | hi | lo'] of irn_split16 and of both directions of irn_split16_pad == the host's, as bit patterns (every NaN counted
    as one pattern): all bands, +-0, fp32 subnormals, +-65504 and its neighbours on both sides of the rounding to inf, +-inf.  With
    batch norm (+ ReLU) on inputs whose x scale + shift is exact in fp64 — the kernel's fmaf is then that value rounded once — all
    three blocks again, lo' included."""
    from irn_amd import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(100 * c + h)
    pool = _edge_pool(gen)
    m, numel = n * h * w, n * h * w * c
    m_pad = n * (h + 2) * (w + 2)
    garbage = torch.tensor([NAN, 1e30] * (c // 2))

    def three_ways(y, x, scale=None, shift=None, relu=False, what=""):
        want = R.split16_host(y)
        sd, td = (None, None) if scale is None else (scale.to(dev), shift.to(dev))
        _assert_bits(ops.split16(_nchw(x, n, h, w).to(dev), sd, td, relu).cpu(), want, ("split16", what))
        buf = torch.full((m_pad, 3 * c), 7.0, dtype=torch.float16, device=dev)          # border rows are written as zeros
        ops.split16_pad(_nchw(x, n, h, w).to(dev), (n, c, h, w), sd, td, relu, out=buf)
        _assert_bits(buf.cpu(), _bordered(want, n, h, w, 0.0), ("split16_pad out", what))
        got = ops.split16_pad(_bordered(x, n, h, w, garbage).to(dev), (n, c, h, w), sd, td, relu, in_padded=True)
        _assert_bits(got.cpu(), want, ("split16_pad in_padded", what))

    met = set()
    for rep in range(max(1, math.ceil(len(pool) / numel))):         # the 8-element map sees the pool in pieces
        idx = (torch.arange(numel) * 5 + rep * numel + c) % len(pool)
        met |= set(idx.tolist())
        x = pool[idx].view(m, c)
        three_ways(x, x, what=("plain", rep))
    assert len(met) == len(pool) == 64
    for relu in (True, False):
        x, scale, shift = R.exact_bn_inputs(m, c, gen)
        y = R.bn_relu_host(x, scale, shift, relu)
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) < R.FP16_MAX
        assert m * c < 64 or (bool(((y != 0) & (y.abs() < 2.0 ** -14)).any()) and bool((y.abs() > 1.0).any()))
        three_ways(y, x, scale, shift, relu, what=("bn", relu))
    ops.split_overflowed()          # (inf and 65520 were among the inputs: leave the flag clear)


# ---- (b) ----
@pytest.mark.parametrize("value,scale,relu,trips", [
    (1e3, 100.0, True, True), (7e4, 0.5, True, False), (-7e4, 1.0, True, False), (-1e3, 100.0, False, True),
    (65504.0, None, False, False), (-65504.0, None, False, False), ("next", None, False, True), (NAN, None, False, True),
    (INF, None, False, True), (-INF, None, False, True), (NAN, 1.0, True, True), (-INF, 1.0, True, False)])
def test_the_overflow_flag_follows_the_value_that_is_split(value, scale, relu, trips):
    """The flag is set by |y| > 65504 or NaN with y = the value AFTER batch norm + ReLU, never by x itself; the offending value sits in the
    last channel of the last interior pixel of the last image (three blocks of threads), for irn_split16 and both directions of
    irn_split16_pad.  Reading the bordered form, border rows full of NaN and 1e30 neither set it nor reach the output."""
    from irn_amd import ops
    dev = _dev()
    n, c, h, w = 2, 64, 5, 7
    if value == "next":
        value = float(torch.nextafter(torch.tensor(R.FP16_MAX), torch.tensor(INF)))
    x = torch.ones(n * h * w, c)
    x[-1, -1] = value
    sd = td = None
    if scale is not None:
        sd, td = torch.full((c,), scale, device=dev), torch.zeros(c, device=dev)
    m_pad = n * (h + 2) * (w + 2)
    ops.split_overflowed()
    assert _flag(dev) == 0
    dense = ops.split16(_nchw(x, n, h, w).to(dev), sd, td, relu)
    assert (_flag(dev) != 0) == trips, "split16"
    assert ops.split_overflowed() == trips and _flag(dev) == 0
    buf = torch.empty((m_pad, 3 * c), dtype=torch.float16, device=dev)
    ops.split16_pad(_nchw(x, n, h, w).to(dev), (n, c, h, w), sd, td, relu, out=buf)
    assert ops.split_overflowed() == trips and _flag(dev) == 0, "split16_pad out"
    assert torch.equal(R.fp16_bits(buf.cpu().view(n, h + 2, w + 2, 3 * c)[:, 1:-1, 1:-1].reshape(-1, 3 * c)), R.fp16_bits(dense.cpu()))
    garbage = torch.tensor([NAN, 1e30] * (c // 2))
    got = ops.split16_pad(_bordered(x, n, h, w, garbage).to(dev), (n, c, h, w), sd, td, relu, in_padded=True)
    assert ops.split_overflowed() == trips and _flag(dev) == 0, "split16_pad in_padded"
    assert torch.equal(R.fp16_bits(got.cpu()), R.fp16_bits(dense.cpu()))
    if not trips:
        assert torch.equal(got, dense)


# ---- (c) ----
GEMM_SHAPES = [(8, 12), (256, 64), (2048, 512)]
_GEMM = {}


def _gemm_case(cin, cout, form):
    """Operands, the operand model without an epilogue and the exact expression: made once, shared by the three epilogues."""
    key = (cin, cout, form)
    if key not in _GEMM:
        from irn_amd import ops
        dev = _dev()
        gen = torch.Generator().manual_seed(77 * cin + cout + R.WEIGHT_FORMS.index(form))
        x = torch.cat([R.band_rows(b, 64, cin, gen) for b in R.BANDS])                 # [5 * 64, cin]: image i of (5, cin, 8, 8) is band i
        wt = R.band_weight(form, cout, cin, gen)
        b16, alpha = ops.split_weight(wt.to(dev))
        a16 = ops.split16(_nchw(x, 5, 8, 8).to(dev))
        a_host = a16.cpu()
        tiny = a_host[:64].float().abs()              # `tiny`: hi subnormal below 6.1e-5, lo' subnormal throughout
        assert torch.equal(a_host, R.split16_host(x)) and bool(((tiny[:, :cin] > 0) & (tiny[:, :cin] < 2.0 ** -14)).any()) and bool((tiny[:, 2 * cin:] <= 2.0 ** -14).all())
        val, S = R.operand_model(a_host, b16.cpu(), alpha)
        bias = (torch.randn(cout, generator=gen).double() * S[:64].mean(0)).float()    # of the tiny band's size: swamps no band
        res = (torch.randn(320, cout, generator=gen).double() * S).float()             # of each element's own size
        # S with every non-zero fp16 subnormal counted as 2^-14, the exponent it carries: what the matrix pipe's error scales with
        nominal = lambda t: torch.where((t != 0) & (t.abs() < 2.0 ** -14), torch.full_like(t, 2.0 ** -14), t.abs())
        S_nom = alpha * (nominal(a_host.double()) @ nominal(b16.cpu().double()).t())
        _GEMM[key] = dict(x=x, wt=wt, a16=a16, b16=b16, alpha=alpha, val=val, S=S, S_nom=S_nom, bias=bias, res=res)
    return _GEMM[key]


@pytest.mark.parametrize("bias,residual,relu", [(True, False, True), (True, True, True), (False, False, False)])
@pytest.mark.parametrize("form", R.WEIGHT_FORMS)
@pytest.mark.parametrize("cin,cout", GEMM_SHAPES)
def test_gemm16_equals_the_sum_of_its_operands_products_in_every_band(cin, cout, form, bias, residual, relu):
    """|irn_gemm16_nhwc - operand model| <= (3 cin + 2) 2^-24 S per element: the fp32 bound of ANY summation order plus the roundings
    of alpha and the epilogue.  A GEMM that flushed subnormal operands, or read a wrong column block, is off by more than 100 times
    that in the `tiny` band (test_split_range_cpu.py).  With the representation bound it is within the sum of both of the exact value.

    Measured on an MI355X (hipBLASLt of ROCm 7.0, the shipped rank table), worst err / (2^-24 S) over the three epilogues and both
    weight forms, cin 8 / 256 / 2048: tiny 23.5 / 4.1 / 6.4, small 2.6 / 3.3 / 5.6, unit 2.6 / 4.2 / 5.5, huge 2.0 / 2.3 / 4.3,
    mixed 5.4 / 8.7 / 10.1, against bounds of 26 / 770 / 6146.  fp16 subnormal operands are NOT flushed.  The 23.5 (cin 8, `rows`,
    no epilogue) is no accident of the summation order: the matrix pipe aligns a product by the exponent FIELDS of its operands,
    and a subnormal carries 2^-14 whatever its value, so its error is 2^-24 of S' = S with every subnormal operand counted as 2^-14
    (printed below: at most 1.8 2^-24 S' in every case).  A row of 8 activations that ALL lie far below 6.1e-5 has S' >> S; with
    256 or more channels some entry of the band's upper end carries S.  In absolute terms this is 2^-38 of the layer's largest
    weight per activation (range ends)."""
    from irn_amd import ops
    dev = _dev()
    g = _gemm_case(cin, cout, form)
    b, r = (g["bias"] if bias else None), (g["res"] if residual else None)
    want, S = R.epilogue(g["val"], g["S"], b, r, relu)
    bd, rd = (None if b is None else b.to(dev)), (None if r is None else _nchw(r, 5, 8, 8).to(dev))
    ops.split_overflowed()
    got_d = ops.gemm16_nhwc(g["a16"], g["b16"], (5, cout, 8, 8), bd, rd, relu, g["alpha"])
    assert got_d.shape == (5, cout, 8, 8) and got_d.dtype == torch.float32 and got_d.is_contiguous(memory_format=torch.channels_last)
    got = _rows(got_d).double()
    err = (got - want).abs()
    unit = 2.0 ** -24 * S
    for i, band in enumerate(R.BANDS):
        e, u = err[64 * i:64 * i + 64], unit[64 * i:64 * i + 64]
        ratio = float(torch.where(u > 0, e / u.clamp_min(1e-300), (e > 0).double() * 1e30).max())
        print("gemm16 cin %d cout %d %s bias %d residual %d relu %d, %s: worst err / (2^-24 S) = %.3f (bound %d)"
              % (cin, cout, form, bias, residual, relu, band, ratio, 3 * cin + 2))
    if not bias and not residual:
        print("gemm16 cin %d cout %d %s, tiny: worst err / (2^-24 S') = %.3f with S' counting subnormal operands as 2^-14"
              % (cin, cout, form, float((err[:64] / (2.0 ** -24 * g["S_nom"][:64])).max())))
    assert bool(torch.isfinite(got).all())
    assert bool((err <= R.accumulation_bound(3 * cin, S)).all()), (cin, cout, form)
    exact, S_e, w_l1, x_l1 = R.exact(g["x"], g["wt"], b, r, relu)
    both = R.accumulation_bound(3 * cin, S) + R.representation_bound(S_e, w_l1, x_l1, g["alpha"])
    assert bool(((got - exact).abs() <= both).all()), (cin, cout, form)
    assert torch.equal(got_d, ops.gemm16_nhwc(g["a16"], g["b16"], (5, cout, 8, 8), bd, rd, relu, g["alpha"]))
    assert not ops.split_overflowed()              # 65504 itself is inside the range


# ---- (d) ----
@pytest.mark.parametrize("n,c,cout,h,w", [(5, 8, 8, 1, 1), (5, 64, 32, 5, 7), (5, 128, 128, 6, 6)])
def test_conv3x3_split_equals_the_sum_of_its_operands_products_one_band_per_image(n, c, cout, h, w, monkeypatch):
    """ops.conv3x3_split, row-fused (three GEMMs over 9 cin) and as nine GEMMs, against the operand model on the bordered operand
    irn_split16_pad wrote: (27 cin + 2) 2^-24 S per interior element; the two forms within twice that of each other."""
    from irn_amd import gemm, ops
    dev = _dev()
    gen = torch.Generator().manual_seed(31 * c + h)
    x = torch.cat([R.band_rows(b, h * w, c, gen) for b in R.BANDS])
    xd = _nchw(x, n, h, w).to(dev)
    m_pad, guard = n * (h + 2) * (w + 2), w + 3
    buf = torch.zeros((m_pad + 2 * guard, 3 * c), dtype=torch.float16, device=dev)
    ops.split_overflowed()
    ops.split16_pad(xd, (n, c, h, w), out=buf[guard:])
    a_pad = buf[guard:guard + m_pad].cpu()
    assert torch.equal(a_pad, _bordered(R.split16_host(x), n, h, w, 0.0)) and not bool((buf[:guard] != 0).any()) and not bool((buf[guard + m_pad:] != 0).any())
    rows = R.interior_rows(n, h, w)
    for form in R.WEIGHT_FORMS:
        wt = R.band_weight(form, cout, c, gen, taps=9)
        results = {}
        for fused in (True, False):
            monkeypatch.setattr(gemm, "CONV3X3_ROW_FUSED", fused)
            w16, alpha = ops.split_weight_3x3(wt.to(dev))
            assert tuple(w16.shape) == ((3, cout, 9 * c) if fused else (9, cout, 3 * c))
            want, S = R.operand_model_3x3(a_pad, w16.cpu(), alpha, n, h, w)
            pad = ops.conv3x3_split(xd, w16, alpha)
            assert not gemm._ROW_FUSED_REFUSED and pad.shape == (m_pad, cout)
            got = pad.cpu()[rows].double()
            err, unit = (got - want).abs(), 2.0 ** -24 * S
            per = (h * w)
            for i, band in enumerate(R.BANDS):
                e, u = err[per * i:per * i + per], unit[per * i:per * i + per]
                ratio = float(torch.where(u > 0, e / u.clamp_min(1e-300), (e > 0).double() * 1e30).max())
                print("3x3 %s -> %d %s %s, %s: worst err / (2^-24 S) = %.3f (bound %d)"
                      % ((n, c, h, w), cout, form, "three over 9 cin" if fused else "nine over 3 cin", band, ratio, 27 * c + 2))
            assert bool(torch.isfinite(got).all())
            assert bool((err <= R.accumulation_bound(27 * c, S)).all()), (form, fused)
            assert torch.equal(pad[rows.to(dev)], ops.conv3x3_split(xd, w16, alpha)[rows.to(dev)])
            results[fused] = (got, S)
        assert bool(((results[True][0] - results[False][0]).abs() <= 2.0 * R.accumulation_bound(27 * c, results[True][1])).all()), form
    assert not ops.split_overflowed()


# ---- (e) ----
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("n,c,cout,h,w", [(2, 64, 32, 5, 7), (1, 8, 8, 1, 6)])
def test_guard_rows_of_the_3x3_operand_cannot_reach_an_interior_result(n, c, cout, h, w, fused, monkeypatch):
    """irn_conv3x3_split_gemm called as ops.conv3x3_split calls it, on a buffer whose w + 3 guard rows on either side hold zeros, NaN
    or 65504: the interior rows of the result are the same bits, and irn_split16_pad wrote no guard row."""
    from irn_amd import gemm, ops
    from irn_amd._lib import _stream, check, lib
    dev = _dev()
    gen = torch.Generator().manual_seed(c + w)
    x = torch.cat([R.band_rows("mixed" if i % 2 else "unit", h * w, c, gen) for i in range(n)])
    xd = _nchw(x, n, h, w).to(dev)
    monkeypatch.setattr(gemm, "CONV3X3_ROW_FUSED", fused)
    w16, alpha = ops.split_weight_3x3(R.band_weight("flat", cout, c, gen, taps=9).to(dev))
    m_pad, guard = n * (h + 2) * (w + 2), w + 3
    ws = gemm._workspace(dev)
    rows = R.interior_rows(n, h, w).to(dev)
    outs = []
    ops.split_overflowed()
    for fill in (0.0, NAN, R.FP16_MAX):
        buf = torch.full((m_pad + 2 * guard, 3 * c), fill, dtype=torch.float16, device=dev)
        ops.split16_pad(xd, (n, c, h, w), out=buf[guard:])
        out = torch.full((m_pad, cout), NAN, dtype=torch.float32, device=dev)
        check(lib.irn_conv3x3_split_gemm(buf[guard:].data_ptr(), w16.data_ptr(), out.data_ptr(), n, h, w, c, cout, float(alpha), 1 if fused else 0, 0,
                                         ws.data_ptr(), ws.numel(), _stream()))
        outs.append(out[rows])
        guards = torch.cat([buf[:guard], buf[guard + m_pad:]]).cpu()
        assert torch.equal(R.fp16_bits(guards), R.fp16_bits(torch.full_like(guards, fill))), fill
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0], ops.conv3x3_split(xd, w16, alpha)[rows])
    assert not ops.split_overflowed()


# ---- (f) ----
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


def _split_switches(monkeypatch, r50, on):
    monkeypatch.setattr(r50, "SPLIT_GEMM", on)
    monkeypatch.setattr(r50, "SPLIT_MIN_PLANES", 64)
    monkeypatch.setattr(r50, "SPLIT_MIN_INPUT", 1 << 20)
    monkeypatch.setattr(r50, "SPLIT_MIN_ROWS_3X3", 1)


def test_a_unit_sets_the_flag_and_the_step_check_raises_once(monkeypatch):
    """Bottleneck(256, 64) on the split path with bn2's scale raised until its output passes 65504: the forward sets the device flag,
    `_common.check_split_overflow` raises naming IRN_SPLIT_GEMM=0, and the next check is silent.  The same unit on the fp32 path
    leaves the flag clear and its result finite."""
    from irn_amd import ops
    from irn_amd.net import resnet50 as r50
    from irn_amd.step import _common
    dev = _dev()
    torch.manual_seed(5)
    unit = _unit(256, 64, dev)
    x = _cl(torch.relu(torch.randn(2, 256, 6, 5, device=dev)))
    _split_switches(monkeypatch, r50, True)
    ops.split_overflowed()
    with torch.no_grad():
        y = unit(x)
        assert "w3_16" in unit.gemm_params() and bool(torch.isfinite(y).all())
        assert _flag(dev) == 0
        _common.check_split_overflow("x")               # an ordinary unit: silent
        unit.bn2.weight.mul_(1e6)
        z = unit.bn2(unit.conv2(torch.relu(unit.bn1(unit.conv1(x)))))          # the composed modules: what the split pass is handed
        assert float(z.max()) > R.FP16_MAX
        unit(x)
        assert _flag(dev) != 0
        with pytest.raises(RuntimeError, match="IRN_SPLIT_GEMM=0"):
            _common.check_split_overflow("x")
        _common.check_split_overflow("x")               # reported once
        assert _flag(dev) == 0
        _split_switches(monkeypatch, r50, False)
        y32 = unit(x)
        assert "w3_16" not in unit.gemm_params()
        assert _flag(dev) == 0 and bool(torch.isfinite(y32).all())
        _common.check_split_overflow("x")


def test_the_bordered_3x3_path_of_a_unit_sets_the_flag(monkeypatch):
    """A 128-plane unit whose 3x3 runs as split GEMMs: bn1 scaled up puts conv1's output beyond 65504, and the flag is up when
    `ops.conv3x3_split` returns — set by irn_split16_pad writing the bordered operand."""
    from irn_amd import ops
    from irn_amd.net import resnet50 as r50
    from irn_amd.step import _common
    dev = _dev()
    torch.manual_seed(6)
    unit = _unit(512, 128, dev)
    x = _cl(torch.relu(torch.randn(2, 512, 6, 5, device=dev)))
    _split_switches(monkeypatch, r50, True)
    seen = []
    real = ops.conv3x3_split
    monkeypatch.setattr(ops, "conv3x3_split", lambda *a, **k: (real(*a, **k), seen.append(_flag(dev)))[0])
    ops.split_overflowed()
    with torch.no_grad():
        y = unit(x)
        assert "w2_16" in unit.gemm_params() and "w1_16" not in unit.gemm_params()
        assert seen == [0] and _flag(dev) == 0 and bool(torch.isfinite(y).all())
        unit.bn1.weight.mul_(1e6)
        unit(x)
    assert len(seen) == 2 and seen[1] != 0
    with pytest.raises(RuntimeError, match="IRN_SPLIT_GEMM=0"):
        _common.check_split_overflow("x")
    _common.check_split_overflow("x")
