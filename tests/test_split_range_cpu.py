"""The split-precision operands at both ends of fp16's range, without a GPU (tests/_split_ref.py; irn_amd/gemm.py split_weight,
irn_amd/csrc/split16.hip restated on the host): the product of the fp16 operands, summed exactly, stays within

    2^-21 S_exact + 2^-36 |w_row|_1 + 2^-25 alpha |x_row|_1

of the exact expression in every magnitude band and for both weight forms — and the two defects the GPU test
(test_gpu_split_range.py) is there to see, flushed fp16 subnormals and a lost lo' block, leave that bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _split_ref as R  # noqa: E402

SHAPES = [(8, 12), (256, 64), (2048, 64)]
ROWS = 64
_CACHE = {}


def _case(cin, cout, form, band):
    """(x, w, a16, b16, alpha, exact value, bound), made once per case and left unchanged."""
    key = (cin, cout, form, band)
    if key not in _CACHE:
        from irn_amd import gemm
        gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + R.BANDS.index(band) + 100 * R.WEIGHT_FORMS.index(form))
        x, w = R.band_rows(band, ROWS, cin, gen), R.band_weight(form, cout, cin, gen)
        b16, alpha = gemm.split_weight(w)
        want, S, w_l1, x_l1 = R.exact(x, w)
        _CACHE[key] = (x, w, R.split16_host(x), b16, alpha, want, R.representation_bound(S, w_l1, x_l1, alpha))
    return _CACHE[key]


@pytest.mark.parametrize("band", R.BANDS)
@pytest.mark.parametrize("form", R.WEIGHT_FORMS)
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_operand_product_is_within_the_representation_bound_in_every_band(cin, cout, form, band):
    x, w, a16, b16, alpha, want, bound = _case(cin, cout, form, band)
    lo, hi = R.BAND_RANGE[band]
    nz = x[x != 0].abs()
    assert float(nz.min()) >= lo * (1 - 1e-6) and float(nz.max()) <= hi * (1 + 1e-6) and 0.05 < float((x == 0).float().mean()) < 0.2
    if band == "huge":
        assert float(x.max()) == R.FP16_MAX and float(x.min()) == -R.FP16_MAX
    assert bool(torch.isfinite(a16.float()).all()) and bool(torch.isfinite(b16.float()).all())
    got, _ = R.operand_model(a16, b16, alpha)
    ratio = float(((got - want).abs() / bound).max())
    print("cin %d cout %d %s %s: worst |operand model - exact| / bound = %.3f" % (cin, cout, form, band, ratio))
    assert bool(((got - want).abs() <= bound).all()), (cin, cout, form, band, ratio)


def _flush_subnormals(a16):
    return torch.where(a16.float().abs() < 2.0 ** -14, torch.zeros_like(a16), a16)


@pytest.mark.parametrize("form", R.WEIGHT_FORMS)
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_flushed_subnormal_activations_leave_the_bound_by_two_orders(cin, cout, form):
    """A GEMM that reads fp16 subnormal operands as zero: the `tiny` band is then off by more than 100 times the bound."""
    x, w, a16, b16, alpha, want, bound = _case(cin, cout, form, "tiny")
    got, _ = R.operand_model(_flush_subnormals(a16), b16, alpha)
    ratio = float(((got - want).abs() / bound).max())
    print("cin %d cout %d %s tiny, subnormal operands flushed: %.0f times the bound" % (cin, cout, form, ratio))
    assert ratio > 100.0


@pytest.mark.parametrize("form", R.WEIGHT_FORMS)
@pytest.mark.parametrize("cin,cout", SHAPES[:2])
def test_a_lost_low_block_leaves_the_bound_in_the_unit_band(cin, cout, form):
    """The lo' block read as zero (a wrong column block, a wrong k): 11 bits of the activation are gone."""
    x, w, a16, b16, alpha, want, bound = _case(cin, cout, form, "unit")
    broken = a16.clone()
    broken[:, 2 * cin:] = 0
    got, _ = R.operand_model(broken, b16, alpha)
    ratio = float(((got - want).abs() / bound).max())
    print("cin %d cout %d %s unit, lo' block zeroed: %.1f times the bound" % (cin, cout, form, ratio))
    assert ratio > 1.0


def test_the_3x3_model_is_the_convolution_of_the_reconstructed_operands():
    """`operand_model_3x3` on a bordered operand, in both weight layouts, equals F.conv2d of hi + 2^-11 lo' with (w_hi + w_lo) alpha
    plus the cross term it keeps — the row offsets (ky-1)(w+2) + (kx-1) and the tap order are the kernel's."""
    import torch.nn.functional as F
    from irn_amd import gemm
    gen = torch.Generator().manual_seed(5)
    n, c, cout, h, w = 2, 8, 16, 3, 4
    x = torch.cat([R.band_rows(b, h * w, c, gen) for b in ("unit", "small")]).view(n, h, w, c)
    wt = R.band_weight("flat", cout, c, gen, taps=9)
    a = R.split16_host(x.reshape(-1, c)).view(n, h, w, 3 * c)
    a_pad = torch.zeros(n, h + 2, w + 2, 3 * c, dtype=torch.float16)
    a_pad[:, 1:-1, 1:-1] = a
    hi, lo = a[..., :c].double().permute(0, 3, 1, 2), a[..., 2 * c:].double().permute(0, 3, 1, 2)
    vals = []
    for fused in (True, False):
        saved, gemm.CONV3X3_ROW_FUSED = gemm.CONV3X3_ROW_FUSED, fused
        try:
            w16, alpha = gemm.split_weight_3x3(wt)
        finally:
            gemm.CONV3X3_ROW_FUSED = saved
        taps = R.taps_of(w16).double()                                               # [9, cout, 3c]
        k = lambda blk: taps[:, :, blk * c:(blk + 1) * c].view(3, 3, cout, c).permute(2, 3, 0, 1)
        want = alpha * (F.conv2d(hi, k(0) + k(1), None, 1, 1) + F.conv2d(lo, k(2), None, 1, 1))
        got, S = R.operand_model_3x3(a_pad.view(-1, 3 * c), w16, alpha, n, h, w)
        got = got.view(n, h, w, cout).permute(0, 3, 1, 2)
        assert float((got - want).abs().max()) <= 2.0 ** -40 * float(S.max())
        vals.append(got)
    assert torch.equal(vals[0], vals[1])
