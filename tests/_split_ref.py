"""References for the split-precision GEMMs at both ends of fp16's range (irn_split16, irn_split16_pad, irn_gemm16_nhwc,
irn_conv3x3_split_gemm; irn_amd/csrc/split16.hip, conv1x1.cpp, irn_amd/gemm.py): plain torch in float64 on the CPU.

    split16_host     the split kernel restated: hi = fp16(y), lo' = fp16((y - hi) 2^11), row = [hi | hi | lo']
    operand_model    act(alpha a16 . b16^T + bias + residual) from the fp16 operands themselves: products of two fp16 numbers are
                     exact in fp64, so what is left between this and the GPU is the GEMM alone — subnormal operands, accumulation,
                     alpha, the epilogue (and, for the 3x3, the row addressing)
    exact            the same expression from the fp32 activation and the fp64 weight: what is left between this and the operand
                     model is the 22-bit representation alone
Both return the sum of absolute values `S` their error bounds are stated in.  `band_rows` / `band_weight` make the inputs: one
magnitude band per ROW of the activation, so that an output element's S has the band's own scale and an error confined to a band
cannot hide behind ordinary-sized neighbours."""
import math

import torch

FP16_MAX = 65504.0
BANDS = ("tiny", "small", "unit", "huge", "mixed")
# tiny: hi is an fp16 subnormal below 6.1e-5, lo' is subnormal throughout; huge: lo' reaches 2^15
BAND_RANGE = {"tiny": (1e-7, 1.2e-4), "small": (1.2e-4, 1e-2), "unit": (0.1, 10.0), "huge": (3e4, FP16_MAX), "mixed": (1e-7, FP16_MAX)}
WEIGHT_FORMS = ("flat", "rows")


def band_rows(band, rows, cin, gen):
    """fp32 [rows, cin]: magnitudes log-uniform in the band, random signs, a tenth of the entries exact zeros; `huge` holds
    +65504 (first entry) and -65504 (last entry) themselves."""
    lo, hi = BAND_RANGE[band]
    u = torch.rand(rows, cin, generator=gen, dtype=torch.float64)
    mag = torch.exp(math.log(lo) + u * (math.log(hi) - math.log(lo))).clamp(lo, hi)
    sign = torch.where(torch.rand(rows, cin, generator=gen) < 0.5, -1.0, 1.0).double()
    zero = torch.rand(rows, cin, generator=gen) < 0.1
    x = torch.where(zero, torch.zeros((), dtype=torch.float64), mag * sign).float()
    x = torch.where(x.abs() > FP16_MAX, torch.sign(x) * FP16_MAX, x)          # (1.2e-4 and 65504 round to fp32 inside the band or onto its end)
    if band == "huge":
        x.view(-1)[0], x.view(-1)[-1] = FP16_MAX, -FP16_MAX
    return x


def band_weight(form, cout, cin, gen, taps=1):
    """float64 [cout, cin] (or [cout, cin, 3, 3] with taps = 9).  flat: folded-batch-norm-sized, randn / sqrt(fan-in) * 0.05;
    rows: the same with output channel o scaled by 2^-(o mod 24) — folded scales spanning 2^23 under ONE shared exponent p."""
    shape = (cout, cin) if taps == 1 else (cout, cin, 3, 3)
    w = torch.randn(shape, generator=gen, dtype=torch.float64) / math.sqrt(cin * taps) * 0.05
    if form == "rows":
        s = 2.0 ** -(torch.arange(cout, dtype=torch.float64) % 24)
        w = w * s.view((-1,) + (1,) * (len(shape) - 1))
    return w


def bn_relu_host(x, scale, shift, relu):
    """y = fmaf(x, scale, shift) (+ ReLU) as the kernel forms it, for inputs whose x scale + shift is EXACT in fp64 (`exact_bn_inputs`):
    the single rounding of fmaf is then the fp64 value rounded once.  x fp32 [rows, c]."""
    y = (x.double() * scale.double() + shift.double()).float()
    return torch.where(y < 0, torch.zeros_like(y), y) if relu else y            # the kernel's `y < 0 ? 0 : y`: NaN and -0 pass


def split16_host(y):
    """fp32 [rows, c] -> fp16 [rows, 3c] = [hi | hi | lo'], every step an IEEE fp32 / fp16 operation as in split16_kernel."""
    hi = y.to(torch.float16)
    lo = ((y - hi.float()) * 2048.0).to(torch.float16)
    return torch.cat([hi, hi, lo], dim=1)


def fp16_bits(t):
    """fp16 tensor -> int16 bit patterns with every NaN mapped to ONE pattern: +-0, +-inf and every finite value compare bit for
    bit; which NaN an invalid operation (inf - inf) returns — sign and payload — is the platform's choice, not the model's."""
    bits = t.contiguous().view(torch.int16).clone()
    bits[torch.isnan(t)] = 0x7E00
    return bits


def exact_bn_inputs(rows, c, gen):
    """(x [rows, c], scale [c], shift [c]) fp32 whose x scale + shift is exact in fp64, 12 significant bits each.  Odd channels:
    exponents of x and scale within 2^+-6, of shift within 2^+-12 — the product has 24 bits above 2^-35, the sum stays below 2^14:
    49 bits.  Even channels: shift 0 and exponents of x and scale from 2^-12 to 2^6 — the product is an fp32 number between 2^-24
    and 2^14, so that the batch norm's output reaches the subnormal end too."""
    def q(shape, lo, hi):
        m = torch.randint(2 ** 11, 2 ** 12, shape, generator=gen).double() * 2.0 ** -11              # [1, 2), 12 bits
        ex = torch.randint(lo, hi + 1, shape, generator=gen).double()
        sg = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).double()
        return m * 2.0 ** ex * sg
    even = (torch.arange(c) % 2 == 0)
    x = torch.where(even, q((rows, c), -12, 6), q((rows, c), -6, 6)).float()
    scale = torch.where(even, q((c,), -12, 6), q((c,), -6, 6)).float()
    shift = torch.where(even, torch.zeros(c, dtype=torch.float64), q((c,), -12, 12)).float()
    prod = x.double() * scale.double()
    s = prod + shift.double()
    bb = s - prod
    assert bool((((prod - (s - bb)) + (shift.double() - bb)) == 0).all()), "x scale + shift must be exact in fp64"
    return x, scale, shift


def epilogue(val, S, bias, residual, relu):
    if bias is not None:
        val, S = val + bias.double().view(1, -1), S + bias.double().abs().view(1, -1)
    if residual is not None:
        val, S = val + residual.double(), S + residual.double().abs()
    return (val.clamp_min(0) if relu else val), S


def operand_model(a16, b16, alpha, bias=None, residual=None, relu=False):
    """a16 fp16 [m, k] as read back from the device, b16 fp16 [cout, k] from `split_weight`; bias fp32 [cout], residual fp32
    [m, cout].  -> (value, S) float64 [m, cout], S = alpha |a16| . |b16|^T + |bias| + |residual|."""
    a, b = a16.double(), b16.double()
    return epilogue(alpha * (a @ b.t()), alpha * (a.abs() @ b.abs().t()), bias, residual, relu)


def taps_of(w16):
    """`split_weight_3x3`'s operand in either layout -> [9, cout, 3c], tap (ky, kx) at 3 ky + kx."""
    if w16.shape[0] == 9:
        return w16
    cout, c3 = int(w16.shape[1]), int(w16.shape[2]) // 3
    return w16.view(3, cout, 3, c3).permute(0, 2, 1, 3).reshape(9, cout, c3)


def interior_rows(n, h, w):
    """Row numbers of the interior pixels of the bordered form [n, h + 2, w + 2], image by image in raster order."""
    r = torch.arange(n * (h + 2) * (w + 2)).view(n, h + 2, w + 2)
    return r[:, 1:-1, 1:-1].reshape(-1)


def operand_model_3x3(a16_pad, w16, alpha, n, h, w):
    """a16_pad fp16 [n (h+2)(w+2), 3c]: the bordered operand as read back; w16 from `split_weight_3x3`.  Tap (ky, kx) is the
    operand shifted by (ky-1)(w+2) + (kx-1) rows; summed over the INTERIOR rows only (every shifted row of those is inside the
    operand).  -> (value, S) float64 [n h w, cout]."""
    a, taps = a16_pad.double(), taps_of(w16).double()
    rows = interior_rows(n, h, w)
    val = S = 0.0
    for ky in range(3):
        for kx in range(3):
            at, bt = a[rows + (ky - 1) * (w + 2) + (kx - 1)], taps[3 * ky + kx]
            val, S = val + at @ bt.t(), S + at.abs() @ bt.abs().t()
    return alpha * val, alpha * S


def exact(x, w, bias=None, residual=None, relu=False):
    """x fp32 [m, cin], w float64 [cout, cin] -> (value, S_exact = |x| . |w|^T + |bias| + |residual|, l1 norm of every weight row
    [cout], l1 norm of every activation row [m]), float64."""
    xd, wd = x.double(), w.double()
    val, S = epilogue(xd @ wd.t(), xd.abs() @ wd.abs().t(), bias, residual, relu)
    return val, S, wd.abs().sum(1), xd.abs().sum(1)


def representation_bound(S_exact, w_l1, x_l1, alpha):
    """|operand_model - exact| <= 2^-21 S_exact + 2^-36 |w_row|_1 + 2^-25 alpha |x_row|_1, element by element: the 22 bits of both
    sides plus the dropped x_lo w_lo; the absolute floor of a subnormal lo' (2^-25 / 2^11 per activation); that of a subnormal
    w_lo (2^-25 of the scaled weight)."""
    return 2.0 ** -21 * S_exact + 2.0 ** -36 * w_l1.view(1, -1) + 2.0 ** -25 * alpha * x_l1.view(-1, 1)


def accumulation_bound(k, S):
    """|GPU - operand_model| <= (k + 2) 2^-24 S: an fp32 sum of k exact products in ANY order, plus the roundings of alpha and
    of the epilogue."""
    return (k + 2) * 2.0 ** -24 * S
