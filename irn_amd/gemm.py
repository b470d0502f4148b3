"""Host side of the hipBLASLt convolutions of the channels-last ResNet-50 trunk (irn_amd/csrc/conv1x1.cpp, split16.hip;
reference net/resnet50.py:34-54 with FixedBatchNorm folded into the operands):
    conv1x1_nhwc                          fp32 GEMM with bias / residual / ReLU in its epilogue
    split16, split_weight, gemm16_nhwc    the split-precision form of the same: fp16 hi/lo operands, fp32 accumulation
    split16_pad, split_weight_3x3, conv3x3_split     3x3 / stride 1 as accumulating split GEMMs on one zero-bordered operand
and their state: the shipped rank table, the per-stream workspace, the fp16 overflow flags (process-wide, or per sample inside `sample_flags`).  `irn_amd.ops` re-exports the
functions; the state lives here only.  GPU tensors in, GPU tensors out; no CPU fallback."""
import contextlib
import ctypes as C
import json
import math
import os
import warnings

import torch

from . import _tuned
from ._lib import _need_cl, _need_cuda, _need_vec, _stream, check, lib

_TABLE = None          # the shipped rank table of this device, read once per process: {"ranks": {problem: rank}, "ranks16", "ranks3x3"}
_WS = {}               # (device index, stream) -> workspace tensor (stream-ordered use)
_N_ALGOS = {}          # (count function, problem) with a non-zero table rank -> length of hipBLASLt's heuristic list in this process
_RANK_WARNED = False


def _rank_table():
    """`irn_amd/data/gemm/<device>-hip<version>.json` (written by tools/conv1x1_tune.py and tools/gemm16_tune.py on a GPU box): for
    the problems listed, which entry of hipBLASLt's heuristic list was fastest.  Problems not listed use entry 0.  The table is
    data, not a timing: every process picks the same kernel for the same problem.  No file, or IRN_GEMM_TABLE=0: empty tables
    (_tuned.warn_missing_shipped_data reports the former); a file that does not hold such tables is an error."""
    global _TABLE
    if _TABLE is None:
        path = os.path.join(_tuned.gemm_table_root(), _tuned.miopen_cache_key() + ".json")
        table = {"ranks": {}, "ranks16": {}, "ranks3x3": {}}
        if os.environ.get("IRN_GEMM_TABLE", "1") != "0" and os.path.exists(path):
            try:
                with open(path) as fh:
                    raw = json.load(fh)
                for name, ranks in table.items():
                    for k, r in raw.get(name, {}).items():
                        if type(r) is not int:
                            raise ValueError("%s[%r] = %r is not an integer" % (name, k, r))
                        ranks[tuple(int(v) for v in k.split(","))] = r
            except (ValueError, AttributeError) as e:          # not JSON, not a dict of dicts, a key or rank that is no integer
                raise ValueError("irn_amd: the GEMM rank table %s is malformed (%s); tools/conv1x1_tune.py and tools/gemm16_tune.py "
                                 "rewrite it, IRN_GEMM_TABLE=0 runs without it" % (path, e)) from e
        _TABLE = table
    return _TABLE


def gemm_ranks():
    """(m, cin, cout, bias, residual, relu) -> entry of hipBLASLt's list for the fp32 1x1 convolutions (tools/conv1x1_tune.py)."""
    return _rank_table()["ranks"]


def gemm_ranks16():
    """(m, k, cout, bias, residual, relu) -> entry for the fp16 operand problems (tools/gemm16_tune.py)."""
    return _rank_table()["ranks16"]


def gemm_ranks3x3():
    """(rows of the bordered operand, cin, cout) -> entry for the row-fused 3x3 split convolution (tools/gemm16_tune.py)."""
    return _rank_table()["ranks3x3"]


def _algo_count(fn, m, k, cout, bias, residual, relu):
    n = C.c_int(0)
    check(fn(int(m), int(k), int(cout), int(bool(bias)), int(bool(residual)), int(bool(relu)), int(lib.irn_conv1x1_workspace_bytes()), C.byref(n)))
    return n.value


def conv1x1_algo_count(m, cin, cout, bias, residual, relu):
    """How many kernels hipBLASLt's heuristic offers for the problem (tools/conv1x1_tune.py times each of them once)."""
    return _algo_count(lib.irn_conv1x1_algo_count, m, cin, cout, bias, residual, relu)


def gemm16_algo_count(m, k, cout, bias, residual, relu):
    """How many kernels hipBLASLt's heuristic offers for the split-precision problem (tools/gemm16_tune.py times each once)."""
    return _algo_count(lib.irn_gemm16_algo_count, m, k, cout, bias, residual, relu)


def _workspace(device):
    """One workspace per (device, stream): GEMMs enqueued on different streams may overlap on the device."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = torch.empty(int(lib.irn_conv1x1_workspace_bytes()), dtype=torch.uint8, device=device)
    return ws


def _table_rank(table, prob, count_fn, device):
    """The table's rank for the 1x1 problem `prob` = (m, k, cout, bias, residual, relu), clamped to what hipBLASLt offers here.
    The table is keyed by architecture / CU count / HIP version only: another hipBLASLt build or workspace size may offer a
    shorter list — then the first pick, with one warning, instead of an error in the middle of a forward."""
    rank = table.get(prob, 0)
    if rank:
        n_algos = _N_ALGOS.get((count_fn, prob))
        if n_algos is None:
            with torch.cuda.device(device):
                n_algos = _N_ALGOS[(count_fn, prob)] = count_fn(*prob)
        if rank >= n_algos:
            global _RANK_WARNED
            if not _RANK_WARNED:
                _RANK_WARNED = True
                warnings.warn("irn_amd: the shipped GEMM rank table names entry %d for the 1x1 convolution m=%d cin=%d cout=%d but "
                              "hipBLASLt offers %d here (another library build?): using its first pick for such problems; "
                              "tools/conv1x1_tune.py rewrites the table" % (rank, prob[0], prob[1], prob[2], n_algos), RuntimeWarning)
            rank = 0
    return rank


def conv1x1_nhwc(x, weight, bias=None, residual=None, relu=False, out=None, algo_rank=None):
    """1x1 convolution (stride 1) of a channels-last activation with bias, residual add and ReLU in the GEMM's epilogue
    (irn_conv1x1_nhwc; reference net/resnet50.py:34-54 with FixedBatchNorm folded into `weight` / `bias`).
    x: GPU fp32 [N, cin, H, W] in torch.channels_last; weight: GPU fp32 [cout, cin] (or [cout, cin, 1, 1]) contiguous;
    bias: GPU fp32 [cout] or None; residual: like the result, or None; out: a channels-last [N, cout, H, W] tensor to write
    (may be `residual`), else a fresh one.  -> act(conv(x, weight) + bias (+ residual))."""
    _need_cuda(x, "x")
    _need_cl(x, "conv1x1_nhwc: x")
    n, cin, h, w_ = (int(v) for v in x.shape)
    cout = int(weight.shape[0])
    if weight.dtype != torch.float32 or weight.device != x.device or not weight.is_contiguous() or weight.numel() != cout * cin:
        raise ValueError("conv1x1_nhwc: weight must be a contiguous fp32 [%d-out, %d] tensor on %s" % (cout, cin, x.device))
    if bias is not None:
        _need_vec(bias, "conv1x1_nhwc: bias", cout, x.device)
    shape = (n, cout, h, w_)
    for name, t in (("residual", residual), ("out", out)):
        if t is not None:
            _need_cl(t, "conv1x1_nhwc: " + name, shape, x.device)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    m = n * h * w_
    if m == 0:
        return out
    ws = _workspace(x.device)
    if algo_rank is None:
        algo_rank = _table_rank(gemm_ranks(), (m, cin, cout, int(bias is not None), int(residual is not None), int(bool(relu))),
                                conv1x1_algo_count, x.device)
    with torch.cuda.device(x.device):
        check(lib.irn_conv1x1_nhwc(x.data_ptr(), weight.data_ptr(), None if bias is None else bias.data_ptr(),
                                   None if residual is None else residual.data_ptr(), out.data_ptr(), m, cin, cout,
                                   1 if relu else 0, int(algo_rank), ws.data_ptr(), ws.numel(), _stream()))
    return out


# ---- split-precision convolutions: fp16 hi/lo operands, fp32 accumulation ----
_SPLIT_FLAGS = {}      # device index -> uint32 [1] device tensor: bit 0 = an activation left fp16's range in irn_split16
# three GEMMs over 9 cin (row-fused) instead of nine over 3 cin: IRN_CONV3X3_ROW_FUSED=0 keeps the nine
CONV3X3_ROW_FUSED = os.environ.get("IRN_CONV3X3_ROW_FUSED", "1") != "0"
_ROW_FUSED_REFUSED = False


def _split_flag(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    f = _SPLIT_FLAGS.get(idx)
    if f is None:
        f = _SPLIT_FLAGS[idx] = torch.zeros(1, dtype=torch.int32, device=device)
    return f


def split_overflowed(reset=True):
    """Did any activation handed to `split16` since the last call exceed fp16's range (|x| > 65504) or hold a NaN, on any
    device of this process?  Reads the device flags (synchronises).  The steps check it at the end of every step and raise:
    such a network needs IRN_SPLIT_GEMM=0 (trained ResNet-50 activations stay below a few hundred)."""
    bad = False
    for f in _SPLIT_FLAGS.values():
        if int(f.item()) != 0:
            bad = True
            if reset:
                f.zero_()
    return bad


_SAMPLE_FLAGS = [None]     # the per-sample flag tensor every split pass records into while a `sample_flags` block is open


def _need_flags(flags, n, device, what):
    """`flags` is a contiguous int32 [n] tensor on `device`: one word per sample (leading row) of the activation."""
    if (not isinstance(flags, torch.Tensor) or flags.dtype != torch.int32 or flags.device != device or not flags.is_contiguous()
            or flags.dim() != 1 or flags.numel() != n):
        raise ValueError("%s: flags must be a contiguous int32 [%d] tensor on %s (one word per sample), got %s" % (
            what, n, device, "%s %s on %s" % (flags.dtype, tuple(flags.shape), flags.device) if isinstance(flags, torch.Tensor) else type(flags)))


@contextlib.contextmanager
def sample_flags(flags):
    """Inside the block every `split16` / `split16_pad` / `conv3x3_split` that is not given `flags` of its own records into
    `flags` (int32 [n_samples], bit 0 of word s = a value of sample s left fp16's range or was NaN; the caller zeroes it and
    reads it behind the stream) INSTEAD of the process-wide flag `split_overflowed` reads: a trunk forward — `model(x)` with
    n_samples = x.shape[0] — is instrumented without an argument through every unit.  Every activation split inside must have
    n_samples leading rows.  `flags` None: the block changes nothing.  The former state comes back however the block ends."""
    prev, _SAMPLE_FLAGS[0] = _SAMPLE_FLAGS[0], flags
    try:
        yield flags
    finally:
        _SAMPLE_FLAGS[0] = prev


def split16(x, scale=None, shift=None, relu=False, flags=None):
    """fp32 channels-last activation [N, C, H, W] -> fp16 [N*H*W, 3C] = [hi | hi | lo'] per pixel (irn_split16), the A operand
    of `gemm16_nhwc`; with `scale` / `shift` (fp32 [C]) the inference batch norm (+ ReLU) of the convolution that produced
    `x` is applied on the way (reference net/resnet50.py:40-42) and `x` is never written back.  `flags` (int32 [N], or the
    tensor of an enclosing `sample_flags`): the overflow is recorded per sample there (pixels_per_sample = H*W) and the
    process-wide flag is left alone; the fp16 result is the same bits."""
    _need_cuda(x, "x")
    _need_cl(x, "split16: x")
    n, c, h, w_ = (int(v) for v in x.shape)
    if c % 8:
        raise ValueError("split16: %d channels; a multiple of 8 is needed" % c)
    m = n * h * w_
    out = torch.empty((m, 3 * c), dtype=torch.float16, device=x.device)
    if m == 0:
        return out
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _need_vec(t, "split16: " + name, c, x.device)
    if flags is None:
        flags = _SAMPLE_FLAGS[0]
    sp, tp = None if scale is None else scale.data_ptr(), None if shift is None else shift.data_ptr()
    with torch.cuda.device(x.device):
        per = max(1, (2 ** 31 - 1) // c)                 # at most 2^31 - 1 elements per call
        pps = 0                                          # pixels per sample; 0 = the one process-wide word
        if flags is not None:
            _need_flags(flags, n, x.device, "split16")
            pps = h * w_
            per = per // pps * pps                       # whole samples per call
            if per == 0:
                raise ValueError("split16: a sample of %d x %d elements; per-sample flags need fewer than 2^31 per sample" % (pps, c))
        for i in range(0, m, per):
            word = _split_flag(x.device).data_ptr() if flags is None else flags.data_ptr() + 4 * (i // pps)
            check(lib.irn_split16(x.data_ptr() + 4 * i * c, sp, tp, 1 if relu else 0, out.data_ptr() + 2 * i * 3 * c, min(per, m - i), c,
                                  pps, word, _stream()))
    return out


def gemm16_nhwc(a16, b16, shape, bias=None, residual=None, relu=False, alpha=1.0, out=None, algo_rank=None):
    """act(alpha * a16 . b16^T + bias (+ residual)) as a channels-last fp32 [N, cout, H, W] tensor of `shape` (irn_gemm16_nhwc):
    a16 fp16 [N*H*W, k] from `split16`, b16 fp16 [cout, k] = [w_hi | w_lo | w_hi 2^-11] of the weight scaled by 1 / alpha."""
    _need_cuda(a16, "a16")
    shape = n, cout, h, w_ = tuple(int(v) for v in shape)
    m, k = int(a16.shape[0]), int(a16.shape[1])
    if a16.dtype != torch.float16 or not a16.is_contiguous() or m != n * h * w_:
        raise ValueError("gemm16_nhwc: a16 must be a contiguous fp16 [%d, k] matrix" % (n * h * w_))
    if b16.dtype != torch.float16 or b16.device != a16.device or not b16.is_contiguous() or tuple(b16.shape) != (cout, k):
        raise ValueError("gemm16_nhwc: b16 must be a contiguous fp16 [%d, %d] matrix on %s" % (cout, k, a16.device))
    if bias is not None:
        _need_vec(bias, "gemm16_nhwc: bias", cout, a16.device)
    for name, t in (("residual", residual), ("out", out)):
        if t is not None:
            _need_cl(t, "gemm16_nhwc: " + name, shape, a16.device)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=a16.device, memory_format=torch.channels_last)
    if m == 0:
        return out
    ws = _workspace(a16.device)
    if algo_rank is None:
        algo_rank = _table_rank(gemm_ranks16(), (m, k, cout, int(bias is not None), int(residual is not None), int(bool(relu))),
                                gemm16_algo_count, a16.device)
    with torch.cuda.device(a16.device):
        check(lib.irn_gemm16_nhwc(a16.data_ptr(), b16.data_ptr(), None if bias is None else bias.data_ptr(),
                                  None if residual is None else residual.data_ptr(), out.data_ptr(), m, k, cout,
                                  1 if relu else 0, float(alpha), int(algo_rank), ws.data_ptr(), ws.numel(), _stream()))
    return out


def _weight_exponent(w64):
    top = float(w64.abs().max())
    return 13 - int(math.floor(math.log2(top))) if top > 0 else 0


def split_weight(w64, p=None):
    """Weight [cout, cin] (float64, batch norm folded in) -> (b16 fp16 [cout, 3 cin] = [w_hi | w_lo | w_hi 2^-11] of w 2^p, alpha =
    2^-p): p puts the largest |w 2^p| into [2^13, 2^14), so that w_lo = fp16(w 2^p - w_hi) <= 8 stays a normal fp16 number for
    every weight above 2^-17 of the largest (smaller ones contribute below the fp32 rounding of the sum).  `p` given: the
    exponent of a larger tensor this one is a slice of (the taps of a 3x3 weight share one)."""
    w64 = w64.detach().double()
    if p is None:
        p = _weight_exponent(w64)
    ws = w64 * (2.0 ** p)
    hi = ws.to(torch.float16)
    lo = (ws - hi.double()).to(torch.float16)
    hi_s = (hi.double() * 2.0 ** -11).to(torch.float16)
    return torch.cat([hi, lo, hi_s], dim=1).contiguous(), 2.0 ** -p


def split_weight_3x3(w64):
    """3x3 weight [cout, cin, 3, 3] (float64) -> (fp16 [9, cout, 3 cin]: one `split_weight` operand per tap (ky, kx) in raster
    order, one common exponent, alpha)."""
    w64 = w64.detach().double()
    p = _weight_exponent(w64)
    taps = [split_weight(w64[:, :, ky, kx], p)[0] for ky in range(3) for kx in range(3)]
    if CONV3X3_ROW_FUSED:      # [3, cout, 9 cin]: the three taps of a kernel row side by side (irn_conv3x3_split_gemm row_fused)
        return torch.stack([torch.cat(taps[3 * ky:3 * ky + 3], dim=1) for ky in range(3)]).contiguous(), 2.0 ** -p
    return torch.stack(taps).contiguous(), 2.0 ** -p


def split16_pad(x, shape, scale=None, shift=None, relu=False, in_padded=False, out=None, flags=None):
    """`split16` between a dense map and its zero-bordered form (irn_split16_pad).  shape = (n, c, h, w) of the DENSE map.
    in_padded: `x` is the bordered fp32 form [n (h+2)(w+2), c] (a `conv3x3_split` result), the result is the dense fp16
    [n h w, 3c]; `out` given (a bordered fp16 buffer's interior view, borders already zero): `x` is a dense channels-last fp32
    tensor and the split goes into the bordered form, zero border rows included.  `flags`: as in `split16`, one word per image
    (per_sample = 1)."""
    n, c, h, w_ = (int(v) for v in shape)
    _need_cuda(x, "x")
    if c % 8:
        raise ValueError("split16_pad: %d channels; a multiple of 8 is needed" % c)
    if in_padded:
        if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != n * (h + 2) * (w_ + 2) * c:
            raise ValueError("split16_pad: x must be the contiguous bordered fp32 form of a %s map" % (shape,))
    else:
        _need_cl(x, "split16_pad: x", (n, c, h, w_))
    out_padded = out is not None
    if out is None:
        out = torch.empty((n * h * w_, 3 * c), dtype=torch.float16, device=x.device)
    elif out.dtype != torch.float16 or not out.is_contiguous() or out.numel() < n * (h + 2) * (w_ + 2) * 3 * c:
        raise ValueError("split16_pad: out must be a contiguous fp16 buffer of the bordered form (its border rows are written too)")
    if n * h * w_ == 0:
        return out
    if flags is None:
        flags = _SAMPLE_FLAGS[0]
    if flags is not None:
        _need_flags(flags, n, x.device, "split16_pad")
    with torch.cuda.device(x.device):
        check(lib.irn_split16_pad(
            x.data_ptr(), None if scale is None else scale.data_ptr(), None if shift is None else shift.data_ptr(),
            1 if relu else 0, out.data_ptr(), n, h, w_, c, 1 if in_padded else 0, 1 if out_padded else 0,
            0 if flags is None else 1, (_split_flag(x.device) if flags is None else flags).data_ptr(), _stream()))
    return out


def conv3x3_split(x, w16, alpha, algo_rank=None):
    """3x3 / stride 1 / pad 1 convolution (no bias) of a channels-last fp32 activation [N, C, H, W] in the split-precision form,
    WITHOUT materialising an im2col operand: the activation is split once into a zero-bordered fp16 matrix [N (H+2)(W+2), 3C]
    (irn_split16_pad writes the borders too); there tap (ky, kx) is the same matrix shifted by (ky-1)(W+2) + (kx-1) rows, so the
    convolution is nine fp16 GEMMs accumulating in fp32 in a fixed order (irn_conv3x3_split_gemm, one call).  w16 =
    `split_weight_3x3` fp16 [9, cout, 3C].  -> the result in the bordered fp32 form [N (H+2)(W+2), cout] (border rows hold
    garbage; `split16_pad(..., in_padded=True)` reads the interior).  Reference: conv2 of Bottleneck.forward, net/resnet50.py:40."""
    _need_cuda(x, "x")
    n, c, h, w_ = (int(v) for v in x.shape)
    cout = int(w16.shape[1])
    fused = int(w16.shape[0]) == 3
    if tuple(w16.shape) not in ((9, cout, 3 * c), (3, cout, 9 * c)) or w16.dtype != torch.float16 or not w16.is_contiguous() or w16.device != x.device:
        raise ValueError("conv3x3_split: w16 must be a contiguous fp16 [9, cout, %d] or [3, cout, %d] tensor on %s" % (3 * c, 9 * c, x.device))
    m_pad, guard = n * (h + 2) * (w_ + 2), w_ + 3
    a_buf = torch.empty((m_pad + 2 * guard, 3 * c), dtype=torch.float16, device=x.device)        # guard rows: valid memory, any content
    out = torch.empty((m_pad, cout), dtype=torch.float32, device=x.device)
    if m_pad == 0:
        return out
    split16_pad(x, (n, c, h, w_), out=a_buf[guard:])
    ws = _workspace(x.device)
    rank = algo_rank
    if rank is None:
        # not through `_table_rank`: irn_conv3x3_split_gemm itself takes entry 0 for a rank outside hipBLASLt's list
        rank = gemm_ranks3x3().get((m_pad, c, cout), 0) if fused else gemm_ranks16().get((m_pad, 3 * c, cout, 0, 1, 0), 0)
    global _ROW_FUSED_REFUSED
    with torch.cuda.device(x.device):
        if fused and not _ROW_FUSED_REFUSED:
            rc = lib.irn_conv3x3_split_gemm(a_buf[guard:].data_ptr(), w16.data_ptr(), out.data_ptr(), n, h, w_, c, cout, float(alpha), 1, int(rank),
                                            ws.data_ptr(), ws.numel(), _stream())
            if rc == 0:
                return out
            # this hipBLASLt build does not take an operand with overlapping rows: the nine-GEMM form computes the same sums
            _ROW_FUSED_REFUSED = True
            warnings.warn("irn_amd: hipBLASLt refused the row-fused 3x3 operand (%s); using nine GEMMs per 3x3 convolution (~7 %% slower "
                          "backbones)" % lib.irn_last_error().decode(errors="replace"), RuntimeWarning)
        if fused:                                   # [3, cout, 9c] -> [9, cout, 3c]: the same taps, one per GEMM
            w16 = w16.view(3, cout, 3, 3 * c).permute(0, 2, 1, 3).reshape(9, cout, 3 * c).contiguous()
            rank = 0
        check(lib.irn_conv3x3_split_gemm(a_buf[guard:].data_ptr(), w16.data_ptr(), out.data_ptr(), n, h, w_, c, cout, float(alpha), 0, int(rank),
                                         ws.data_ptr(), ws.numel(), _stream()))
    return out
