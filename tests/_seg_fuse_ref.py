"""numpy restatement of `irn_seg_fuse` (include/irn_hip.h) — the oracle of `ops.seg_fuse`.

The taps are computed in float32 exactly as irn_amd/csrc/upsample.hpp states them: rs = (float)((double)Hs / ((double)stride * H)),
s = rs * (o + 0.5f) - 0.5f clamped at 0, i0 = (int)s, l = s - i0, i1 = i0 + 1 clamped to n - 1.  The blend, the softmax, the sum
over the maps and the division by their number are float64.  `emulate=True` runs everything in float32 in the kernel's order of
operations instead (a CPU emulation of the kernel, for the expectation of its distance from the float64 form)."""
import numpy as np

F32 = np.float32


def ratio(size, stride, out):
    return F32(np.float64(size) / (np.float64(stride) * np.float64(out)))


def taps(n_out, n, rs):
    """(i0, i1, l) of every output index of an axis with `n` inputs read at ratio `rs`: int64, int64, float32 arrays."""
    rs = F32(rs)
    o = np.arange(n_out, dtype=np.int64).astype(F32)
    s = (rs * (o + F32(0.5))).astype(F32) - F32(0.5)
    s = np.where(s < 0, F32(0), s).astype(F32)
    i0 = s.astype(np.int64)
    assert int(i0.max()) <= n - 1, "tap %d past an axis of %d inputs (ratio %r, %d outputs)" % (int(i0.max()), n, rs, n_out)
    i1 = i0 + (i0 < n - 1)
    return i0, i1, (s - i0.astype(F32)).astype(F32)


def integer_factor_taps(n_out, n, factor):
    """The same for the integer-factor upsampling of irn_upsample_bilinear: rscale = (float)(1.0 / factor)."""
    return taps(n_out, n, F32(1.0 / np.float64(factor)))


def upsample(logits, size, stride, out_hw, dtype=np.float64):
    """z [C,H,W] of one map [C,h,w] computed from a rescaled image of `size` = (Hs, Ws)."""
    x = np.asarray(logits, F32)
    (hh, ww), (_, h, w) = out_hw, x.shape
    y0, y1, ly = taps(hh, h, ratio(size[0], stride, hh))
    x0, x1, lx = taps(ww, w, ratio(size[1], stride, ww))
    x = x.astype(dtype)
    one = dtype(1)
    ly, lx = ly.astype(dtype)[:, None], lx.astype(dtype)[None, :]
    ly0, lx0 = (one - ly).astype(dtype), (one - lx).astype(dtype)       # exact in float32: l in [0, 1)
    a, b = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    c, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    with np.errstate(invalid="ignore"):
        return (ly0 * (lx0 * a + lx * b).astype(dtype)).astype(dtype) + (ly * (lx0 * c + lx * d).astype(dtype)).astype(dtype)


def fuse(maps, sizes, stride, out_hw, emulate=False):
    """P [C,H,W]: float64, or float32 in the kernel's order of operations with `emulate`."""
    dtype = F32 if emulate else np.float64
    total = None
    with np.errstate(invalid="ignore", over="ignore"):
        for logits, size in zip(maps, sizes):
            z = upsample(logits, size, stride, out_hw, dtype)
            e = np.exp((z - np.fmax.reduce(z, axis=0, keepdims=True)).astype(dtype)).astype(dtype)
            s = np.zeros(z.shape[1:], dtype)
            for c in range(z.shape[0]):
                s = (s + e[c]).astype(dtype)
            p = (e * (dtype(1) / s).astype(dtype)).astype(dtype) if emulate else e / s
            total = p if total is None else (total + p).astype(dtype)
        return (total * dtype(1.0 / len(maps))).astype(dtype) if emulate else total / len(maps)


def labels_of(p):
    """The first class that attains the maximum, a NaN counting as the maximum (np.argmax's rule, and torch's); uint8 [H,W]."""
    return np.argmax(p, axis=0).astype(np.uint8)


def top2_gap(p):
    s = np.sort(p, axis=0)
    return s[-1] - s[-2]


def touched(n_out, n, rs, cell):
    """Outputs of an axis one of whose taps is `cell`, whatever its weight: bool [n_out]."""
    i0, i1, _ = taps(n_out, n, rs)
    return (i0 == cell) | (i1 == cell)


def case_maps(shape, seed=0):
    """(maps, sizes) of a test shape (H, W, C, scales, stride): random normal x 3 logits of ceil(Hs / stride) cells, Hs the
    np.round of H * scale."""
    hh, ww, c, scales, stride = shape
    rng = np.random.RandomState(seed)
    maps, sizes = [], []
    for s in scales:
        hs, ws = int(np.round(hh * s)), int(np.round(ww * s))
        maps.append((3 * rng.standard_normal((c, -(-hs // stride), -(-ws // stride)))).astype(F32))
        sizes.append((hs, ws))
    return maps, sizes
