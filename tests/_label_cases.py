"""Inputs of the label epilogue and the CAM merge at the launch shapes and extremes the smooth synthetic CAMs never reach
(plain numpy, deterministic by seed; shared by tests/test_label_cases_cpu.py and tests/test_gpu_label_epilogue.py).

A label case is ``(rw [C,1,h,w] float32, out_size (H, W), keys int64 [C], bg_thres)``; `label_cases()` returns
``[(name, case), ...]``.  The geometry the cases aim at (irn_amd/csrc/label.hip): source cell (k, l) owns the output rows
4k+2 .. 4k+5 (0 .. 5 for k = 0, up to 4h-1 for k = h-1) and the same in x; the global maximum is searched in the cells
whose largest corner reaches a lower bound taken from one output per cell; the argmax pass handles four output columns
per thread."""
import numpy as np

F32 = np.float32
BG = 0.25


def _keys(c, seed=0):
    return np.sort(np.random.RandomState(1000 + seed).choice(20, c, replace=False)).astype(np.int64)


def _floor(c, h, w, seed):
    """A low positive noise floor: every cell is far below a peak of 1."""
    return np.random.RandomState(seed).uniform(0.01, 0.05, (c, 1, h, w)).astype(F32)


def hot_pixel(c, h, w, seed, pos=None):
    """abs(randn) with one entry x50; the position comes from the seed unless given.  Returns (rw, (ch, y, x))."""
    rng = np.random.RandomState(seed)
    rw = np.abs(rng.randn(c, 1, h, w)).astype(F32)
    if pos is None:
        pos = (int(rng.randint(c)), int(rng.randint(h)), int(rng.randint(w)))
    rw[pos[0], 0, pos[1], pos[2]] *= F32(50)
    return rw, pos


def _corner_cases():
    out = []
    for n, (h, w) in enumerate(((1, 1), (1, 9), (9, 1), (2, 2), (5, 7), (33, 29))):
        spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h - 1, w // 2), (h // 2, w - 1)]
        for y, x in sorted(set(spots)):
            c = 1 + (n + y + x) % 3
            rw = _floor(c, h, w, seed=100 * n + 7 * y + x)
            rw[(y + x) % c, 0, y, x] = F32(1.0)
            out.append(("corner_%dx%d_at_%d_%d" % (h, w, y, x), (rw, (4 * h, 4 * w), _keys(c, n), BG)))
    # the same spots with a crop that keeps only the first of the last cell's two rows / columns
    for y, x in ((32, 28), (32, 14), (16, 28)):
        rw = _floor(2, 33, 29, seed=900 + y + x)
        rw[1, 0, y, x] = F32(1.0)
        out.append(("corner_33x29_at_%d_%d_crop" % (y, x), (rw, (4 * 33 - 1, 4 * 29 - 1), _keys(2, 9), BG)))
    return out


def _cropped_cases():
    """Source 32x32 whose largest value sits where the crop removes it: cell 31 starts at output 126, cell 30 at 122, so
    121 drops both, 125 drops cell 31, 123 keeps only the first row / column of cell 30 (the one the peak is a corner of)."""
    out = []
    for y, x in ((31, 31), (31, 5), (5, 31)):
        for size in ((121, 121), (125, 128), (128, 125), (123, 123)):
            rw = _floor(2, 32, 32, seed=31 * y + x)
            rw[0, 0, 10, 12] = F32(0.4)                   # an interior bump: the maximum of a crop that loses the peak entirely
            rw[1, 0, y, x] = F32(1.0)
            out.append(("cropped_at_%d_%d_to_%dx%d" % (y, x, size[0], size[1]), (rw, size, _keys(2, 3), BG)))
    return out


def _plateau_cases():
    out = []
    flat = np.full((2, 1, 8, 8), 0.7, F32)
    out.append(("plateau_constant", (flat, (30, 31), _keys(2, 1), BG)))
    out.append(("plateau_constant_bg_ties", (flat, (32, 32), _keys(2, 1), 1.0)))      # background == 1.0 == every score
    out.append(("plateau_constant_inexact", (np.full((3, 1, 7, 5), 0.1, F32) * F32(3), (27, 19), _keys(3, 2), BG)))
    two = _floor(3, 9, 11, seed=41)
    two[1, 0, 2, 3] = two[2, 0, 6, 8] = F32(0.9)                                     # equal peaks, different channels
    out.append(("plateau_two_equal_peaks", (two, (36, 44), _keys(3, 4), BG)))
    twin = _floor(3, 9, 11, seed=42)
    twin[2, 0, 4, 4] = F32(0.8)
    twin[1] = twin[2]                                                                # channels 1 and 2 tie at every pixel
    out.append(("plateau_twin_channels", (twin, (35, 42), _keys(3, 5), 0.05)))
    return out


# hot-pixel positions (channel, y, x) of a 3 x 24 x 20 source: interior, last column, last row, the output rows and columns
# 64 +- 1 (a 256-thread boundary of the argmax pass at out_w = 80) and the first cell
HOT_SPOTS = ((0, 11, 9), (2, 15, 19), (1, 23, 7), (1, 16, 16), (2, 0, 0))


def _hot_cases():
    out = []
    for seed, pos in enumerate(HOT_SPOTS):
        rw, _ = hot_pixel(3, 24, 20, seed, pos)
        out.append(("hot_seed%d" % seed, (rw, (96, 80) if seed % 2 == 0 else (94, 77), _keys(3, seed), BG)))
    for seed in (5, 6):                                   # ... and wherever the seed itself puts it
        rw, _ = hot_pixel(4, 13, 17, seed)
        out.append(("hot_seed%d" % seed, (rw, (51, 66), _keys(4, seed), BG)))
    return out


def _magnitude_cases():
    out = []
    for tag, scale in (("1e-30", 1e-30), ("1e-38", 1e-38), ("1e+30", 1e+30)):
        for seed in (0, 1, 3):
            rw, _ = hot_pixel(3, 24, 20, seed, HOT_SPOTS[seed])
            out.append(("magnitude_%s_seed%d" % (tag, seed), ((rw * F32(scale)).astype(F32), (96, 80), _keys(3, seed), BG)))
    return out


def _sign_cases():
    rng = np.random.RandomState(77)
    neg = (-np.abs(rng.randn(3, 1, 10, 12)) - 0.1).astype(F32)
    mixed = rng.randn(3, 1, 10, 12).astype(F32)
    mixed[1, 0, 9, 11] = F32(4.5)
    return [("sign_all_negative", (neg, (40, 47), _keys(3, 6), BG)),
            ("sign_mixed", (mixed, (39, 48), _keys(3, 7), BG))]


def _zero_cases():
    return [("all_zero", (np.zeros((2, 1, 5, 6), F32), (20, 24), np.array([3, 7], np.int64), BG))]


ALIGN_WIDTHS = (1, 2, 3, 5, 6, 7, 375)


def align_cases():
    """out_w with a partial 4-pixel group; C and out_h odd so that C*oh*ow is odd wherever out_w is: the planes of rw_up
    and the rows of argmax / labels start at addresses that are not multiples of 16 (4 for the labels)."""
    out = []
    for n, ow in enumerate(ALIGN_WIDTHS):
        c, oh = 3, (5 if ow == 375 else 9)
        h, w = (oh + 3) // 4, (ow + 3) // 4 + (n % 2)
        rw = np.abs(np.random.RandomState(300 + ow).randn(c, 1, h, w)).astype(F32)
        out.append(("align_w%d" % ow, (rw, (oh, ow), _keys(c, ow), 0.5)))
    return out


def label_cases():
    return (_corner_cases() + _cropped_cases() + _plateau_cases() + _hot_cases() + _magnitude_cases() + _sign_cases() +
            _zero_cases() + align_cases())


def _peaked(rng, c, h, w):
    """A noise floor with one small blob of its own position (edges included) and scale."""
    rw = (np.abs(rng.randn(c, 1, h, w)) * 0.02).astype(F32)
    ch, y, x = int(rng.randint(c)), int(rng.randint(h)), int(rng.randint(w))
    scale = F32(10.0 ** rng.uniform(-2, 2))
    rw *= scale
    rw[ch, 0, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = scale * F32(0.5)
    rw[ch, 0, y, x] = scale
    if c > 1:                                             # a second class that wins a region of its own
        rw[(ch + 1) % c, 0, :h // 3, :w // 2] = scale * F32(0.4)
    return rw


def production_batch(n=256, seed=2024):
    """A batch of the production shape: ragged sources 24x20 .. 40x36, 1 .. 7 channels (mostly five or more, so that
    c*h*w > 4096 = the 16 workgroups x 256 threads an image gets in the maximum passes), a crop of 0 .. 7 per side."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        c = int(rng.choice([1, 2, 3, 4, 5, 6, 7], p=[.05, .05, .05, .1, .25, .25, .25]))
        h, w = int(rng.randint(24, 41)), int(rng.randint(20, 37))
        size = (4 * h - int(rng.randint(8)), 4 * w - int(rng.randint(8)))
        out.append((_peaked(rng, c, h, w), size, _keys(c, i), BG))
    assert sum(r.size > 4096 for r, _, _, _ in out) > n // 2
    return out


def tiny_batch(n=4097, seed=7):
    """n images of 2 x 8 x 8: more images than the maximum passes have workgroups to share out (one each)."""
    rng = np.random.RandomState(seed)
    rws = np.abs(rng.randn(n, 2, 1, 8, 8)).astype(F32)
    hot = rng.randint(0, 128, n)
    rws.reshape(n, 128)[np.arange(n), hot] *= F32(20)
    sizes = [(32 - int(a), 32 - int(b)) for a, b in rng.randint(0, 4, (n, 2))]
    keys = np.array([4, 11], np.int64)
    return rws, sizes, keys


BIG_SRC, BIG_OUT = (260, 132), (1040, 528)               # 549 120 pixels > 4 x 256 x 512: the argmax pass strides


def big_case(out_w=528):
    """One image whose argmax pass takes a second iteration (output rows >= 993 at out_w = 528); the global maximum and a
    region of another label lie in those rows only."""
    h, w = BIG_SRC
    rw = _floor(3, h, w, seed=5)
    rw[0, 0, 10:30, 15:60] = F32(0.45)                     # first iteration: class 0
    rw[2, 0, 250:259, 20:40] = F32(0.6)                    # second iteration only: class 2
    rw[1, 0, 255, 70] = F32(1.0)                           # ... and the global maximum
    return rw, (BIG_OUT[0], out_w), np.array([1, 8, 15], np.int64), BG


def mixed_batch():
    """The big image, a 1x1 source and a cropped-peak image: the launch sizes come from different images."""
    cropped = dict(label_cases())["cropped_at_31_31_to_123x123"]
    one = (np.full((2, 1, 1, 1), 0.3, F32) * np.array([1, 2], F32).reshape(2, 1, 1, 1), (3, 2), _keys(2, 8), BG)
    return [big_case(), one, cropped]


# ---------------------------------------------------------------------------------------------------------------------
# CAM merge
# ---------------------------------------------------------------------------------------------------------------------

def _label(n_cls, present):
    lab = np.zeros(n_cls, F32)
    lab[list(present)] = 1
    return lab


def merge_cases():
    """[(name, (outputs [n_classes, hs, ws] per scale, size (H, W), label multi-hot))] for irn_cam_merge."""
    out = []
    rng = np.random.RandomState(11)
    n_cls = 20

    def srcs(shapes):
        return [rng.randn(n_cls, hs, ws).astype(F32) for hs, ws in shapes]

    for H in (1, 3, 4, 5, 16, 17):
        for W in (1, 3, 4, 5, 16, 17):
            if (H + W) % 2 and H != 1 and W != 1:        # a third of the grid is plenty; keep every H = 1 and W = 1
                continue
            out.append(("size_%dx%d" % (H, W), (srcs([(2, 3), (1, 1), (5, 4)]), (H, W), _label(n_cls, (2, 9, 19)))))
    out.append(("eight_scales", (srcs([(1 + s, 9 - s) for s in range(8)]), (21, 30), _label(n_cls, (0, 7)))))
    out.append(("src_1x1", (srcs([(1, 1)]), (9, 7), _label(n_cls, (4,)))))
    out.append(("src_1xN", (srcs([(1, 6), (1, 1), (7, 1)]), (13, 33), _label(n_cls, (4, 5)))))
    out.append(("class_0_only", (srcs([(4, 5), (3, 3)]), (18, 15), _label(n_cls, (0,)))))
    out.append(("class_19_only", (srcs([(4, 5), (3, 3)]), (18, 15), _label(n_cls, (19,)))))
    s = srcs([(4, 5), (6, 7)])
    for o in s:
        o[3] = 0                                          # 0 / 1e-5
        o[6] = -np.abs(o[6]) - F32(0.5)                   # all negative: (negative max) + 1e-5
    out.append(("zero_and_negative_channels", (s, (19, 22), _label(n_cls, (3, 6, 12)))))
    # H, W = 17, 18 are interpolated at 32 x 32 and cropped: a channel whose only large values sit in the last source
    # column / row has its maximum where the crop removes it
    s = [np.full((n_cls, 8, 8), 0.1, F32) + rng.rand(n_cls, 8, 8).astype(F32) * F32(0.01) for _ in range(2)]
    for o in s:
        o[5, :, 7] = 3.0
        o[8, 7, :] = 2.0
    out.append(("max_in_cropped_margin", (s, (17, 18), _label(n_cls, (5, 8, 10)))))
    return out
