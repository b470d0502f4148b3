"""The counting kernels at a run-time class count (eval.hip, label.hip, thres_hist.hpp; `n_classes` of ops.cam_confusion,
cam_confusion_matrices, label_confusion, ir_label_confusion, label_sweep_confusion): nc = 2, 21 and 81 classes including
the background.  Every count is an integer and must equal the numpy restatement in this file exactly, the `bad` count
included.  The images are 61 x 67 (4 087 pixels: one partial block of 4 096) and 97 x 131 (12 707 pixels: four blocks, the
last one partial, a length that is no multiple of 4); one accumulator takes both.  GT holds 0, nc-1, 255 and the bad values
nc and 254; predictions hold nc-1 and nc; keys hold nc-2 (valid) and nc-1 (bad).  At nc = 21 the entry points without a
class count must give the same tensors as the new ones."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _label_sweep_ref as S  # noqa: E402  (pixel_pairs and thresholds carry no class count)

pytestmark = pytest.mark.gpu

NCS = (2, 21, 81)
SIZES = ((61, 67), (97, 131))


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _gt(size, nc, seed):
    """uint8 [h,w]: blocks of 0..nc-1 and 255, with 0, nc-1, 255 and the bad values nc and 254 planted."""
    rng = np.random.RandomState(seed)
    h, w = size
    vals = np.concatenate([np.arange(nc), [255]]).astype(np.uint8)
    coarse = vals[rng.randint(0, vals.size, ((h + 4) // 5, (w + 6) // 7))]
    gt = np.repeat(np.repeat(coarse, 5, axis=0), 7, axis=1)[:h, :w].copy()
    flat = gt.reshape(-1)
    pos = rng.permutation(flat.size)[:25]
    flat[pos] = np.resize(np.uint8([0, nc - 1, 255, nc, 254]), 25)
    flat[-1] = nc                                  # a bad value in the last, partial group of four
    return gt


def _row(gt, nc):
    """GT -> histogram row: g <= nc-1 -> g, 255 -> nc, anything else -1 (bad)."""
    g = gt.astype(np.int64)
    return np.where(g <= nc - 1, g, np.where(g == 255, nc, -1))


def _confusion(row, pred, nc):
    """(conf [nc,nc], void [nc]) of the pixels given (rows 0..nc, predictions 0..nc-1)."""
    full = np.bincount(row * nc + pred, minlength=(nc + 1) * nc).reshape(nc + 1, nc)
    return full[:nc], full[nc]


# ------------------------------------------------------------------------------------------------
# cam_confusion + cam_confusion_matrices
# ------------------------------------------------------------------------------------------------
def _cam(size, k, seed):
    """fp32 [k,h,w] in eighths (ties between planes and maxima equal to a threshold are common), one planted tie at the
    maximum between planes 0 and 1 and a NaN in the last plane."""
    rng = np.random.RandomState(seed)
    h, w = size
    cam = (rng.randint(0, 9, (k, h, w)) / 8.0).astype(np.float32)
    if k >= 2:
        cam[:, 3, 5] = 0.25
        cam[0, 3, 5] = cam[1, 3, 5] = 2.0          # planes 0 and 1 tie: plane 0 keeps the pixel
    if k >= 1:
        cam[k - 1, 7, 11] = np.nan
        cam[0, h - 1, w - 2] = np.nan
    return cam


def _cam_pixels(cam, keys, gt, nc):
    """-> (row, col, m) of the pixels that count, and the number that do not."""
    row = _row(gt, nc).reshape(-1)
    k = cam.shape[0]
    if k == 0:
        ok = row >= 0
        return row[ok], np.zeros(ok.sum(), np.int64), np.full(ok.sum(), -np.inf, np.float32), int((~ok).sum())
    flat = cam.reshape(k, -1)
    nan = np.isnan(flat).any(axis=0)
    c = np.argmax(np.where(np.isnan(flat), -np.inf, flat), axis=0)             # the first plane at the maximum
    m = flat[c, np.arange(flat.shape[1])]
    key = np.asarray(keys, np.int64)[c]
    ok = (row >= 0) & ~nan & (key >= 0) & (key <= nc - 2)
    return row[ok], key[ok] + 1, m[ok], int((~ok).sum())


def _cam_expected(images, nc, th):
    t = th.size
    hist = np.zeros((nc + 1, nc, t + 1), np.int64)
    conf = np.zeros((t, nc, nc), np.int64)
    void = np.zeros((t, nc), np.int64)
    bad = 0
    for cam, keys, gt in images:
        row, col, m, b = _cam_pixels(cam, keys, gt, nc)
        bad += b
        j = np.searchsorted(th, m, side="left")                                # thresholds < m
        np.add.at(hist, (row, col, j), 1)
        for i in range(t):                                                     # straight from the pixels, not from hist
            cf, vd = _confusion(row, np.where(m > th[i], col, 0), nc)
            conf[i] += cf
            void[i] += vd
    return hist, conf, void, bad


def _cam_images(nc, k):
    keys_a = nc - 2 - np.arange(k, dtype=np.int64)                             # holds nc-2, all valid
    keys_b = keys_a.copy()
    if k:
        keys_b[-1] = nc - 1                                                    # one bad key
    return [(_cam(SIZES[0], k, 10 * nc + k), keys_a, _gt(SIZES[0], nc, nc)),
            (_cam(SIZES[1], k, 10 * nc + k + 1), keys_b, _gt(SIZES[1], nc, nc + 1))]


def _thres(t):
    return np.float32([0.5]) if t == 1 else (np.arange(t, dtype=np.float32) / np.float32(200.0))


@pytest.mark.parametrize("t", [1, 256])
@pytest.mark.parametrize("nc", NCS)
def test_cam_confusion_and_reduce(nc, t):
    from irn_amd import ops
    th = _thres(t)
    for k in sorted({0, 1, nc - 1}):
        images = _cam_images(nc, k)
        hist = bad = None
        for cam, keys, gt in images:
            hist, bad = ops.cam_confusion(_t(cam), keys, _t(gt), th, hist, bad, n_classes=nc)
        conf, void = ops.cam_confusion_matrices(hist, n_classes=nc)
        w_hist, w_conf, w_void, w_bad = _cam_expected(images, nc, th)
        assert w_bad > 0 and w_hist.sum() > 0
        assert int(bad.item()) == w_bad, (k, int(bad.item()), w_bad)
        assert tuple(hist.shape) == (nc + 1, nc, t + 1) and tuple(conf.shape) == (t, nc, nc) and tuple(void.shape) == (t, nc)
        assert np.array_equal(hist.cpu().numpy(), w_hist), k
        assert np.array_equal(conf.cpu().numpy(), w_conf), k
        assert np.array_equal(void.cpu().numpy(), w_void), k
        if k == nc - 1 and nc > 2:
            assert w_conf[:, :, nc - 1].sum() > 0, "the last class must be predicted somewhere"


def test_cam_confusion_refuses_what_does_not_fit():
    from irn_amd import ops
    gt = _t(_gt(SIZES[0], 2, 0))
    with pytest.raises(ValueError, match="n_classes"):
        ops.cam_confusion(torch.zeros((0,) + SIZES[0], device=_dev()), [], gt, [0.5], n_classes=82)
    with pytest.raises(ValueError, match="n_classes"):
        ops.label_confusion(gt, gt, n_classes=1)
    with pytest.raises(ValueError, match="planes"):
        ops.cam_confusion(torch.zeros((2,) + SIZES[0], device=_dev()), [0, 1], gt, [0.5], n_classes=2)
    hist, _ = ops.cam_confusion(torch.zeros((1,) + SIZES[0], device=_dev()), [0], gt, [0.5], n_classes=2)
    with pytest.raises(ValueError):
        ops.cam_confusion_matrices(hist)                                       # a [3,2,2] histogram is not a 21-class one


# ------------------------------------------------------------------------------------------------
# label_confusion
# ------------------------------------------------------------------------------------------------
def _pred(size, nc, seed):
    rng = np.random.RandomState(seed)
    h, w = size
    pred = rng.randint(0, nc, (h, w)).astype(np.uint8)
    flat = pred.reshape(-1)
    pos = rng.permutation(flat.size)[:40]
    flat[pos] = np.resize(np.uint8([nc - 1, nc, 255, 0]), 40)
    return pred


@pytest.mark.parametrize("pred_255_as", [-1, 0])
@pytest.mark.parametrize("nc", NCS)
def test_label_confusion(nc, pred_255_as):
    from irn_amd import ops
    conf = void = bad = None
    w_conf, w_void, w_bad = np.zeros((nc, nc), np.int64), np.zeros(nc, np.int64), 0
    for n, size in enumerate(SIZES):
        gt, pred = _gt(size, nc, 50 + n), _pred(size, nc, 60 + n)
        conf, void, bad = ops.label_confusion(_t(pred), _t(gt), conf, bad, pred_255_as=None if pred_255_as < 0 else pred_255_as,
                                              void=void, n_classes=nc)
        row = _row(gt, nc).reshape(-1)
        q = pred.reshape(-1).astype(np.int64)
        if pred_255_as >= 0:
            q = np.where(q == 255, pred_255_as, q)
        ok = (row >= 0) & (q < nc)
        cf, vd = _confusion(row[ok], q[ok], nc)
        w_conf += cf
        w_void += vd
        w_bad += int((~ok).sum())
    assert w_bad > 0 and w_conf[nc - 1, nc - 1] + w_conf[:, nc - 1].sum() > 0
    assert int(bad.item()) == w_bad
    assert np.array_equal(conf.cpu().numpy(), w_conf) and np.array_equal(void.cpu().numpy(), w_void)


# ------------------------------------------------------------------------------------------------
# ir_label_confusion
# ------------------------------------------------------------------------------------------------
def _planes(size, nc, seed):
    """uint8 [16,h,w]: half of every plane 0, the rest 0..nc-1; plane 5 holds the bad value nc at a few pixels."""
    rng = np.random.RandomState(seed)
    h, w = size
    pl = np.where(rng.rand(16, h, w) < 0.5, 0, rng.randint(0, nc, (16, h, w))).astype(np.uint8)
    pl[:, 2, 3] = nc - 1
    pl[5].reshape(-1)[rng.permutation(h * w)[:9]] = nc
    return pl


def _ir_expected(planes, fg_idx, bg_idx, gt, nc):
    row = _row(gt, nc).reshape(-1)
    flat = planes.reshape(planes.shape[0], -1).astype(np.int64)
    ok = (row >= 0) & (flat <= nc - 1).all(axis=0)
    hist = np.zeros((len(fg_idx), len(bg_idx), nc + 1, nc + 1), np.int64)
    for i, fi in enumerate(fg_idx):
        for j, bj in enumerate(bg_idx):
            fgv, bgv = flat[fi][ok], flat[bj][ok]
            col = np.where(fgv != 0, fgv, np.where(bgv == 0, 0, nc))           # column nc = label 255
            hist[i, j] = np.bincount(row[ok] * (nc + 1) + col, minlength=(nc + 1) ** 2).reshape(nc + 1, nc + 1)
    return hist, int((~ok).sum())


@pytest.mark.parametrize("grid", ["1x1", "16x16"])
@pytest.mark.parametrize("nc", NCS)
def test_ir_label_confusion(nc, grid):
    """16 x 16 at 81 classes needs ten times the LDS of a workgroup: the fg axis runs in groups, and neither the histogram
    nor the bad count may show it."""
    from irn_amd import ops
    fg_idx, bg_idx = ([3], [7]) if grid == "1x1" else (list(range(16)), list(range(15, -1, -1)))
    hist = bad = None
    w_hist, w_bad = 0, 0
    for n, size in enumerate(SIZES):
        gt, planes = _gt(size, nc, 70 + n), _planes(size, nc, 80 + n)
        hist, bad = ops.ir_label_confusion(_t(planes), fg_idx, bg_idx, _t(gt), hist, bad, n_classes=nc)
        h, b = _ir_expected(planes, fg_idx, bg_idx, gt, nc)
        w_hist, w_bad = w_hist + h, w_bad + b
    assert w_bad >= 9 and w_hist[..., nc].sum() > 0 and w_hist[..., nc - 1].sum() > 0
    assert int(bad.item()) == w_bad
    assert np.array_equal(hist.cpu().numpy(), w_hist)


# ------------------------------------------------------------------------------------------------
# label_sweep_confusion
# ------------------------------------------------------------------------------------------------
def _scores(c, h, w, seed):
    rng = np.random.RandomState(seed)
    rw = np.abs(rng.randn(c, 1, h, w)).astype(np.float32) * 0.05
    for ch in range(c):                            # every channel wins a patch of its own
        y, x = (3 * ch) % (h - 2), (5 * ch) % (w - 3)
        rw[ch, 0, y:y + 2, x:x + 3] = 0.3 + 0.005 * ch
    return rw


def _sweep_expected(items, nc, th):
    t = th.size
    hist = np.zeros((nc + 1, nc, t + 1), np.int64)
    bad = 0
    for rw, size, keys, gt in items:
        cstar, m, nan = (np.asarray(a).reshape(size) for a in S.pixel_pairs(rw, size))
        j = np.where(nan, t, np.searchsorted(th, m, side="left"))
        row = _row(gt, nc)
        key = np.asarray(keys, np.int64)[cstar]
        ok = (row >= 0) & (key >= 0) & (key <= nc - 2)
        bad += int((~ok).sum())
        np.add.at(hist, (row[ok], key[ok] + 1, j[ok]), 1)
    return hist, bad


def _sweep_items(nc):
    c = nc - 1
    a = (_scores(c, 24, 20, 90 + nc), (93, 77), np.arange(c, dtype=np.int64)[::-1].copy())
    b = (_scores(1, 20, 24, 91 + nc), (77, 93), np.int64([nc - 2]))
    b_bad = (b[0], b[1], np.int64([nc - 1]))
    return [it + (_gt(it[1], nc, 95 + n),) for n, it in enumerate((a, b, b_bad))]


@pytest.mark.parametrize("t", [1, 16])
@pytest.mark.parametrize("nc", NCS)
def test_label_sweep_confusion(nc, t):
    from irn_amd import ops
    items = _sweep_items(nc)
    th = S.thresholds(items[0][0], items[0][1], t, seed=nc)
    hist = bad = None
    for batch in (items[:2], items[2:]):           # a batch of two images, then the image whose key is out of range
        hist, bad = ops.label_sweep_confusion([_t(i[0]) for i in batch], [i[1] for i in batch], [_t(i[2]) for i in batch],
                                              [_t(i[3]) for i in batch], th, hist, bad, n_classes=nc)
    w_hist, w_bad = _sweep_expected(items, nc, th)
    assert w_bad > 77 * 93 // 2 and w_hist[:, nc - 1].sum() > 0
    assert int(bad.item()) == w_bad
    assert np.array_equal(hist.cpu().numpy(), w_hist)
    conf, void = ops.cam_confusion_matrices(hist, n_classes=nc)
    for i in range(t):
        above, below = w_hist[:, :, i + 1:].sum(axis=2), w_hist[:, :, :i + 1].sum(axis=2)
        full = above.copy()
        full[:, 0] = w_hist[:, 0].sum(axis=1) + below[:, 1:].sum(axis=1)
        assert np.array_equal(conf[i].cpu().numpy(), full[:nc]) and np.array_equal(void[i].cpu().numpy(), full[nc])


# ------------------------------------------------------------------------------------------------
# nc = 21: the C entries with 21 passed explicitly are the wrappers called without a class count
# ------------------------------------------------------------------------------------------------
def test_old_entries_equal_the_new_ones_at_21_classes():
    """The raw C entries, called through `lib` with n_classes = 21 written out, give the bits of the `ops` wrappers called
    without `n_classes`: pins the argument's position in `_lib._SIGS` and the wrappers' default."""
    from irn_amd import ops
    from irn_amd._lib import _stream, check, i32_array, lib, ptr_array
    nc, size = 21, SIZES[1]
    h, w = size
    dev = _dev()

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.int64, device=dev)

    gt = _t(_gt(size, nc, 1))
    th = _t(_thres(256))
    cam, keys_a, _ = _cam_images(nc, nc - 1)[1]
    cam_d, keys_d = _t(cam), _t(keys_a)
    hist, bad = zeros(nc + 1, nc, 257), zeros(1)
    check(lib.irn_cam_confusion(cam_d.data_ptr(), keys_d.data_ptr(), nc - 1, gt.data_ptr(), h, w, th.data_ptr(), 256,
                                21, hist.data_ptr(), bad.data_ptr(), _stream()))
    n_hist, n_bad = ops.cam_confusion(cam_d, keys_d, gt, th)
    assert torch.equal(hist, n_hist) and torch.equal(bad, n_bad) and int(hist.sum()) > 0

    conf, void = zeros(256, nc, nc), zeros(256, nc)
    check(lib.irn_cam_confusion_reduce(hist.data_ptr(), 256, 21, conf.data_ptr(), void.data_ptr(), _stream()))
    n_conf, n_void = ops.cam_confusion_matrices(hist)
    assert torch.equal(conf, n_conf) and torch.equal(void, n_void)

    pred = _t(_pred(size, nc, 2))
    conf, void, bad = zeros(nc, nc), zeros(nc), zeros(1)
    check(lib.irn_label_confusion(pred.data_ptr(), gt.data_ptr(), h, w, 0, 21, conf.data_ptr(), void.data_ptr(), bad.data_ptr(),
                                  _stream()))
    n_conf, n_void, n_bad = ops.label_confusion(pred, gt)
    assert torch.equal(conf, n_conf) and torch.equal(void, n_void) and torch.equal(bad, n_bad)

    planes = _t(_planes(size, nc, 3))
    idx = np.arange(16, dtype=np.int32)
    pi32 = C.POINTER(C.c_int32)
    hist, bad = zeros(16, 16, nc + 1, nc + 1), zeros(1)
    check(lib.irn_ir_label_confusion(planes.data_ptr(), 16, idx.ctypes.data_as(pi32), 16, idx.ctypes.data_as(pi32), 16,
                                     gt.data_ptr(), h, w, 21, hist.data_ptr(), bad.data_ptr(), _stream()))
    n_hist, n_bad = ops.ir_label_confusion(planes, idx, idx, gt)
    assert torch.equal(hist, n_hist) and torch.equal(bad, n_bad) and int(bad) > 0

    rw, out, keys, sgt = _sweep_items(nc)[0]
    rw_d, keys_d, sgt_d = _t(rw).reshape(nc - 1, 24, 20), _t(keys), _t(sgt)
    sth = _t(S.thresholds(rw, out, 16, seed=4))
    hist, bad = zeros(nc + 1, nc, 17), zeros(1)
    scratch = torch.empty(64, dtype=torch.int32, device=dev)
    check(lib.irn_label_sweep_confusion(1, ptr_array([rw_d.data_ptr()]), i32_array([nc - 1]), i32_array([24]), i32_array([20]),
                                        i32_array([out[0]]), i32_array([out[1]]), ptr_array([keys_d.data_ptr()]),
                                        ptr_array([sgt_d.data_ptr()]), sth.data_ptr(), 16, 21, hist.data_ptr(), bad.data_ptr(),
                                        scratch.data_ptr(), _stream()))
    n_hist, n_bad = ops.label_sweep_confusion([rw_d], [out], [keys_d], [sgt_d], sth)
    torch.cuda.synchronize()
    assert torch.equal(hist, n_hist) and torch.equal(bad, n_bad) and int(hist.sum()) > 0
