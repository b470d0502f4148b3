"""The boundary kernels of irn_amd/csrc/eval.hip (irn_label_band, irn_label_boundary_counts, irn_mask_boundary_overlap)
bit for bit against the plain-loop restatement tests/_boundary_ref.py.  The kernels' tile is 32 rows x 64 columns, so 33x70
and 130x67 cross tile edges in both directions."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _boundary_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 32, 64
LABELS = [0, 3, 20, 254, 255]


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(_dev())          # a copy: the cached cases are read-only


def _blobs(h, w, labels, seed, cell=5):
    rng = np.random.RandomState(seed)
    low = rng.choice(np.asarray(labels, np.uint8), ((h - 1) // cell + 1, (w - 1) // cell + 1))
    return np.ascontiguousarray(np.repeat(np.repeat(low, cell, axis=0), cell, axis=1)[:h, :w])


def _band(L, d):
    from irn_amd import ops
    out = ops.label_band(_t(L), d)
    assert out.dtype == torch.uint8 and tuple(out.shape) == L.shape
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _blob_case(h, w):
    """One blob map per size and its restated bands, computed once for every test that needs them."""
    L = _blobs(h, w, LABELS, h * 1000 + w, cell=7)
    L[:, w // 3:w // 3 + 2] = 254                        # 254 and 255 side by side
    L[:, w // 3 + 2:w // 3 + 4] = 255
    L.setflags(write=False)
    return L, {d: B.band(L, d) for d in (1, 3, 12, 64)}


# ---------------------------------------------------------------------------------------------------------------------
# label_band
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,d", [(1, 1, 1), (1, 37, 1), (37, 1, 1), (5, 7, 1), (5, 7, 2), (5, 7, 8)])
def test_band_small_shapes(h, w, d):
    L = _blobs(h, w, [0, 3, 255], h * 100 + w + d, cell=2)
    got = _band(L, d)
    assert np.array_equal(got, B.band(L, d))
    if (h, w, d) == (5, 7, 8) or min(h, w) == 1:
        assert got.all()                                  # the window leaves the image at every pixel


@pytest.mark.parametrize("h,w", [(33, 70), (130, 67)])
@pytest.mark.parametrize("d", [1, 3, 12, 64])
def test_band_random_blobs_across_tiles(h, w, d):
    L, want = _blob_case(h, w)
    assert np.array_equal(_band(L, d), want[d])


@pytest.mark.parametrize("d", [1, 3, 12])
def test_band_constant_map_is_the_frame(d):
    h, w = 70, 130
    for value in (0, 255):
        want = np.ones((h, w), np.uint8)
        want[d:h - d, d:w - d] = 0
        assert np.array_equal(_band(np.full((h, w), value, np.uint8), d), want)


def test_band_checkerboard_and_line():
    h, w = 33, 70
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 254).astype(np.uint8)
    for d in (1, 3):
        assert _band(board, d).all()
    line = np.zeros((h, w), np.uint8)
    line[:, 40] = 7                                       # one pixel wide, through two tiles
    line[20, :] = 9
    for d in (1, 3, 12):
        assert np.array_equal(_band(line, d), B.band(line, d))


@pytest.mark.parametrize("d", [1, 3, 12])
def test_band_rectangle_edges_at_d_and_d_plus_1_from_a_tile_boundary(d):
    h, w = 2 * TILE_H + 6, 2 * TILE_W + 2                 # 70 x 130: the tile boundaries are y = 32 and x = 64
    for off in (d, d + 1):
        for side in ("left", "right", "top", "bottom"):
            L = np.zeros((h, w), np.uint8)
            if side == "left":                            # the rectangle begins `off` cells right of the boundary
                L[5:60, TILE_W + off:w - 1] = 3
            elif side == "right":                         # and ends `off` cells left of it
                L[5:60, 2:TILE_W - off] = 3
            elif side == "top":
                L[TILE_H + off:h - 1, 4:120] = 3
            else:
                L[1:TILE_H - off, 4:120] = 3
            assert np.array_equal(_band(L, d), B.band(L, d)), (off, side)


# ---------------------------------------------------------------------------------------------------------------------
# label_boundary_counts
# ---------------------------------------------------------------------------------------------------------------------
def _sem_case(nc, h=70, w=130, seed=0):
    """pred / GT blob maps over 0..nc-1: a void ring around every GT blob, 255 pixels in pred, one class only in pred, one
    only in the GT (nc > 2), and one GT byte out of range."""
    rng = np.random.RandomState(seed + nc)
    base = _blobs(h, w, np.arange(min(nc, 6)), seed + nc, cell=11)
    gt = base.copy()
    gt[B.band(base, 1).astype(bool)] = 255                # the ring VOC draws around every object
    pred = np.roll(base, (2, 3), axis=(0, 1))
    pred[rng.rand(h, w) < 0.02] = 255
    if nc > 2:
        pred[pred == 1] = nc - 1                          # classes nc-1 (pred only) and 1 (GT only)
    gt[3, 5] = nc if nc < 200 else 0                      # out of range
    return pred, gt


@functools.lru_cache(maxsize=None)
def _sem_want(nc, d, pred_255_as):
    pred, gt = _sem_case(nc)
    return B.semantic_counts(pred, gt, d, nc, pred_255_as)


@pytest.mark.parametrize("nc", [2, 21, 81])
@pytest.mark.parametrize("pred_255_as", [0, None])
def test_boundary_counts_exact(nc, pred_255_as):
    from irn_amd import ops
    pred, gt = _sem_case(nc)
    d = 3
    want, want_bad = _sem_want(nc, d, pred_255_as)
    counts, bad = ops.label_boundary_counts(_t(pred), _t(gt), d, pred_255_as=pred_255_as, n_classes=nc)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (nc, 3)
    assert np.array_equal(counts.cpu().numpy(), want)
    assert int(bad.item()) == want_bad
    n255 = int((pred == 255).sum()) - int(pred[3, 5] == 255)              # (3, 5) holds the out-of-range GT byte: bad once
    assert n255 > 0 and want_bad == 1 + (0 if pred_255_as == 0 else n255)
    if nc > 2:
        assert want[nc - 1, 2] == 0 and want[nc - 1, 1] > 0 and want[1, 1] == 0 and want[1, 2] > 0
    assert want[:, 0].sum() > 0


def test_boundary_counts_accumulate_and_repeat_bit_for_bit():
    from irn_amd import ops
    nc, d = 21, 3
    pred, gt = _sem_case(nc)
    p2, g2 = np.ascontiguousarray(pred[:33, :70]), np.ascontiguousarray(gt[:33, :70])
    w1, b1 = _sem_want(nc, d, 0)
    w2, b2 = B.semantic_counts(p2, g2, 12, nc, 0)
    counts, bad = ops.label_boundary_counts(_t(pred), _t(gt), d, n_classes=nc)
    c_again, b_again = ops.label_boundary_counts(_t(p2), _t(g2), 12, counts, bad, n_classes=nc)
    assert c_again is counts and b_again is bad
    assert np.array_equal(counts.cpu().numpy(), w1 + w2) and int(bad.item()) == b1 + b2
    runs = [ops.label_boundary_counts(_t(pred), _t(gt), d, n_classes=nc)[0] for _ in range(5)]
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    bands = [ops.label_band(_t(gt), 12) for _ in range(5)]
    assert all(torch.equal(bands[0], b) for b in bands[1:])


# ---------------------------------------------------------------------------------------------------------------------
# mask_boundary_overlap
# ---------------------------------------------------------------------------------------------------------------------
def _ins_case():
    h, w = 70, 130
    inst = np.zeros((h, w), np.uint8)
    inst[0:30, 0:40] = 1                                  # touches the top and left edges
    inst[40:70, 90:130] = 2                               # bottom and right
    inst[10:50, 50:80] = 3
    masks = np.zeros((5, h, w), bool)
    masks[0, 0:28, 0:44] = True
    masks[1, 5:45, 45:85] = True                          # overlaps masks 0 (no) and 2
    masks[2, 20:60, 60:100] = True
    masks[3] = True                                       # all ones: its band is the image frame
    masks[4, 42:70, 88:130] = True
    return masks, inst


def _check_ins(masks, inst, g, d, inst_band=None):
    from irn_amd import ops
    bad = torch.zeros(1, dtype=torch.int64, device=_dev())
    got = ops.mask_boundary_overlap(_t(masks), _t(inst), g, d, bad, inst_band)
    want = B.instance_counts(masks, inst, g, d)
    for a, b in zip(got, want[:3]):
        assert a.dtype == torch.int64 and np.array_equal(a.cpu().numpy(), b)
    assert int(bad.item()) == want[3]
    return got, want


@pytest.mark.parametrize("d", [1, 3, 12])
def test_mask_boundary_overlap_exact(d):
    masks, inst = _ins_case()
    got, want = _check_ins(masks, inst, 3, d)
    assert tuple(got[0].shape) == (5, 3) and want[0].sum() > 0
    frame = 70 * 130 - (70 - 2 * d) * (130 - 2 * d)
    assert want[1][3] == frame


def test_mask_boundary_overlap_empty_sides_and_bad_ids():
    masks, inst = _ins_case()
    got, _ = _check_ins(masks[:0], inst, 3, 3)            # N = 0
    assert tuple(got[0].shape) == (0, 3) and tuple(got[1].shape) == (0,) and int(got[2].sum()) > 0
    got, _ = _check_ins(masks, np.zeros_like(inst), 0, 3)  # G = 0
    assert tuple(got[0].shape) == (5, 0) and tuple(got[2].shape) == (0,) and int(got[1].sum()) > 0
    _check_ins(masks[:0], np.zeros_like(inst), 0, 3)
    got, want = _check_ins(masks, inst, 2, 3)             # id 3 is above G = 2: every pixel of it is bad, none is counted
    assert want[3] == int((inst == 3).sum()) > 0
    empty = np.zeros((1, 70, 130), bool)
    got, _ = _check_ins(empty, inst, 3, 3)
    assert int(got[1][0]) == 0


def test_mask_boundary_overlap_200_instances():
    h = w = 64
    yy, xx = np.mgrid[0:h, 0:w]
    cell = (yy // 2) * (w // 2) + xx // 2                 # 1024 cells of 2x2
    inst = np.where(cell < 200, cell + 1, 0).astype(np.uint8)
    masks = np.zeros((3, h, w), bool)
    masks[0, :9, :] = True
    masks[1, 3:20, 10:50] = True
    masks[2, 11:13, :] = True
    _check_ins(masks, inst, 200, 1)
    _check_ins(masks, inst, 200, 2)


def test_mask_boundary_overlap_reuses_the_scratch_across_sizes():
    from irn_amd import ops
    masks, inst = _ins_case()
    scratch = torch.full((70 * 130 + 11,), 9, dtype=torch.uint8, device=_dev())
    _check_ins(masks, inst, 3, 3, scratch)
    assert np.array_equal(scratch[:70 * 130].cpu().numpy().reshape(70, 130), B.band(inst, 3))
    assert bool((scratch[70 * 130:] == 9).all())
    m2, i2 = np.ascontiguousarray(masks[:, :33, :70]), np.ascontiguousarray(inst[:33, :70])
    _check_ins(m2, i2, 3, 12, scratch)
    assert np.array_equal(scratch[:33 * 70].cpu().numpy().reshape(33, 70), B.band(i2, 12))
    _check_ins(masks, inst, 3, 1, scratch)
    runs = [ops.mask_boundary_overlap(_t(masks), _t(inst), 3, 3) for _ in range(5)]
    assert all(torch.equal(a, b) for r in runs[1:] for a, b in zip(runs[0], r))


# ---------------------------------------------------------------------------------------------------------------------
# refusals: nothing is written
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    from irn_amd import ops
    from irn_amd._lib import IrnHipError
    dev = _dev()
    m = torch.zeros(8, 9, dtype=torch.uint8, device=dev)
    counts = torch.full((21, 3), 7, dtype=torch.int64, device=dev)
    bad = torch.full((1,), 7, dtype=torch.int64, device=dev)
    scratch = torch.full((100,), 9, dtype=torch.uint8, device=dev)
    masks = torch.zeros(2, 8, 9, dtype=torch.uint8, device=dev)
    errors = (ValueError, IrnHipError)
    with pytest.raises(errors):                                           # shapes
        ops.label_boundary_counts(m, m[:, :8], 1, counts, bad)
    with pytest.raises(errors):
        ops.mask_boundary_overlap(masks[:, :7], m, 1, 1, bad, scratch)
    with pytest.raises(errors):                                           # dtypes
        ops.label_band(m.to(torch.int32), 1)
    with pytest.raises(errors):
        ops.label_boundary_counts(m.to(torch.int64), m, 1, counts, bad)
    with pytest.raises(errors):
        ops.mask_boundary_overlap(masks.to(torch.float32), m, 1, 1, bad, scratch)
    with pytest.raises(errors):
        ops.mask_boundary_overlap(masks, m, 1, 1, bad, scratch.to(torch.int32))
    with pytest.raises(errors):
        ops.mask_boundary_overlap(masks, m, 1, 1, bad, scratch[:50])      # scratch too small for 8 x 9
    for d in (0, 65, -3, 1.5):                                            # d
        with pytest.raises(errors):
            ops.label_band(m, d)
        with pytest.raises(errors):
            ops.label_boundary_counts(m, m, d, counts, bad)
        with pytest.raises(errors):
            ops.mask_boundary_overlap(masks, m, 1, d, bad, scratch)
    with pytest.raises(errors):                                           # accumulators of another shape or type
        ops.label_boundary_counts(m, m, 1, torch.zeros(3, 21, dtype=torch.int64, device=dev), bad)
    with pytest.raises(errors):
        ops.label_boundary_counts(m, m, 1, counts, torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(errors):
        ops.label_boundary_counts(m, m, 1, counts.to(torch.int32), bad)
    with pytest.raises(errors):
        ops.label_boundary_counts(m, m, 1, counts, bad, n_classes=82)
    with pytest.raises(errors):
        ops.label_boundary_counts(m, m, 1, counts, bad, pred_255_as=21)
    torch.cuda.synchronize()
    assert bool((counts == 7).all()) and int(bad.item()) == 7 and bool((scratch == 9).all())
