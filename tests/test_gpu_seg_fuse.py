"""`ops.seg_fuse` (irn_amd/csrc/seg_fuse.hip) against the numpy restatement tests/_seg_fuse_ref.py.

The bars are those of tests/_parity.py and tests/test_gpu_score_crf.py: the probabilities within 1e-4 max-abs of the float64
restatement, and a label may differ only where the restatement's two best probabilities are a < TIE_TOL tie (and then the GPU
picked an entry inside that band), with no allowance on the count.  A float32 CPU emulation of the kernel lies 3e-8 to 5e-7 from
the float64 form on these shapes and differs in no label (an expectation from the CPU, not a GPU measurement).  Everything else
— the label against the call's own probabilities, the three output modes, repeated calls, the clean pixels of a NaN run — is
bitwise."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _seg_fuse_ref as R  # noqa: E402
from _parity import TIE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

# (H, W, C, scales, stride): the smallest shapes at which each part can go wrong
SHAPES = [
    (37, 53, 21, (0.5, 0.75, 1, 1.25, 1.5), 16),     # the production scale list
    (130, 150, 21, (0.5, 1, 1.5), 16),               # several output tiles per axis: seams
    (9, 7, 2, (1, 2), 16),                           # maps of one or two cells, clamped on every side
    (64, 64, 81, (0.75, 1), 16),                     # the class cap
    (33, 47, 21, (1,), 16),                          # one map
    (40, 40, 5, (0.5, 1.5), 4),                      # ratio up to 0.375: wide rectangles
    (9, 9, 2, (1,) * 16, 16),                        # the map cap
    # ... and the two at which the 32 x 32 tile's rectangles exceed 64 KB of LDS, so that the host picks the smaller tiles
    (40, 40, 21, (1, 0.5), 1),                       # 16 x 16 tiles: 116 KB at 32, 33 KB at 16
    (20, 20, 81, (1,), 1),                           # 8 x 8 tiles: 94 KB at 16, 26 KB at 8
]
_IDS = ["%dx%dx%d_%dmaps_s%d" % (s[0], s[1], s[2], len(s[3]), s[4]) for s in SHAPES]
_CASES = {}


def _dev():
    return torch.device("cuda", 0)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _case(shape):
    """(maps, sizes, the restatement's P) of a shape, computed once and left unchanged."""
    if shape not in _CASES:
        maps, sizes = R.case_maps(shape)
        _CASES[shape] = (maps, sizes, R.fuse(maps, sizes, shape[4], shape[:2]))
    return _CASES[shape]


def _fuse(maps, sizes, shape, **kw):
    from irn_amd import ops
    return ops.seg_fuse([_gpu(m) for m in maps], sizes, shape[4], shape[:2], **kw)


def _first_max(p):
    """torch.argmax's rule on a [C,H,W] tensor, class by class as the kernel states it."""
    return torch.argmax(p, 0).to(torch.uint8)


@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_prob_and_label_vs_restatement(shape):
    maps, sizes, want = _case(shape)
    label, prob = _fuse(maps, sizes, shape, want_label=True, want_prob=True)
    assert label.dtype == torch.uint8 and tuple(label.shape) == shape[:2] and label.is_cuda
    assert prob.dtype == torch.float32 and tuple(prob.shape) == (shape[2],) + shape[:2]
    assert torch.equal(label, _first_max(prob)), "the label is not the first maximum of the call's own probabilities"
    got, lab = prob.cpu().numpy(), label.cpu().numpy()
    err = float(np.abs(got - want).max())
    ties = float((R.top2_gap(want) < TIE_TOL).mean())
    diff = lab != R.labels_of(want)
    print("\n%s: prob max-abs %.3g vs the float64 restatement; %d of %d labels differ (%.3f %% of the pixels are ties)"
          % (shape, err, int(diff.sum()), diff.size, 100 * ties))
    assert err <= 1e-4, (shape, err)
    if diff.any():
        gap = R.top2_gap(want)[diff]
        assert float(gap.max()) < TIE_TOL, "%s: %d pixels differ, one is not a tie (gap %.3g)" % (shape, int(diff.sum()), float(gap.max()))
        ys, xs = np.nonzero(diff)
        assert (want[lab[ys, xs], ys, xs] >= want[:, ys, xs].max(0) - TIE_TOL).all(), "a differing pixel chose an entry outside the tie band"
    assert len(np.unique(lab)) >= min(2, len(np.unique(R.labels_of(want))))     # not vacuous wherever the restatement is not


@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_output_modes_and_repeated_calls_give_the_same_bits(shape):
    maps, sizes, _ = _case(shape)
    dev_maps = [_gpu(m) for m in maps]
    from irn_amd import ops
    label, prob = ops.seg_fuse(dev_maps, sizes, shape[4], shape[:2], want_label=True, want_prob=True)
    only_label, none = ops.seg_fuse(dev_maps, sizes, shape[4], shape[:2])
    assert none is None and torch.equal(only_label, label)
    none, only_prob = ops.seg_fuse(dev_maps, sizes, shape[4], shape[:2], want_label=False, want_prob=True)
    assert none is None and torch.equal(only_prob.view(torch.int32), prob.view(torch.int32))
    for _ in range(5):
        again, p2 = ops.seg_fuse(dev_maps, sizes, shape[4], shape[:2], want_label=True, want_prob=True)
        assert torch.equal(again, label) and torch.equal(p2.view(torch.int32), prob.view(torch.int32))


def test_a_tie_goes_to_the_first_class():
    shape = (37, 53, 21, (0.5, 0.75, 1, 1.25, 1.5), 16)
    maps, sizes, _ = _case(shape)
    tied = [m.copy() for m in maps]
    for m in tied:
        m[3] = 40.0                                  # two classes with equal logits in every map, far above the others
        m[11] = 40.0
    label, prob = _fuse(tied, sizes, shape, want_label=True, want_prob=True)
    assert bool((label == 3).all())
    assert torch.equal(prob[3].view(torch.int32), prob[11].view(torch.int32)) and bool((prob[3] > 0.49).all())
    two = (9, 7, 2, (1, 2), 16)
    maps, sizes, _ = _case(two)
    label, prob = _fuse([np.zeros_like(m) for m in maps], sizes, two, want_label=True, want_prob=True)
    assert not label.any() and bool((prob == 0.5).all())


@pytest.mark.parametrize("shape,m,cell", [((37, 53, 21, (0.5, 0.75, 1, 1.25, 1.5), 16), 2, (5, 1, 2)),
                                          ((130, 150, 21, (0.5, 1, 1.5), 16), 0, (20, 4, 0)),
                                          ((40, 40, 5, (0.5, 1.5), 4), 1, (2, 7, 3))])
def test_a_nan_logit_reaches_exactly_the_pixels_whose_taps_read_it(shape, m, cell):
    maps, sizes, _ = _case(shape)
    clean_label, clean_prob = _fuse(maps, sizes, shape, want_label=True, want_prob=True)
    bad = [x.copy() for x in maps]
    c, y, x = cell
    bad[m][c, y, x] = np.nan
    label, prob = _fuse(bad, sizes, shape, want_label=True, want_prob=True)
    hh, ww, _, _, stride = shape
    hit = (R.touched(hh, maps[m].shape[1], R.ratio(sizes[m][0], stride, hh), y)[:, None]
           & R.touched(ww, maps[m].shape[2], R.ratio(sizes[m][1], stride, ww), x)[None, :])
    assert hit.any() and not hit.all()
    hit_t = torch.from_numpy(hit).to(_dev())
    assert torch.equal(torch.isnan(prob), hit_t[None].expand_as(prob)), "NaN probabilities elsewhere than under the NaN cell's taps"
    assert not label[hit_t].any(), "a pixel under the NaN is not labelled 0"
    assert torch.equal(label[~hit_t], clean_label[~hit_t])
    assert torch.equal(prob[:, ~hit_t].view(torch.int32), clean_prob[:, ~hit_t].view(torch.int32))
    assert np.array_equal(np.isnan(R.fuse(bad, sizes, stride, (hh, ww))), np.broadcast_to(hit, prob.shape))       # ... as the restatement has it


def test_huge_logits_give_finite_probabilities():
    shape = (33, 47, 21, (0.75, 1, 1.5), 16)
    maps, sizes = R.case_maps(shape, seed=3)
    rng = np.random.RandomState(4)
    big = [np.where(rng.rand(*m.shape) < 0.5, np.float32(1e4), np.float32(-1e4)) + m for m in maps]
    label, prob = _fuse(big, sizes, shape, want_label=True, want_prob=True)
    assert bool(torch.isfinite(prob).all()) and bool((prob >= 0).all())
    assert float((prob.sum(0) - 1).abs().max()) <= 1e-5
    want = R.fuse(big, sizes, 16, shape[:2])
    err = float(np.abs(prob.cpu().numpy() - want).max())
    print("\n+-1e4 logits: prob max-abs %.3g vs the float64 restatement" % err)
    # (no bar against the restatement here: the blend of 1e4-sized logits rounds at 1e-3, which the softmax turns into a
    # relative error of the same size; the definition asks for finite values, and the sum above pins the normalisation)
    assert torch.equal(label, _first_max(prob))


@pytest.mark.parametrize("hw,c,stride", [((33, 47), 21, 16), ((64, 50), 5, 8), ((9, 7), 2, 4)])
def test_one_map_at_full_size_is_the_softmax_of_upsample_bilinear(hw, c, stride):
    from irn_amd import ops
    hh, ww = hw
    rng = np.random.RandomState(7)
    logits = _gpu((3 * rng.standard_normal((c, -(-hh // stride), -(-ww // stride)))).astype(np.float32))
    label, prob = ops.seg_fuse([logits], [hw], stride, hw, want_label=True, want_prob=True)
    up = ops.upsample_bilinear(logits, stride)[:, :hh, :ww]
    want = torch.softmax(up.contiguous(), 0)
    err = float((prob - want).abs().max())
    print("\n%s C=%d stride %d: prob max-abs %.3g vs softmax(upsample_bilinear)" % (hw, c, stride, err))
    assert err <= 1e-4
    assert torch.equal(label, _first_max(prob))
