"""`ops.crf_prob` (irn_amd/csrc/crf.hip) against the numpy restatement tests/_prob_crf_ref.py.

The bars are those of tests/test_gpu_score_crf.py and tests/_parity.py: Q within 1e-4 max-abs of the float64 restatement, and a
label may differ only where the restatement's two best Q entries are a < TIE_TOL tie (and then the GPU picked an entry inside
that band), with no allowance on the count.  Reproducibility is bitwise."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _densecrf_ref as R  # noqa: E402
import _prob_crf_ref as P  # noqa: E402
from _parity import TIE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 48, 64
_KERNELS = {}


def _dev():
    return torch.device("cuda", 0)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _kernels(img, seed):
    """The restatement's pairwise kernels of one image, computed once and left unchanged."""
    key = (img.shape, seed)
    if key not in _KERNELS:
        _KERNELS[key] = R.Kernels(img)
    return _KERNELS[key]


def _check(img, prob, t, seed, what):
    from irn_amd import ops
    h, w = img.shape[:2]
    l = prob.shape[0]
    labels, q = ops.crf_prob(_gpu(img), _gpu(prob), t=t, want_q=True)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (h, w) and labels.is_cuda
    assert q.dtype == torch.float32 and tuple(q.shape) == (l, h, w)
    assert torch.equal(ops.crf_prob(_gpu(img), _gpu(prob), t=t), labels)            # without Q: the same map
    labels, q = labels.cpu().numpy(), q.cpu().numpy().reshape(l, -1)
    want = P.inference(img, prob, t=t, kernels=_kernels(img, seed) if t > 0 else None)
    err = float(np.abs(q - want).max())
    diff = (labels != P.labels_of(want, h, w)).reshape(-1)
    print("\n%s: Q max-abs %.3g vs the float64 restatement, %d of %d labels differ" % (what, err, int(diff.sum()), diff.size))
    assert err <= 1e-4, (what, err)
    if diff.any():
        gap = P.top2_gap(want)[diff]
        assert float(gap.max()) < TIE_TOL, "%s: %d pixels differ, one is not a tie (gap %.3g)" % (what, int(diff.sum()), float(gap.max()))
        cols = np.nonzero(diff)[0]
        assert (want[labels.reshape(-1)[cols], cols] >= want[:, cols].max(0) - TIE_TOL).all(), "%s: a pick outside the tie band" % what
    return labels


@pytest.mark.parametrize("l", [2, 4, 21])
@pytest.mark.parametrize("t", [0, 1, 10])
def test_q_and_labels_vs_restatement(t, l):
    from irn_amd import synth
    img = synth.photo(H, W, seed=5)
    labels = _check(img, P.random_prob(l, H, W, seed=l), t, 5, "t=%d l=%d" % (t, l))
    assert len(np.unique(labels)) >= 2


@pytest.mark.parametrize("l", [2, 4, 21, 32])
def test_t0_is_the_argmax_of_the_clipped_input(l):
    from irn_amd import ops, synth
    img = synth.photo(H, W, seed=5)
    prob = P.random_prob(l, H, W, seed=l)
    prob[0, :4] = 0.0                                                        # below the clip ...
    prob[1, :2] = -0.25                                                      # ... and below zero: both become 1e-5
    labels, q = ops.crf_prob(_gpu(img), _gpu(prob), t=0, want_q=True)
    clipped = np.maximum(prob, P.EPS)
    want = clipped / clipped.sum(0, dtype=np.float64)
    diff = labels.cpu().numpy() != np.argmax(clipped, 0).astype(np.uint8)
    assert not diff.any() or float(P.top2_gap(want)[diff].max()) < TIE_TOL, int(diff.sum())
    # one fp32 logarithm of a value in [1e-5, 1] (an ulp of 11.5 is 1e-6), one exponential and one product behind it
    assert float(np.abs(q.cpu().numpy() - want).max()) <= 1e-5
    flat = np.full((l, H, W), 1.0 / l, np.float32)                            # equal everywhere: the first label
    assert not ops.crf_prob(_gpu(img), _gpu(flat), t=0).any()


@pytest.mark.parametrize("h,w", [(1, 1), (1, 37), (29, 1)])
def test_degenerate_sizes_vs_restatement(h, w):
    from irn_amd import synth
    seed = h * 100 + w
    _check(synth.photo(h, w, seed=seed), P.random_prob(3, h, w, seed=seed), 10, seed, "%dx%d" % (h, w))


def test_nan_rule():
    """A pixel with a NaN has p' = 1 at its first NaN channel and 1e-5 elsewhere: a whole NaN channel wins everywhere at every
    t (its unary leads by log(1e5), the pairwise terms only add to it); single NaN pixels are pinned at t = 0 and held to the
    restatement at t = 10, where their neighbours can outvote them."""
    from irn_amd import ops, synth
    img = synth.photo(H, W, seed=7)
    prob = P.random_prob(4, H, W, seed=7)
    whole = prob.copy()
    whole[2] = np.nan
    for t in (0, 1, 10):
        assert bool((ops.crf_prob(_gpu(img), _gpu(whole), t=t) == 2).all()), t
    both = whole.copy()
    both[3] = np.nan                                                         # the first NaN channel wins
    assert bool((ops.crf_prob(_gpu(img), _gpu(both), t=10) == 2).all())
    single = prob.copy()
    pts = [(0, 0), (10, 20), (24, 32), (H - 1, W - 1)]
    for y, x in pts:
        single[1, y, x] = np.nan
    labels, q = ops.crf_prob(_gpu(img), _gpu(single), t=0, want_q=True)
    assert bool(torch.isfinite(q).all())
    for y, x in pts:
        assert int(labels[y, x]) == 1 and float(q[1, y, x]) > 0.9999
    _check(img, single, 10, 7, "single NaN pixels")


def test_two_calls_give_identical_bits():
    from irn_amd import ops, synth
    img, prob = _gpu(synth.photo(H, W, seed=3)), _gpu(P.random_prob(21, H, W, seed=3))
    a, qa = ops.crf_prob(img, prob, want_q=True)
    b, qb = ops.crf_prob(img, prob, want_q=True)
    assert torch.equal(a, b) and torch.equal(qa.view(torch.int32), qb.view(torch.int32))


def test_refusals_leave_the_labels_untouched():
    from irn_amd import _lib, ops, synth
    img, prob = _gpu(synth.photo(H, W, seed=2)), _gpu(P.random_prob(4, H, W, seed=2))
    for bad, match in ((prob[:, :-1], "prob"), (prob[0], "prob"), (prob.double(), "prob"), (prob[:1], "2..32"),
                       (torch.zeros((33, H, W), device=_dev()), "2..32")):
        with pytest.raises(ValueError, match=match):
            ops.crf_prob(img, bad)
    with pytest.raises(ValueError, match="iterations"):
        ops.crf_prob(img, prob, t=-1)
    need = int(_lib.lib.irn_crf_prob_workspace_bytes(H, W, 4))
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())
    labels = torch.full((H, W), 7, dtype=torch.uint8, device=_dev())

    def call(ws_bytes=need, l=4, t=10):
        return _lib.lib.irn_crf_prob(img.data_ptr(), prob.data_ptr(), l, H, W, t, labels.data_ptr(), None, ws.data_ptr(), ws_bytes,
                                     _lib._stream())
    assert call(ws_bytes=need - 1) == 3 and b"irn_crf_prob" in _lib.lib.irn_last_error() and b"workspace" in _lib.lib.irn_last_error()
    assert call(l=1) == 1 and call(l=33) == 1 and call(t=-1) == 1
    torch.cuda.synchronize()
    assert bool((labels == 7).all())
    assert call() == 0                                                       # ... and the same call with the workspace it asked for
    torch.cuda.synchronize()
    assert bool((labels < 4).all())
