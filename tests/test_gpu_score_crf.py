"""`ops.crf_score_sweep` (irn_amd/csrc/crf.hip) against the numpy restatement tests/_score_crf_ref.py.

The bars are those of tests/test_gpu_crf.py and tests/_parity.py: Q within 1e-4 max-abs of the float64 restatement, and a
label may differ only where the restatement's two best Q entries are a < TIE_TOL tie (and then the GPU picked an entry inside
that band), with no allowance on the count.  The restatement is fed the GPU's own `rw_up`: the epilogue is tested elsewhere.
Chunk independence and reproducibility are bitwise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _densecrf_ref as R  # noqa: E402
import _score_crf_ref as S  # noqa: E402
from _parity import TIE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 48, 64
_KERNELS = {}


def _dev():
    return torch.device("cuda", 0)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _keys(c, seed):
    return (np.sort(np.random.RandomState(seed).choice(20, c, replace=False)) if c <= 20 else np.arange(c)).astype(np.int64)


def _walk_scores(c, h, w, seed, rw=None):
    """(rw, GPU fp32 [c,h,w]): the `rw_up` the label epilogue computes from a synthetic quarter-resolution walk output."""
    from irn_amd import ops, synth
    if rw is None:
        rw = synth.cam_blobs(c, (h + 3) // 4, (w + 3) // 4, seed=seed)
    up = ops.label_epilogue([_gpu(rw)[:, None]], [(h, w)], 0.25, want_labels=False, want_rw_up=True)["rw_up"][0]
    return rw, up


def _case(c, h, w, seed):
    from irn_amd import synth
    img = synth.photo(h, w, seed=seed)
    return img, _walk_scores(c, h, w, seed)[1], _keys(c, seed)


def _kernels(img, seed):
    """The restatement's pairwise kernels of one image, computed once and left unchanged."""
    key = (img.shape, seed)
    if key not in _KERNELS:
        _KERNELS[key] = R.Kernels(img)
    return _KERNELS[key]


def _assert_parity(plane, q_want, keys, what):
    """plane uint8 [H,W] of the GPU; q_want the restatement's Q [L, H*W]."""
    h, w = plane.shape
    want = S.labels_of(q_want, keys, h, w)
    diff = (plane != want).reshape(-1)
    if not diff.any():
        return 0
    gap = S.top2_gap(q_want)[diff]
    assert float(gap.max()) < TIE_TOL, "%s: %d pixels differ, one is not a tie (gap %.3g)" % (what, int(diff.sum()), float(gap.max()))
    index_of = {0: 0, **{int(k) + 1: i + 1 for i, k in enumerate(keys)}}
    pick = np.array([index_of[int(v)] for v in plane.reshape(-1)[diff]])
    cols = np.nonzero(diff)[0]
    assert (q_want[pick, cols] >= q_want[:, cols].max(0) - TIE_TOL).all(), "%s: a differing pixel chose an entry outside the tie band" % what
    return int(diff.sum())


def _check_against_restatement(img, up, keys, thres, t, seed, what):
    from irn_amd import ops
    h, w = img.shape[:2]
    c = len(keys)
    planes, q = ops.crf_score_sweep(_gpu(img), up, keys, thres, t=t, want_q=True)
    assert planes.dtype == torch.uint8 and tuple(planes.shape) == (len(thres), h, w) and planes.is_cuda
    assert q.dtype == torch.float32 and tuple(q.shape) == (len(thres), c + 1, h, w)
    planes, q, scores = planes.cpu().numpy(), q.cpu().numpy(), up.cpu().numpy()
    kern = _kernels(img, seed) if t > 0 else None
    for i, th in enumerate(thres):
        q_want = S.inference(img, scores, th, t=t, kernels=kern)
        err = float(np.abs(q[i].reshape(c + 1, -1) - q_want).max())
        print("%s thres %g: Q max-abs %.3g" % (what, th, err))
        assert err <= 1e-4, (what, th, err)
        _assert_parity(planes[i], q_want, keys, "%s thres %g" % (what, th))
    return planes


@pytest.mark.parametrize("c", [1, 3, 20])
@pytest.mark.parametrize("t", [0, 1, 10])
def test_q_and_labels_vs_restatement(t, c):
    img, up, keys = _case(c, H, W, seed=5)
    planes = _check_against_restatement(img, up, keys, [0.05, 0.25], t, 5, "t=%d c=%d" % (t, c))
    assert len(np.unique(planes)) >= 2


@pytest.mark.parametrize("h,w", [(1, 1), (1, 37), (29, 1), (7, 5)])
def test_degenerate_lattices_vs_restatement(h, w):
    img, up, keys = _case(2, h, w, seed=h * 100 + w)
    _check_against_restatement(img, up, keys, [0.25], 10, h * 100 + w, "%dx%d" % (h, w))


@pytest.mark.parametrize("c", [1, 3, 20])
def test_t0_is_the_epilogue_label_map(c):
    from irn_amd import ops, synth
    img = synth.photo(H, W, seed=5)
    rw, up = _walk_scores(c, H, W, seed=5)
    keys = _keys(c, 5)
    for th in (0.05, 0.25, 0.6):
        want = ops.label_epilogue([_gpu(rw)[:, None]], [(H, W)], th, keys=[_gpu(keys)])["labels"][0].cpu().numpy()
        got = ops.crf_score_sweep(_gpu(img), up, keys, [th], t=0).cpu().numpy()[0]
        q = S.inference(None, up.cpu().numpy(), th, t=0)
        diff = (got != want).reshape(-1)
        if diff.any():
            gap = S.top2_gap(q)[diff]
            assert float(gap.max()) < TIE_TOL, (c, th, int(diff.sum()), float(gap.max()))
        assert len(np.unique(want)) >= 2                                    # not vacuous: the epilogue's map has several labels


@pytest.mark.parametrize("c,n_t", [(20, 4), (31, 3)])                       # chunks of 3 + 1 and of 2 + 1 CRFs
def test_plane_does_not_depend_on_its_chunk_and_calls_repeat_bit_for_bit(c, n_t):
    from irn_amd import ops
    img, up, keys = _case(c, H, W, seed=c)
    thres = np.linspace(0.05, 0.6, n_t).astype(np.float32)
    planes, q = ops.crf_score_sweep(_gpu(img), up, keys, thres, want_q=True)
    again, q2 = ops.crf_score_sweep(_gpu(img), up, keys, thres, want_q=True)
    assert torch.equal(planes, again) and torch.equal(q, q2)
    for i, th in enumerate(thres):
        one, q1 = ops.crf_score_sweep(_gpu(img), up, keys, [th], want_q=True)
        assert torch.equal(one[0], planes[i]), (c, i)
        assert torch.equal(q1[0], q[i]), (c, i)
    assert (planes != planes[0]).any()                                      # not vacuous: the planes differ


def test_voc_size_sweep_of_16_equals_16_single_calls():
    from irn_amd import ops
    h, w = 375, 500
    img, up, keys = _case(3, h, w, seed=11)
    thres = np.linspace(0.05, 0.8, 16).astype(np.float32)
    rgb = _gpu(img)
    planes = ops.crf_score_sweep(rgb, up, keys, thres)
    for i, th in enumerate(thres):
        assert torch.equal(ops.crf_score_sweep(rgb, up, keys, [th])[0], planes[i]), i
    assert (planes != planes[0]).any()


def test_no_classes_gives_zeros_without_a_workspace():
    from irn_amd import _lib, ops, synth
    h, w = 7, 5
    img = synth.photo(h, w, seed=1)
    out = torch.full((3, h, w), 9, dtype=torch.uint8, device=_dev())
    got, q = ops.crf_score_sweep(_gpu(img), torch.zeros((0, h, w), device=_dev()), np.zeros(0, np.int64), [0.1, 0.2, 0.3], out=out,
                                 want_q=True)
    assert got is out and not out.any() and tuple(q.shape) == (3, 1, h, w) and bool((q == 1).all())
    planes = torch.full((2, h, w), 7, dtype=torch.uint8, device=_dev())
    th = (C.c_float * 2)(0.1, 0.2)
    rc = _lib.lib.irn_crf_score_sweep(_gpu(img).data_ptr(), None, None, 0, h, w, th, 2, 10, planes.data_ptr(), None, None, 0,
                                      _lib._stream())
    assert rc == 0 and not planes.any()


def test_nan_scores():
    """The NaN rule.  A NaN reaches the scores through the walk, and the epilogue divides by the image's global
    maximum, so a NaN channel is NaN at every pixel: then every pixel's unary favours that channel's label by log(1e5) over
    every other one, the pairwise terms only add to it, and the map is keys[channel] + 1 at every threshold and every T.  A
    single NaN pixel inside another label's region has the same unary but its neighbours can outvote it after some iterations
    (3 + 10 > log(1e5)): it is pinned at T = 0 and held to the restatement at T = 10."""
    from irn_amd import ops
    img, up, keys = _case(3, H, W, seed=7)
    thres = [1e-5, 0.05, 0.25, 0.9]
    whole = up.clone()
    whole[1] = float("nan")
    for t in (0, 1, 10):
        planes = ops.crf_score_sweep(_gpu(img), whole, keys, thres, t=t).cpu().numpy()
        assert (planes == keys[1] + 1).all(), (t, np.unique(planes))
    both = whole.clone()
    both[2] = float("nan")                                                   # the first NaN channel wins
    assert (ops.crf_score_sweep(_gpu(img), both, keys, thres, t=10) == int(keys[1]) + 1).all()
    single = up.clone()
    pts = [(0, 0), (10, 20), (24, 32), (H - 1, W - 1)]
    for y, x in pts:
        single[1, y, x] = float("nan")
    planes = ops.crf_score_sweep(_gpu(img), single, keys, thres, t=0).cpu().numpy()
    for y, x in pts:
        assert (planes[:, y, x] == keys[1] + 1).all(), (y, x, planes[:, y, x])
    _check_against_restatement(img, single, keys, [0.05, 0.25], 10, 7, "single NaN pixels")


def test_zero_plane_and_scores_on_the_threshold():
    from irn_amd import ops
    img, up, keys = _case(3, H, W, seed=9)
    zero = up.clone()
    zero[0] = 0                                                              # a class the walk never reached: clamped to the clip
    zero[2, :, : W // 2] = -0.125                                            # ... and a stretch below zero
    planes = _check_against_restatement(img, zero, keys, [0.05, 0.25], 10, 9, "zero plane")
    assert not (planes == keys[0] + 1).any()
    th = np.float32(0.25)
    tie = torch.minimum(up, torch.tensor(float(np.nextafter(th, np.float32(0))), device=_dev()))
    tie[1, ::2] = float(th)                                                  # exactly the threshold on every other row
    tie[2, ::4] = float(th)                                                  # ... two classes there on every fourth
    got = ops.crf_score_sweep(_gpu(img), tie, keys, [th], t=0).cpu().numpy()[0]
    assert not got.any()                                                     # equal unaries: the first maximum is the background
    _check_against_restatement(img, tie, keys, [th], 10, 9, "scores on the threshold")


def test_refusals_leave_the_planes_untouched():
    from irn_amd import _lib, ops
    img, up, keys = _case(3, H, W, seed=2)
    rgb = _gpu(img)

    def refused(exc, match, thres, scores=up, ks=keys, **kw):
        out = torch.full((len(thres), H, W), 7, dtype=torch.uint8, device=_dev())
        with pytest.raises(exc, match=match):
            ops.crf_score_sweep(rgb, scores, ks, thres, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == 7).all()), match

    refused(ValueError, "at least 1e-05", [9e-6, 0.25])
    refused(ValueError, "at least 1e-05", [0.0])
    refused(ValueError, "at least 1e-05", [-0.5, 0.25])
    refused(ValueError, "ascending", [0.3, 0.2])
    refused(ValueError, "ascending", [0.3, 0.3])
    refused(ValueError, "ascending", [0.1, float("nan")])
    refused(ValueError, "scores", [0.25], scores=up[:, :-1])
    refused(ValueError, "scores", [0.25], scores=up[0])
    refused(ValueError, "keys", [0.25], ks=keys[:2])
    refused(ValueError, "iterations", [0.25], t=-1)
    with pytest.raises(ValueError, match="1..16"):
        ops.crf_score_sweep(rgb, up, keys, [])
    with pytest.raises(ValueError, match="1..16"):
        ops.crf_score_sweep(rgb, up, keys, np.linspace(0.1, 0.9, 17))
    wide = torch.zeros((32, H, W), device=_dev())                            # c = 32: 33 labels
    refused(ValueError, "at most 31", [0.25], scores=wide, ks=np.arange(32))
    with pytest.raises(ValueError, match="out must be"):
        ops.crf_score_sweep(rgb, up, keys, [0.25], out=torch.zeros((2, H, W), dtype=torch.uint8, device=_dev()))

    # the C entry's own refusals, past the wrapper: IRN_ERR_ARG = 1 before any device work, a short workspace IRN_ERR_STATE = 3
    ks = _gpu(keys)
    need = int(_lib.lib.irn_crf_score_sweep_workspace_bytes(H, W, 4, 2))
    assert need > 0 and _lib.lib.irn_crf_score_sweep_workspace_bytes(H, W, 33, 1) == 0
    assert _lib.lib.irn_crf_score_sweep_workspace_bytes(H, W, 4, 0) == 0 == _lib.lib.irn_crf_score_sweep_workspace_bytes(H, W, 4, 17)
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())
    planes = torch.full((17, H, W), 7, dtype=torch.uint8, device=_dev())

    def call(th, n_t, c=3, t=10, ws_bytes=need, scores=up):
        arr = (C.c_float * max(len(th), 1))(*th)
        return _lib.lib.irn_crf_score_sweep(rgb.data_ptr(), scores.data_ptr(), ks.data_ptr(), c, H, W, arr, n_t, t, planes.data_ptr(),
                                            None, ws.data_ptr(), ws_bytes, _lib._stream())
    for th, n_t, kw, msg in (([9e-6, 0.25], 2, {}, b"below"), ([0.3, 0.2], 2, {}, b"ascending"), ([0.1, float("nan")], 2, {}, b"NaN"),
                             ([0.1], 0, {}, b"t_count"), ([0.1] * 17, 17, {}, b"t_count"), ([0.1, 0.2], 2, {"c": 32}, b"n_labels"),
                             ([0.1, 0.2], 2, {"c": -1}, b"bad argument"), ([0.1, 0.2], 2, {"t": -1}, b"bad argument")):
        assert call(th, n_t, **kw) == 1 and msg in _lib.lib.irn_last_error(), (th, n_t, kw, _lib.lib.irn_last_error())
    assert call([0.1, 0.2], 2, ws_bytes=need - 1) == 3 and b"workspace" in _lib.lib.irn_last_error()
    torch.cuda.synchronize()
    assert bool((planes == 7).all())
    assert call([0.1, 0.2], 2) == 0                                          # ... and the same call with the workspace it asked for
    torch.cuda.synchronize()
    assert bool((planes[:2] != 7).all()) and bool((planes[2:] == 7).all())
