"""The score-seeded dense CRF without a GPU: the numpy restatement tests/_score_crf_ref.py against the label
epilogue's own rule at T = 0, its NaN rule, its float32 arithmetic against its float64 one (the project's 1e-4 bar for fp32
must be reachable before a kernel is held to it), that the CRF changes labels at all, and the command line."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _densecrf_ref as R  # noqa: E402
import _score_crf_ref as S  # noqa: E402
from _parity import TIE_TOL  # noqa: E402

H, W = 48, 64
THETA = 0.25
_CACHE = {}


def _image():
    from irn_amd import synth
    return synth.photo(H, W, seed=5)


def _kernels(dtype):
    if dtype not in _CACHE:
        _CACHE[dtype] = R.Kernels(_image(), dtype)
    return _CACHE[dtype]


def _scores(c):
    from irn_amd import synth
    return synth.cam_blobs(c, H, W, seed=c)


def _q10(c, dtype):
    key = ("q", c, dtype)
    if key not in _CACHE:
        _CACHE[key] = S.inference(_image(), _scores(c), THETA, t=10, dtype=dtype, kernels=_kernels(dtype))
    return _CACHE[key]


def _edge_scores(c, theta, seed):
    """Scores whose entries sit exactly on the threshold, one ulp either side, at zero, below zero and below the clip; in the
    second half of the scenarios two classes share the value."""
    f32 = np.float32
    th = f32(theta)
    vals = [th, np.nextafter(th, f32(-1)), np.nextafter(th, f32(1)), f32(0), f32(-0.0), f32(-0.3), f32(3e-6), f32(0.7), f32(1)]
    rng = np.random.RandomState(seed)
    v = (rng.rand(c, H * W) * 0.2 - 0.05).astype(f32)
    for p in range(H * W):
        s = p % (2 * len(vals))
        c1 = int(rng.randint(c))
        v[c1, p] = vals[s % len(vals)]
        if s >= len(vals) and c > 1:
            v[(c1 + 1 + int(rng.randint(c - 1))) % c, p] = vals[s % len(vals)]
    return v.reshape(c, H, W)


@pytest.mark.parametrize("theta", [0.25, 1e-5, 0.05])
@pytest.mark.parametrize("c", [1, 3, 20])
def test_t0_is_the_epilogue_rule_up_to_ties(c, theta):
    keys = np.sort(np.random.RandomState(c).choice(20, c, replace=False))
    for scores in (_edge_scores(c, theta, seed=c), _scores(c)):
        for dtype in (np.float64, np.float32):
            q = S.inference(None, scores, theta, t=0, dtype=dtype)
            got, want = S.labels_of(q, keys, H, W), S.epilogue_rule(scores, theta, keys)
            diff = (got != want).reshape(-1)
            if diff.any():
                gap = S.top2_gap(q)[diff]
                assert float(gap.max()) < TIE_TOL, (c, theta, dtype, int(diff.sum()), float(gap.max()))
    # Q0 = s' / sum(s'): the definition, spelt out
    s = S.clamped_scores(scores, theta).astype(np.float64)
    assert np.abs(S.inference(None, scores, theta, t=0) - s / s.sum(0)).max() < 1e-12


def test_nan_rule():
    c = 3
    scores = _scores(c).copy()
    scores[1, 0, 0] = np.nan                      # first NaN channel 1
    scores[:, 0, 1] = np.nan                      # every channel: the first one wins
    scores[2, 0, 2] = np.nan
    scores[0, 0, 2] = 5.0                         # a NaN beats any number, as in the epilogue
    s = S.clamped_scores(scores, THETA)
    assert s.dtype == np.float32
    for px, ch in ((0, 1), (1, 0), (2, 2)):
        want = np.full(c + 1, S.EPS, np.float32)
        want[ch + 1] = 1
        assert np.array_equal(s[:, px], want), (px, s[:, px])
    keys = np.array([2, 7, 14])
    for theta in (1e-5, 0.25, 0.99):
        lab = S.labels_of(S.inference(None, scores, theta, t=0), keys, H, W)
        assert [int(lab[0, 0]), int(lab[0, 1]), int(lab[0, 2])] == [8, 3, 15]
    assert np.isfinite(S.neg_unary(scores, THETA)).all()
    for bad in (0.0, 9e-6, -1.0, float("nan")):
        with pytest.raises(ValueError, match="below the clip"):
            S.clamped_scores(scores, bad)


@pytest.mark.parametrize("c", [1, 3, 20])
def test_float32_restatement_within_1e_4_of_float64_and_the_crf_changes_labels(c):
    q64, q32 = _q10(c, np.float64), _q10(c, np.float32)
    assert q32.dtype == np.float32
    err = float(np.abs(q32 - q64).max())
    print("c=%d: float32 vs float64 max-abs %.3g" % (c, err))
    assert err <= 1e-4, (c, err)
    assert np.abs(q64.sum(0) - 1).max() < 1e-9
    keys = np.arange(c)
    before = S.labels_of(S.inference(None, _scores(c), THETA, t=0), keys, H, W)
    after = S.labels_of(q64, keys, H, W)
    changed = int((before != after).sum())
    print("c=%d: the CRF changed %d of %d pixels" % (c, changed, H * W))
    assert changed > 0, c


def test_parser_and_tune_axes():
    import run_sample
    from irn_amd import ops
    from irn_amd.step import _labels, tune_sem_seg as T
    p = run_sample.build_parser()
    assert p.parse_args(["--voc12_root", "x"]).sem_seg_crf_iters == 0
    assert p.parse_args(["--voc12_root", "x", "--sem_seg_crf_iters", "10"]).sem_seg_crf_iters == 10
    with pytest.raises(SystemExit):
        p.parse_args(["--voc12_root", "x", "--sem_seg_crf_iters", "-1"])
    assert _labels.crf_iters(argparse.Namespace()) == 0                 # args built by hand, without the flag

    def args(**kw):
        base = dict(beta=10.0, exp_times=8, sem_seg_bg_thres=0.25, tune_beta=[], tune_exp_times=[], tune_bg_thres=[])
        base.update(kw)
        return argparse.Namespace(**base)
    sixteen, seventeen = list(np.linspace(0.3, 0.9, 15)), list(np.linspace(0.3, 0.9, 16))     # + the configured one
    assert len(T.grid_axes(args(tune_bg_thres=seventeen))[3]) == 17
    assert len(T.grid_axes(args(tune_bg_thres=seventeen, sem_seg_crf_iters=0))[3]) == 17
    assert len(T.grid_axes(args(tune_bg_thres=sixteen, sem_seg_crf_iters=10))[3]) == 16 == ops.CRF_MAX_SWEEP
    with pytest.raises(ValueError, match="17 background thresholds.*IRN_CRF_MAX_SWEEP"):
        T.grid_axes(args(tune_bg_thres=seventeen, sem_seg_crf_iters=10))
    with pytest.raises(ValueError, match="at least 1e-05"):
        T.grid_axes(args(tune_bg_thres=[0.0], sem_seg_crf_iters=10))
    T.grid_axes(args(tune_bg_thres=[0.0]))                                                   # fine without the CRF


def test_step_refuses_host_preprocessing_with_the_crf_on():
    from irn_amd.step import make_sem_seg_labels as M
    with pytest.raises(ValueError, match="sem_seg_crf_iters.*device_preprocess"):
        M.run(argparse.Namespace(sem_seg_crf_iters=10, device_preprocess=False, sem_seg_bg_thres=0.25))
    with pytest.raises(ValueError, match="at least 1e-05"):
        M.run(argparse.Namespace(sem_seg_crf_iters=10, sem_seg_bg_thres=0.0))
