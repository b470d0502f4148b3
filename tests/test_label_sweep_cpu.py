"""The one-pass formulation of irn_label_sweep_confusion, proven without a GPU: on every input of tests/_label_cases.py the
histogram of tests/_label_sweep_ref.py (per pixel the first arg-max channel, its score and the NaN rule), reduced as
`k_cam_reduce` reduces it, equals at EVERY threshold the chainercv confusion (tests/_eval_ref.py) of the labels the oracle's
epilogue writes at that threshold — integer for integer.  The thresholds contain 0.25, a negative value, one above 1 and the
exact float32 scores of several pixels, so the `thres == m` side of the tie (background, the epilogue's strict >) is
exercised.  Also: the C entry point and the op refuse loudly without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import irn_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_ref as E  # noqa: E402
import _label_cases as LC  # noqa: E402
import _label_sweep_ref as S  # noqa: E402

CASES = LC.label_cases()
T = 9


def _composed(rw, size, keys, gt, th):
    """conf [T,21,21], void [T,21] from the oracle's epilogue per threshold + the chainercv confusion."""
    conf = np.zeros((len(th), 21, 21), np.int64)
    void = np.zeros((len(th), 21), np.int64)
    g = gt.astype(np.int32)
    g[gt == 255] = -1
    for i, t in enumerate(th):
        _, lab, _ = O.sem_seg_epilogue(rw, size, keys, t)
        c = E.calc_semantic_segmentation_confusion([lab], [g])
        conf[i, :c.shape[0], :c.shape[1]] = c
        void[i] = np.bincount(lab[gt == 255].astype(np.int64), minlength=21)
    return conf, void


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_restated_histogram_equals_the_composed_reference(name, case):
    rw, size, keys, _ = case
    n = [c[0] for c in CASES].index(name)
    gt = S.ground_truth(size, seed=n)
    if gt.size >= 22:
        assert set(np.unique(gt)) == set(range(21)) | {255}
    th = S.thresholds(rw, size, T, seed=n)
    assert len(th) == T and (np.diff(th) > 0).all() and np.float32(0.25) in th and th[0] < 0 and th[-1] > 1
    _, m, nan = S.pixel_pairs(rw, size)
    if not nan.all():
        assert np.isin(th, m[~nan]).sum() >= 1, "no threshold equals a pixel's score"
    hist, bad = S.histogram(rw, size, keys, gt, th)
    assert bad == 0 and hist.sum() == gt.size
    conf, void = S.reduce(hist)
    want_conf, want_void = _composed(rw, size, keys, gt, th)
    assert np.array_equal(conf, want_conf) and np.array_equal(void, want_void)


def test_all_zero_map_lands_in_the_first_key_at_every_threshold():
    rw, size, keys, _ = dict(CASES)["all_zero"]
    gt = S.ground_truth(size, seed=3)
    th = np.float32([-1.0, 0.25, 1e30])
    hist, bad = S.histogram(rw, size, keys, gt, th)
    assert bad == 0 and hist[:, keys[0] + 1, 3].sum() == gt.size == hist.sum()
    conf, void = S.reduce(hist)
    assert (conf.sum(axis=1)[:, keys[0] + 1] + void[:, keys[0] + 1] == gt.size).all()


def test_restatement_counts_bad_values():
    rw, size, keys, _ = dict(CASES)["hot_seed0"]
    gt = S.ground_truth(size, seed=1)
    gt[0, :5] = 21
    gt[1, 0] = 254
    _, bad = S.histogram(rw, size, keys, gt, np.float32([0.5, 0.25, 0.3]))
    assert bad == 6 + 1


def test_entry_point_and_op_fail_loudly_without_gpu():
    import torch
    from irn_amd import _lib, ops
    L = _lib.lib
    one = C.c_void_p(64)                                                        # never dereferenced on these paths
    ptrs, i1 = _lib.ptr_array([64]), _lib.i32_array([1])
    assert L.irn_label_sweep_confusion(0, ptrs, i1, i1, i1, i1, i1, ptrs, ptrs, one, 1, 21, one, one, one, None) == 1
    assert b"irn_label_sweep_confusion" in L.irn_last_error()
    assert L.irn_label_sweep_confusion(1, ptrs, i1, i1, i1, i1, i1, ptrs, ptrs, one, 0, 21, one, one, one, None) == 1      # t < 1
    assert L.irn_label_sweep_confusion(1, ptrs, i1, i1, i1, i1, i1, ptrs, ptrs, one, 257, 21, one, one, one, None) == 1    # t over the cap
    assert L.irn_label_sweep_confusion(1, ptrs, _lib.i32_array([21]), i1, i1, i1, i1, ptrs, ptrs, one, 1, 21, one, one, one, None) == 1
    assert L.irn_label_sweep_confusion(1, ptrs, i1, i1, i1, _lib.i32_array([5]), i1, ptrs, ptrs, one, 1, 21, one, one, one, None) == 1
    assert L.irn_label_sweep_confusion(1, ptrs, i1, i1, i1, i1, i1, None, ptrs, one, 1, 21, one, one, one, None) == 1      # no keys
    assert L.irn_label_sweep_confusion(1, ptrs, i1, i1, i1, i1, i1, ptrs, _lib.ptr_array([None]), one, 1, 21, one, one, one, None) == 1
    assert L.irn_label_sweep_confusion(1, ptrs, i1, i1, i1, i1, i1, ptrs, ptrs, one, 1, 21, None, one, one, None) == 1     # no accumulator
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.label_sweep_confusion([torch.zeros(1, 2, 2)], [(8, 8)], [[3]], [torch.zeros(8, 8, dtype=torch.uint8)], [0.25])
    if not torch.cuda.is_available():
        # valid arguments: the call reaches the device and reports it, no crash
        assert L.irn_label_sweep_confusion(1, ptrs, i1, i1, i1, i1, i1, ptrs, ptrs, one, 1, 21, one, one, one, None) == 2
        assert L.irn_last_error()
