"""irn_label_sweep_confusion (irn_amd/csrc/label.hip) through ops.label_sweep_confusion: exactly equal to the numpy
restatement (tests/_label_sweep_ref.py, proven against the oracle in tests/test_label_sweep_cpu.py) on every input of
tests/_label_cases.py, and to the shipped kernels (label_epilogue + label_confusion per threshold) on a batch of the
launch shapes — packed ground truth at odd addresses, the grid-stride iteration, c = 1 and 20, t = 256 (bins beyond any
LDS: the multi-pass path)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import irn_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _label_cases as LC  # noqa: E402
import _label_sweep_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = LC.label_cases()


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _host(hist):
    from irn_amd import ops
    conf, void = ops.cam_confusion_matrices(hist)
    return hist.cpu().numpy(), conf.cpu().numpy(), void.cpu().numpy()


def _oracle_conf(rw, size, keys, gt, t):
    _, lab, _ = O.sem_seg_epilogue(rw, size, keys, t)
    conf = np.zeros((21, 21), np.int64)
    void = np.zeros(21, np.int64)
    m = gt != 255
    np.add.at(conf, (gt[m].astype(np.int64), lab[m].astype(np.int64)), 1)
    np.add.at(void, lab[~m].astype(np.int64), 1)
    return conf, void


@pytest.mark.parametrize("t", [1, 7, 256])
def test_kernel_equals_restatement_and_oracle_on_every_label_case(t):
    from irn_amd import ops
    for n, (name, (rw, size, keys, _)) in enumerate(CASES):
        gt = S.ground_truth(size, seed=n)
        th = S.thresholds(rw, size, t, seed=n)
        hist, bad = ops.label_sweep_confusion([_t(rw)], [size], [_t(keys)], [_t(gt)], th)
        got_hist, got_conf, got_void = _host(hist)
        want_hist, want_bad = S.histogram(rw, size, keys, gt, th)
        assert int(bad.item()) == want_bad == 0, name
        assert np.array_equal(got_hist, want_hist), name
        want_conf, want_void = S.reduce(want_hist)
        assert np.array_equal(got_conf, want_conf) and np.array_equal(got_void, want_void), name
        for i in sorted(set(np.linspace(0, t - 1, 3).astype(int))):          # ... and the oracle's own composition
            oc, ov = _oracle_conf(rw, size, keys, gt, th[i])
            assert np.array_equal(got_conf[i], oc) and np.array_equal(got_void[i], ov), (name, i)


def _mixed():
    """[(rw, size, keys)]: 1x1 and 5x7 outputs, a 94x125 grid cropped to 375x500, the two big images whose 4-pixel groups
    exceed 128 chunks of 4096 pixels (a second grid-stride iteration), c = 1 and c = 20."""
    rng = np.random.RandomState(77)
    one = (np.full((2, 1, 1, 1), 0.3, np.float32) * np.float32([1, 2]).reshape(2, 1, 1, 1), (1, 1), np.int64([4, 9]))
    small = (np.abs(rng.randn(3, 1, 2, 2)).astype(np.float32), (5, 7), np.int64([0, 7, 19]))
    voc = np.abs(rng.randn(20, 1, 94, 125)).astype(np.float32) * 0.05
    for c in range(20):                                                        # every channel wins a block of its own
        voc[c, 0, 4 * c:4 * c + 6, 5 * c:5 * c + 30] = 0.3 + 0.03 * c
    voc20 = (voc, (375, 500), np.arange(20, dtype=np.int64))
    single = (np.abs(rng.randn(1, 1, 30, 41)).astype(np.float32), (118, 161), np.int64([11]))
    out = [one, small, single, voc20]
    for ow in (527, 528):
        rw, size, keys, _ = LC.big_case(ow)
        out.append((rw, size, keys))
    return out


def test_batch_equals_shipped_kernels_and_single_calls():
    from irn_amd import ops
    items = _mixed()
    rng = np.random.RandomState(5)
    gts = [S.ground_truth(size, seed=100 + i) for i, (_, size, _) in enumerate(items)]
    flat = _t(np.concatenate([g.reshape(-1) for g in gts]))
    offs = np.cumsum([0] + [g.size for g in gts])[:-1]
    assert sum(int(o) % 4 != 0 for o in offs[1:]) >= 4                         # packed: most maps start off a 4-byte boundary
    picks = [S.pixel_pairs(rw, size)[1].reshape(-1)[size[0] * size[1] // 3] for rw, size, _ in items[1:4]]     # exact scores
    assert len(set(picks)) == 3 and all(0 < p < 1 for p in picks)
    th = list(np.unique(np.float32(picks + [0.25, -0.5, 1.5])))
    for v in rng.uniform(0, 1.1, 400).astype(np.float32):
        if len(th) < 256 and v not in th:
            th.append(v)
    th = np.sort(np.float32(th))
    assert th.size == 256 and 257 * 22 * 20 > 15360
    rws, sizes, keys = [_t(i[0]) for i in items], [i[1] for i in items], [_t(i[2]) for i in items]
    hist, bad = ops.label_sweep_confusion(rws, sizes, keys, flat, th)
    assert int(bad.item()) == 0
    got_hist, got_conf, got_void = _host(hist)
    assert got_hist.sum() == sum(g.size for g in gts)
    # the shipped kernels at 5 thresholds, ties included
    dev_gts = [_t(g) for g in gts]
    checked = sorted({int(np.searchsorted(th, np.float32(0.25))), int(np.searchsorted(th, picks[0])),
                      int(np.searchsorted(th, picks[1])), 0, 255})
    assert len(checked) == 5
    for i in checked:
        labels = ops.label_epilogue(rws, sizes, float(th[i]), keys=keys)["labels"]
        conf = void = b = None
        for lab, g in zip(labels, dev_gts):
            conf, void, b = ops.label_confusion(lab, g, conf, b, pred_255_as=None, void=void)
        assert int(b.item()) == 0
        assert np.array_equal(got_conf[i], conf.cpu().numpy()) and np.array_equal(got_void[i], void.cpu().numpy()), i
    assert len({got_conf[i].tobytes() for i in checked}) > 1                   # the thresholds do change the labels
    # the batch = the sum of its images alone (list form of the ground truth)
    h1 = b1 = None
    for j in range(len(items)):
        h1, b1 = ops.label_sweep_confusion([rws[j]], [sizes[j]], [keys[j]], [dev_gts[j]], th, h1, b1)
    assert int(b1.item()) == 0 and torch.equal(h1, hist)
    # ... and the restatement, on the image with 20 channels
    h20, _ = ops.label_sweep_confusion([rws[3]], [sizes[3]], [keys[3]], [dev_gts[3]], th)
    want20 = S.histogram(items[3][0], items[3][1], items[3][2], gts[3], th)[0]
    assert np.array_equal(h20.cpu().numpy(), want20) and (want20.sum(axis=(0, 2)) > 0).sum() == 20


def test_all_zero_map_goes_to_the_first_key_at_every_threshold():
    from irn_amd import ops
    rw, size, keys, _ = dict(CASES)["all_zero"]
    gt = S.ground_truth(size, seed=3)
    th = np.float32([-1.0, 0.25, 1.0, 1e30])
    hist, bad = ops.label_sweep_confusion([_t(rw)], [size], [_t(keys)], [_t(gt)], th)
    h = hist.cpu().numpy()
    assert int(bad.item()) == 0 and h.sum() == gt.size and h[:, keys[0] + 1, 4].sum() == gt.size
    conf, void = ops.cam_confusion_matrices(hist)
    assert ((conf.sum(dim=1)[:, keys[0] + 1] + void[:, keys[0] + 1]) == gt.size).all()


def test_accumulation_and_bad_values():
    from irn_amd import ops
    rw, size, keys, _ = dict(CASES)["hot_seed1"]                                # 3 channels, 94 x 77
    gt = S.ground_truth(size, seed=9)
    th = S.thresholds(rw, size, 7, seed=9)
    hist, bad = ops.label_sweep_confusion([_t(rw)], [size], [_t(keys)], [_t(gt)], th)
    once = hist.clone()
    hist, bad = ops.label_sweep_confusion([_t(rw)], [size], [_t(keys)], [_t(gt)], th, hist, bad)
    assert torch.equal(hist, 2 * once) and int(bad.item()) == 0
    # GT 21..254: per pixel
    g2 = gt.copy()
    g2[0, :5] = 21
    g2[7, 3] = 254
    h2, b2 = ops.label_sweep_confusion([_t(rw)], [size], [_t(keys)], [_t(g2)], th)
    want, want_bad = S.histogram(rw, size, keys, g2, th)
    assert int(b2.item()) == want_bad == 6 and np.array_equal(h2.cpu().numpy(), want)
    # keys -1 and 20: the pixels whose best channel carries them, once each (also where the GT is bad too)
    for k_bad in (-1, 20):
        k2 = keys.copy()
        k2[1] = k_bad
        h3, b3 = ops.label_sweep_confusion([_t(rw)], [size], [_t(k2)], [_t(g2)], th)
        want, want_bad = S.histogram(rw, size, k2, g2, th)
        cstar = S.pixel_pairs(rw, size)[0]
        assert want_bad == 6 + int(((cstar == 1) & (g2 != 21) & (g2 != 254)).sum()) > 6
        assert int(b3.item()) == want_bad and np.array_equal(h3.cpu().numpy(), want)
    # a descending pair: once per call, whatever the number of blocks and images; the counts still follow the list as given
    th_bad = _t(np.float32([0.1, 0.5, 0.3, 0.7]))
    h4, b4 = ops.label_sweep_confusion([_t(rw), _t(rw)], [size, size], [_t(keys)] * 2, [_t(gt)] * 2, th_bad)
    assert int(b4.item()) == 1 and int(h4.sum().item()) == 2 * gt.size


def test_refusals_leave_the_accumulators_untouched():
    from irn_amd import ops
    rw, size, keys, _ = dict(CASES)["hot_seed1"]
    gt = S.ground_truth(size, seed=9)
    th = np.float32([0.1, 0.25])
    hist = torch.full((22, 21, 3), 7, dtype=torch.int64, device=_dev())
    bad = torch.full((1,), 5, dtype=torch.int64, device=_dev())
    good = ([_t(rw)], [size], [_t(keys)], [_t(gt)])

    def refused(rws=good[0], sizes=good[1], ks=good[2], gts=good[3], thres=th, h=hist, b=bad, exc=ValueError):
        with pytest.raises(exc):
            ops.label_sweep_confusion(rws, sizes, ks, gts, thres, h, b)

    refused(rws=[torch.from_numpy(rw)])                                         # CPU tensors
    refused(gts=[torch.from_numpy(gt)])
    refused(gts=[_t(gt[:-1])])                                                  # GT / output shape mismatch
    refused(gts=_t(gt.reshape(-1)[:-1]))                                        # packed buffer of the wrong length
    refused(thres=np.zeros(0, np.float32))                                      # t = 0
    refused(thres=np.linspace(0, 1, 257).astype(np.float32))                    # t = 257
    refused(thres=torch.linspace(0, 1, 257, device=_dev()), h=torch.zeros((22, 21, 258), dtype=torch.int64, device=_dev()))
    refused(rws=[_t(np.zeros((21, 1, 24, 20), np.float32))], ks=[_t(np.arange(21) % 20)])      # 21 channels
    refused(sizes=[(4 * 24 + 1, 77)], gts=[_t(np.zeros((97, 77), np.uint8))])    # out_h > 4h
    refused(h=torch.zeros((22, 21, 4), dtype=torch.int64, device=_dev()))       # accumulator of another t
    torch.cuda.synchronize()
    assert (hist == 7).all() and (bad == 5).all()
    # two images, the second one invalid at the C ABI (c = 21): nothing is launched for the first either
    from irn_amd._lib import _stream, i32_array, lib, ptr_array
    r, k, g, thd = _t(rw.reshape(3, 24, 20)), _t(keys), _t(gt), _t(th)
    scratch = torch.zeros(64, dtype=torch.int32, device=_dev())
    rc = lib.irn_label_sweep_confusion(2, ptr_array([r.data_ptr()] * 2), i32_array([3, 21]), i32_array([24, 24]), i32_array([20, 20]),
                                       i32_array([size[0]] * 2), i32_array([size[1]] * 2), ptr_array([k.data_ptr()] * 2),
                                       ptr_array([g.data_ptr()] * 2), thd.data_ptr(), 2, 21, hist.data_ptr(), bad.data_ptr(),
                                       scratch.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 1 and b"image 1" in lib.irn_last_error()
    assert (hist == 7).all() and (bad == 5).all()
