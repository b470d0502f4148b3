"""The evaluation counting kernels (irn_amd/csrc/eval.hip) exactly against numpy, and the eval_cam / eval_sem_seg /
eval_ins_seg steps end to end through run_sample.py against the chainercv restatement tests/_eval_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_ref as R  # noqa: E402
import _steps as S  # noqa: E402

pytestmark = pytest.mark.gpu

os.environ.setdefault("MIOPEN_FIND_MODE", "2")     # fast find: the backbones are plumbing here, not the subject

CAP = 256
LEVELS = np.float32([0.0, 0.125, 0.15, 0.25, 0.5, 0.75, 1.0])   # CAM values: planted ties between planes and thresholds


def _dev():
    return torch.device("cuda", 0)


def _gt(h, w, rng):
    gt = rng.randint(0, 21, (h, w)).astype(np.uint8)
    gt[rng.rand(h, w) < 0.1] = 255
    if h > 4 and w > 4:
        gt[h // 3:h // 2, :] = 255                        # a void band
    return gt


def _cams(k, h, w, rng):
    cams = rng.choice(LEVELS, (k, h, w)).astype(np.float32)
    cams[:, rng.rand(h, w) < 0.3] = rng.choice(LEVELS)        # equal maxima across planes, equal to a threshold
    smooth = rng.rand(k, h, w).astype(np.float32)
    return np.where(rng.rand(k, h, w) < 0.5, cams, smooth).astype(np.float32)


def _thresholds(t, rng):
    if t == 1:
        return np.float32([0.15])
    th = np.unique(np.concatenate([LEVELS, rng.rand(t).astype(np.float32)]))[:t]
    assert len(th) == t
    return th


def _want_cam(cams, keys, gt, th):
    conf = np.zeros((len(th), 21, 21), np.int64)
    void = np.zeros((len(th), 21), np.int64)
    keys_pad = np.pad(np.asarray(keys) + 1, (1, 0), mode="constant")
    g = gt.astype(np.int64)
    for i, t in enumerate(th):
        pred = keys_pad[np.argmax(np.pad(cams, ((1, 0), (0, 0), (0, 0)), mode="constant", constant_values=t), axis=0)]
        m = g != 255
        np.add.at(conf[i], (g[m], pred[m]), 1)
        np.add.at(void[i], pred[~m], 1)
    return conf, void


@pytest.mark.parametrize("h,w", [(1, 1), (7, 5), (500, 375), (375, 500)])
@pytest.mark.parametrize("k", [0, 1, 3, 20])
@pytest.mark.parametrize("t", [1, 100, CAP])
def test_cam_confusion_exact(h, w, k, t):
    from irn_amd import ops
    rng = np.random.RandomState(h * 7 + w * 3 + k * 11 + t)
    gt = _gt(h, w, rng)
    cams = _cams(k, h, w, rng) if k else np.zeros((0, h, w), np.float32)
    keys = np.sort(rng.choice(20, k, replace=False)).astype(np.int64)
    th = _thresholds(t, rng)
    hist, bad = ops.cam_confusion(torch.from_numpy(cams).to(_dev()), torch.from_numpy(keys), torch.from_numpy(gt).to(_dev()), th)
    conf, void = ops.cam_confusion_matrices(hist)
    want_conf, want_void = _want_cam(cams, keys, gt, th)
    assert int(bad.item()) == 0
    assert np.array_equal(conf.cpu().numpy(), want_conf)
    assert np.array_equal(void.cpu().numpy(), want_void)


def test_cam_confusion_accumulates_and_counts_bad_values():
    from irn_amd import ops
    rng = np.random.RandomState(5)
    th = _thresholds(100, rng)
    hist = bad = None
    want_conf = want_void = 0
    for i, (h, w, k) in enumerate([(33, 47, 2), (64, 20, 0), (90, 91, 5)]):
        gt = _gt(h, w, rng)
        cams = _cams(k, h, w, rng) if k else np.zeros((0, h, w), np.float32)
        keys = np.sort(rng.choice(20, k, replace=False))
        hist, bad = ops.cam_confusion(torch.from_numpy(cams).to(_dev()), keys, torch.from_numpy(gt).to(_dev()), th, hist, bad)
        c, v = _want_cam(cams, keys, gt, th)
        want_conf, want_void = want_conf + c, want_void + v
    conf, void = ops.cam_confusion_matrices(hist)
    assert int(bad.item()) == 0
    assert np.array_equal(conf.cpu().numpy(), want_conf) and np.array_equal(void.cpu().numpy(), want_void)
    # GT 21 and a NaN: skipped and counted
    gt = _gt(20, 30, rng)
    gt[0, :5] = 21
    gt[1, 0] = 200
    cams = _cams(2, 20, 30, rng)
    cams[1, 5, 5] = np.nan
    gt[5, 5] = 3
    hist2, bad2 = ops.cam_confusion(torch.from_numpy(cams).to(_dev()), [4, 9], torch.from_numpy(gt).to(_dev()), th)
    assert int(bad2.item()) == 7
    conf2, _ = ops.cam_confusion_matrices(hist2)
    assert int(conf2[0].sum()) + int(((gt == 255)).sum()) == 20 * 30 - 7


def test_cam_confusion_bad_keys_and_descending_thresholds():
    from irn_amd import ops
    rng = np.random.RandomState(11)
    h, w = 130, 70                                            # 9100 pixels: three blocks of 4096
    gt = _gt(h, w, rng)
    cams = _cams(3, h, w, rng)
    th = _thresholds(100, rng)
    cstar, m = np.argmax(cams, axis=0), cams.max(axis=0)      # first arg-max plane; no NaN, every GT value in range
    j = np.searchsorted(th, m, side="left")                   # number of thresholds < m
    row = np.where(gt == 255, 21, gt).astype(np.int64)
    on_plane = cstar == 1
    assert 0 < on_plane.sum() < h * w and (on_plane & (gt == 255)).any()
    # keys -1 and 20 on plane 1: its pixels are counted as bad, once each, and left out of the histogram
    for k_bad in (-1, 20):
        keys = np.int64([4, k_bad, 9])
        hist, bad = ops.cam_confusion(torch.from_numpy(cams).to(_dev()), keys, torch.from_numpy(gt).to(_dev()), th)
        want = np.zeros((22, 21, len(th) + 1), np.int64)
        np.add.at(want, (row[~on_plane], keys[cstar[~on_plane]] + 1, j[~on_plane]), 1)
        assert int(bad.item()) == int(on_plane.sum())
        assert np.array_equal(hist.cpu().numpy(), want)
    # a descending pair, as a float32 GPU tensor (which `eval_thresholds` never sees): once per call whatever the number
    # of blocks; the counts still follow the list as given
    th_bad = torch.from_numpy(np.float32([0.5, 0.3])).to(_dev())
    for hh, ww in [(33, 47), (h, w)]:
        g = _gt(hh, ww, rng)
        c = _cams(3, hh, ww, rng)
        hist, bad = ops.cam_confusion(torch.from_numpy(c).to(_dev()), [4, 7, 9], torch.from_numpy(g).to(_dev()), th_bad)
        assert int(bad.item()) == 1
        assert int(hist.sum().item()) == hh * ww


@pytest.mark.parametrize("h,w", [(1, 1), (7, 5), (500, 375)])
def test_label_confusion_exact(h, w):
    from irn_amd import ops
    rng = np.random.RandomState(h + w)
    conf = void = bad = None
    want = np.zeros((21, 21), np.int64)
    want_void = np.zeros(21, np.int64)
    for _ in range(3):
        gt = _gt(h, w, rng)
        pred = rng.randint(0, 21, (h, w)).astype(np.uint8)
        pred[rng.rand(h, w) < 0.2] = 255
        conf, void, bad = ops.label_confusion(torch.from_numpy(pred).to(_dev()), torch.from_numpy(gt).to(_dev()), conf, bad,
                                              void=void)
        p = np.where(pred == 255, 0, pred).astype(np.int64)
        m = gt != 255
        np.add.at(want, (gt[m].astype(np.int64), p[m]), 1)
        np.add.at(want_void, p[~m], 1)
    assert int(bad.item()) == 0
    assert np.array_equal(conf.cpu().numpy(), want) and np.array_equal(void.cpu().numpy(), want_void)
    gt = np.full((h, w), 21, np.uint8)
    _, _, bad = ops.label_confusion(torch.from_numpy(gt.copy()).to(_dev()), torch.from_numpy(gt).to(_dev()))
    assert int(bad.item()) == h * w


@pytest.mark.parametrize("n,g", [(0, 0), (0, 3), (4, 0), (5, 3), (40, 12)])
def test_mask_overlap_exact(n, g):
    from irn_amd import ops
    rng = np.random.RandomState(n * 13 + g)
    h, w = 375, 500
    inst = rng.randint(0, g + 1, (h, w)).astype(np.uint8)
    masks = rng.rand(n, h, w) < 0.3
    inter, ap, ag = ops.mask_overlap(torch.from_numpy(masks).to(_dev()), torch.from_numpy(inst).to(_dev()), g)
    gm = np.stack([inst == i + 1 for i in range(g)]) if g else np.zeros((0, h, w), bool)
    assert np.array_equal(inter.cpu().numpy(), (masks[:, None] & gm[None]).sum(axis=(2, 3)).reshape(n, g))
    assert np.array_equal(ap.cpu().numpy(), masks.sum(axis=(1, 2)))
    assert np.array_equal(ag.cpu().numpy(), gm.sum(axis=(1, 2)))
    bad = torch.zeros(1, dtype=torch.int64, device=_dev())
    inst[0, :3] = g + 1
    ops.mask_overlap(torch.from_numpy(masks).to(_dev()), torch.from_numpy(inst).to(_dev()), g, bad)
    assert int(bad.item()) == 3


# ---------------------------------------------------------------------------------------------------------------------
# end to end through run_sample.py
# ---------------------------------------------------------------------------------------------------------------------
def _make_voc(tmp, n=8):
    root = tmp / "voc"
    for d in ("JPEGImages", "SegmentationClass", "SegmentationObject", "ImageSets/Segmentation"):
        (root / d).mkdir(parents=True)
    rng = np.random.RandomState(0)
    names, labels = [], {}
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        h, w = ((96, 128), (113, 150))[i % 2]
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8)
        Image.fromarray(img).resize((w, h), Image.BICUBIC).save(root / "JPEGImages" / (name + ".jpg"), quality=95)
        classes = rng.choice(20, rng.randint(1, 4), replace=False)
        lab = np.zeros(20, np.float32)
        lab[classes] = 1
        labels[int(name.replace("_", ""))] = lab
        cls = np.zeros((h, w), np.uint8)
        obj = np.zeros((h, w), np.uint8)
        for j in range(rng.randint(1, 5)):
            y0, x0 = rng.randint(0, h - 20), rng.randint(0, w - 20)
            y1, x1 = y0 + rng.randint(10, h // 2), x0 + rng.randint(10, w // 2)
            c = classes[j % len(classes)]
            cls[y0:y1, x0:x1] = 255
            obj[y0:y1, x0:x1] = 255
            cls[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = c + 1
            obj[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = 3 * j + 2
        R.save_p_png(root / "SegmentationClass" / (name + ".png"), cls)
        R.save_p_png(root / "SegmentationObject" / (name + ".png"), obj)
        names.append(name)
    (root / "ImageSets" / "Segmentation" / "train.txt").write_text("\n".join(names) + "\n")
    (tmp / "lists").mkdir()
    (tmp / "lists" / "train.txt").write_text("\n".join(names) + "\n")
    np.save(tmp / "lists" / "cls_labels.npy", labels)
    return root, names


SWEEP = ["0.05", "0.1", "0.15", "0.2", "0.3", "0.45", "0.6"]


def _run(tmp_path, root, tag, extra):
    lst = str(tmp_path / "lists" / "train.txt")
    return S.run_sample_main(["--voc12_root", str(root), "--train_list", lst, "--infer_list", lst, "--num_workers", "2",
                              "--cam_weights_name", str(tmp_path / "res50_cam"),
                              "--irn_weights_name", str(tmp_path / "res50_irn.pth"),
                              "--cam_out_dir", str(tmp_path / tag / "cam"), "--sem_seg_out_dir", str(tmp_path / tag / "sem"),
                              "--ins_seg_out_dir", str(tmp_path / tag / "ins"), "--log_name", str(tmp_path / tag),
                              "--cam_scales", "1.0", "0.5", "--eval_cam_pass", "True", "--eval_ins_seg_pass", "True",
                              "--eval_sem_seg_pass", "True", "--cam_eval_thres_sweep"] + SWEEP + extra)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        else:
            np.testing.assert_array_equal(a[k], b[k])


def test_run_sample_eval_passes_vs_restatement(tmp_path):
    from irn_amd.net import weights
    root, names = _make_voc(tmp_path)
    torch.save(weights.random_cam_state(1), tmp_path / "res50_cam.pth")
    torch.save(weights.random_irn_state(2), tmp_path / "res50_irn.pth")
    got = _run(tmp_path, root, "one", [])
    assert set(got) == {"eval_cam", "eval_ins_seg", "eval_sem_seg"}
    cam_dir, sem_dir, ins_dir = (str(tmp_path / "one" / d) for d in ("cam", "sem", "ins"))
    want = R.eval_cam(str(root), "train", cam_dir, 0.15)
    np.testing.assert_array_equal(got["eval_cam"]["iou"], want["iou"])
    assert got["eval_cam"]["miou"] == want["miou"]
    for t in SWEEP:
        assert got["eval_cam"]["sweep"][float(t)] == R.eval_cam(str(root), "train", cam_dir, float(t))["miou"], t
    best = got["eval_cam"]["best_thres"]
    assert got["eval_cam"]["sweep"][best] == max(got["eval_cam"]["sweep"].values())
    want, _, _ = R.eval_sem_seg(str(root), "train", sem_dir)
    np.testing.assert_array_equal(got["eval_sem_seg"]["iou"], want["iou"])
    assert got["eval_sem_seg"]["miou"] == want["miou"]
    want = R.eval_ins_seg(str(root), "train", ins_dir)
    np.testing.assert_array_equal(got["eval_ins_seg"]["ap"], want["ap"])
    np.testing.assert_array_equal(got["eval_ins_seg"]["map"], want["map"])
    # another worker layout for the label steps: the same files, the same scores
    again = _run(tmp_path, root, "two", ["--worker_devices", "0,0"])
    _same(got, again)


def test_eval_step_names_a_missing_file(tmp_path):
    import argparse
    from irn_amd.step import eval_sem_seg
    root, names = _make_voc(tmp_path, n=2)
    sem = tmp_path / "sem"
    sem.mkdir()
    Image.fromarray(np.zeros((96, 128), np.uint8)).save(sem / (names[0] + ".png"))
    args = argparse.Namespace(voc12_root=str(root), chainer_eval_set="train", sem_seg_out_dir=str(sem), num_workers=2)
    with pytest.raises(FileNotFoundError, match=names[1]):
        eval_sem_seg.run(args)
    Image.fromarray(np.zeros((10, 10), np.uint8)).save(sem / (names[1] + ".png"))
    with pytest.raises(ValueError, match=names[1]):
        eval_sem_seg.run(args)
