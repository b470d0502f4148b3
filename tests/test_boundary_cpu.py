"""Boundary IoU / Boundary AP without a GPU: the plain-loop restatement (tests/_boundary_ref.py) against scipy's erosion (the
published definition), the host scores, the argument checks of the three C entries and of their wrappers, the flag, and
that the two evaluation steps touch none of it while the flag is 0."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _boundary_ref as B  # noqa: E402


def _blobs(h, w, labels, seed, cell=5):
    rng = np.random.RandomState(seed)
    low = rng.choice(np.asarray(labels, np.uint8), ((h - 1) // cell + 1, (w - 1) // cell + 1))
    return np.ascontiguousarray(np.repeat(np.repeat(low, cell, axis=0), cell, axis=1)[:h, :w])


@pytest.mark.parametrize("n_labels", [2, 3, 4, 5])
def test_restatement_equals_the_published_erosion(n_labels):
    ndi = pytest.importorskip("scipy.ndimage", reason="scipy is not installed: nothing to compare the restatement with")
    labels = [0, 3, 20, 254, 255][:n_labels]
    for seed, (h, w) in enumerate([(23, 31), (40, 17)]):
        L = _blobs(h, w, labels, 10 * n_labels + seed, cell=4 + seed * 3)
        for d in (1, 2, 3, 6):
            got = B.band(L, d)
            for c in labels:
                m = L == c
                want = m & ~ndi.binary_erosion(m, structure=np.ones((3, 3)), iterations=d, border_value=0)
                assert np.array_equal(got.astype(bool) & m, want), (n_labels, seed, d, c)
            assert np.array_equal(B.mask_band(L == labels[1], d),
                                  (L == labels[1]) & ~ndi.binary_erosion(L == labels[1], structure=np.ones((3, 3)), iterations=d,
                                                                         border_value=0))


def test_band_of_the_restatement_is_the_per_pixel_definition():
    L = _blobs(13, 17, [0, 3, 254, 255], 3, cell=4)
    for d in (1, 2, 5):
        want = np.array([[B.band_at(L, d, y, x) for x in range(L.shape[1])] for y in range(L.shape[0])], np.uint8)
        assert np.array_equal(B.band(L, d), want), d


def test_boundary_distance():
    from irn_amd import ops
    for fn in (ops.boundary_distance, B.boundary_distance):
        assert fn(375, 500, 0.02) == 12                   # 12.5: ties to even
        assert fn(512, 512, 0.02) == 14
        assert fn(10, 10, 0.02) == 1
    for h, w, r in [(333, 500, 0.02), (96, 128, 0.02), (113, 150, 0.02), (500, 375, 0.05), (7, 5, 0.5)]:
        assert ops.boundary_distance(h, w, r) == B.boundary_distance(h, w, r)


def test_boundary_iou_scores():
    from irn_amd.misc import evaluation
    counts = np.array([[50, 100, 150], [0, 10, 0], [0, 0, 0], [7, 7, 7]], np.int64)
    s = evaluation.boundary_iou_scores(counts)
    assert set(s) == {"biou", "mbiou"}
    assert s["biou"][0] == 50 / 200 and s["biou"][1] == 0.0 and np.isnan(s["biou"][2]) and s["biou"][3] == 1.0
    assert s["mbiou"] == np.mean([0.25, 0.0, 1.0])
    assert np.isnan(evaluation.boundary_iou_scores(np.zeros((3, 3), np.int64))["mbiou"])


def test_instance_ap_boundary_matches_on_the_minimum():
    from irn_amd.misc import evaluation
    # one detection of class 2 against its only GT: mask IoU 60 / (80 + 80 - 60) = 0.6, band IoU 9 / (20 + 19 - 9) = 0.3
    rec = {"pred_class": np.array([2]), "pred_score": np.array([0.9]), "gt_class": np.array([2]),
           "inter": np.array([[60]]), "area_pred": np.array([80]), "area_gt": np.array([80]),
           "inter_b": np.array([[9]]), "band_pred": np.array([20]), "band_gt": np.array([19])}
    plain = evaluation.instance_ap_voc([rec], iou_thresh=0.5)
    assert plain["ap"][2] == 1.0 and plain["map"] == 1.0
    same = evaluation.instance_ap_voc([rec], iou_thresh=0.5, boundary=False)
    np.testing.assert_array_equal(plain["ap"], same["ap"])
    without = {k: v for k, v in rec.items() if k not in ("inter_b", "band_pred", "band_gt")}
    np.testing.assert_array_equal(evaluation.instance_ap_voc([without], iou_thresh=0.5)["ap"], plain["ap"])
    b = evaluation.instance_ap_voc([rec], iou_thresh=0.5, boundary=True)
    assert b["ap"][2] == 0.0 and b["map"] == 0.0          # a false positive, and the GT is missed
    # a band IoU above the mask IoU changes nothing
    rec2 = dict(rec, inter_b=np.array([[19]]), band_pred=np.array([20]), band_gt=np.array([19]))
    assert evaluation.instance_ap_voc([rec2], iou_thresh=0.5, boundary=True)["ap"][2] == 1.0


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    from irn_amd._lib import lib
    p = C.c_void_p(64)                                    # never dereferenced on these paths
    for d in (0, 65, -1):
        assert lib.irn_label_band(p, 4, 4, d, p, None) == 1 and b"irn_label_band: d" in lib.irn_last_error()
        assert lib.irn_label_boundary_counts(p, p, 4, 4, d, 0, 21, p, p, None) == 1 and b"d %d" % d in lib.irn_last_error()
        assert lib.irn_mask_boundary_overlap(p, 1, p, p, 1, 4, 4, d, p, p, p, p, None) == 1
        assert b"irn_mask_boundary_overlap: d" in lib.irn_last_error()
    assert lib.irn_label_band(None, 4, 4, 1, p, None) == 1
    assert lib.irn_label_band(p, 4, 4, 1, None, None) == 1
    assert lib.irn_label_band(p, 0, 4, 1, p, None) == 1
    assert lib.irn_label_band(p, 4, -3, 1, p, None) == 1 and b"irn_label_band" in lib.irn_last_error()
    for nc in (1, 82, 0):
        assert lib.irn_label_boundary_counts(p, p, 4, 4, 1, 0, nc, p, p, None) == 1 and b"n_classes" in lib.irn_last_error()
    assert lib.irn_label_boundary_counts(None, p, 4, 4, 1, 0, 21, p, p, None) == 1
    assert lib.irn_label_boundary_counts(p, None, 4, 4, 1, 0, 21, p, p, None) == 1
    assert lib.irn_label_boundary_counts(p, p, 4, 4, 1, 0, 21, None, p, None) == 1
    assert lib.irn_label_boundary_counts(p, p, 4, 4, 1, 0, 21, p, None, None) == 1
    assert lib.irn_label_boundary_counts(p, p, 4, 0, 1, 0, 21, p, p, None) == 1
    assert lib.irn_label_boundary_counts(p, p, 4, 4, 1, 21, 21, p, p, None) == 1
    assert b"irn_label_boundary_counts" in lib.irn_last_error()
    assert lib.irn_mask_boundary_overlap(p, -1, p, p, 1, 4, 4, 1, p, p, p, p, None) == 1
    assert lib.irn_mask_boundary_overlap(p, 1, p, p, 256, 4, 4, 1, p, p, p, p, None) == 1
    assert lib.irn_mask_boundary_overlap(None, 2, p, p, 1, 4, 4, 1, p, p, p, p, None) == 1
    assert lib.irn_mask_boundary_overlap(p, 1, None, p, 1, 4, 4, 1, p, p, p, p, None) == 1
    assert lib.irn_mask_boundary_overlap(p, 1, p, None, 1, 4, 4, 1, p, p, p, p, None) == 1
    assert lib.irn_mask_boundary_overlap(p, 1, p, p, 1, 4, 4, 1, None, p, p, p, None) == 1
    assert lib.irn_mask_boundary_overlap(p, 1, p, p, 1, 4, 4, 1, p, p, p, None, None) == 1
    assert lib.irn_mask_boundary_overlap(p, 1, p, p, 1, 0, 4, 1, p, p, p, p, None) == 1
    assert b"irn_mask_boundary_overlap" in lib.irn_last_error()


def test_ops_refuse_cpu_tensors():
    from irn_amd import ops
    m = torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.label_band(m, 1)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.label_boundary_counts(m, m, 1)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.mask_boundary_overlap(torch.zeros(1, 4, 4, dtype=torch.uint8), m, 1, 1)


def test_flag_parses_and_is_off_by_default():
    import run_sample
    p = run_sample.build_parser()
    assert p.parse_args(["--voc12_root", "x"]).boundary_iou_ratio == 0
    assert p.parse_args(["--voc12_root", "x", "--boundary_iou_ratio", "0.02"]).boundary_iou_ratio == 0.02
    for bad in ("-0.1", "nan", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["--voc12_root", "x", "--boundary_iou_ratio", bad])
    p.format_help()
    from irn_amd.step import _eval
    import argparse
    assert _eval.boundary_ratio(argparse.Namespace()) == 0          # a caller's own namespace without the flag: off
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="boundary_iou_ratio"):
            _eval.boundary_ratio(argparse.Namespace(boundary_iou_ratio=bad))
    with pytest.raises(ValueError, match=r"2008_000001: --boundary_iou_ratio 0.2 .* 125 pixels"):
        _eval.boundary_d("2008_000001", (375, 500), 0.2)
    assert _eval.boundary_d("x", (375, 500), 0.02) == 12


def _raiser(name):
    def f(*a, **k):
        raise AssertionError("ops.%s was called with --boundary_iou_ratio 0" % name)
    return f


def test_steps_do_not_touch_the_new_ops_with_the_flag_at_0(tmp_path, monkeypatch, capsys):
    """Both steps on a two-image tree with the device calls they make today replaced by numpy on CPU tensors and the new ops
    replaced by functions that raise: they run through, print what they printed and return the keys they returned."""
    import run_sample
    from PIL import Image
    from irn_amd import ops
    from irn_amd.step import _eval, eval_ins_seg, eval_sem_seg
    root, sem, ins = tmp_path / "voc", tmp_path / "sem", tmp_path / "ins"
    for d in (root / "SegmentationClass", root / "SegmentationObject", root / "ImageSets" / "Segmentation", sem, ins):
        d.mkdir(parents=True)
    names = ["2008_000001", "2008_000002"]
    (root / "ImageSets" / "Segmentation" / "train.txt").write_text("\n".join(names) + "\n")
    for i, name in enumerate(names):
        cls = np.zeros((12, 16), np.uint8)
        cls[2:8, 3:9 + i] = 5
        obj = (cls > 0).astype(np.uint8)
        for arr, d in ((cls, root / "SegmentationClass"), (obj, root / "SegmentationObject"), (np.roll(cls, 1, axis=1), sem)):
            Image.fromarray(arr, mode="L").save(d / (name + ".png"))
        np.save(ins / (name + ".npy"), {"score": np.array([0.5]), "mask": np.roll(obj, 1, axis=0)[None] > 0, "class": np.array([4])})

    def label_confusion(pred, gt, conf, bad, pred_255_as=0, void=None, n_classes=21):
        conf = torch.zeros(n_classes, n_classes, dtype=torch.int64) if conf is None else conf
        void = torch.zeros(n_classes, dtype=torch.int64) if void is None else void
        bad = torch.zeros(1, dtype=torch.int64) if bad is None else bad
        for g, p in zip(gt.reshape(-1).tolist(), pred.reshape(-1).tolist()):
            conf[g, p] += 1
        return conf, void, bad

    def mask_overlap(masks, inst_map, g, bad):
        m = masks.numpy().astype(bool)
        inst = inst_map.numpy()
        inter = np.array([[(mk & (inst == j + 1)).sum() for j in range(g)] for mk in m], np.int64).reshape(len(m), g)
        return (torch.from_numpy(inter), torch.from_numpy(m.reshape(len(m), -1).sum(1).astype(np.int64)),
                torch.from_numpy(np.array([(inst == j + 1).sum() for j in range(g)], np.int64)))

    monkeypatch.setattr(_eval, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(ops, "label_confusion", label_confusion)
    monkeypatch.setattr(ops, "mask_overlap", mask_overlap)
    for name in ("label_band", "label_boundary_counts", "mask_boundary_overlap", "boundary_distance"):
        monkeypatch.setattr(ops, name, _raiser(name))
    args = run_sample.build_parser().parse_args(["--voc12_root", str(root), "--sem_seg_out_dir", str(sem), "--ins_seg_out_dir", str(ins),
                                                 "--num_workers", "0"])
    assert args.boundary_iou_ratio == 0
    out = eval_sem_seg.run(args)
    assert set(out) == {"iou", "miou"}
    text = capsys.readouterr().out
    assert "biou" not in text and text.endswith(str(out) + "\n") and len(text[:-len(str(out)) - 1].splitlines()) == 2
    out = eval_ins_seg.run(args)
    assert set(out) == {"ap", "map"}
    assert capsys.readouterr().out == "0.5iou: %s\n" % out
    # and with the flag set the steps do reach for them
    args.boundary_iou_ratio = 0.02
    with pytest.raises(AssertionError, match="boundary_distance"):
        eval_sem_seg.run(args)
    with pytest.raises(AssertionError, match="boundary_distance"):
        eval_ins_seg.run(args)
