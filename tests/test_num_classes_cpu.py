"""`--num_classes` / `--class_names` without a GPU: the three parsers, the size-generic score functions at 81 classes, the
CAM classifier's width and the refusal of a checkpoint of another width, the cls_labels.npy row check, the
make_cls_labels tool on a three-image XML tree, and the argument checks of the new C entries."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------------
# command lines
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", ["run_sample", "run_train", "run_train_cam"])
def test_parsers_take_one_to_eighty_classes(module, capsys):
    import importlib
    p = importlib.import_module(module).build_parser()
    base = ["--voc12_root", "x"]
    a = p.parse_args(base)
    assert a.num_classes == 20 and a.class_names is None
    assert p.parse_args(base + ["--num_classes", "1"]).num_classes == 1
    assert p.parse_args(base + ["--num_classes", "80", "--class_names", "names.txt"]).class_names == "names.txt"
    for bad in ("0", "81", "-3", "many"):
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--num_classes", bad])
        assert "--num_classes" in capsys.readouterr().err


def test_class_names_default_and_file(tmp_path):
    from irn_amd.step import _classes, make_cocoann
    assert _classes.num_classes(argparse.Namespace()) == 20                      # an args object of an older caller
    assert _classes.class_names(argparse.Namespace(num_classes=20)) == list(make_cocoann.CATEGORIES)
    assert _classes.class_names(argparse.Namespace(num_classes=3)) == ["class_1", "class_2", "class_3"]
    f = tmp_path / "names.txt"
    f.write_text("cat\n dog \n\nzebra\n")
    assert _classes.class_names(argparse.Namespace(num_classes=3, class_names=str(f))) == ["cat", "dog", "zebra"]
    with pytest.raises(ValueError, match=r"names\.txt: 3 class names for --num_classes 4"):
        _classes.class_names(argparse.Namespace(num_classes=4, class_names=str(f)))
    with pytest.raises(ValueError, match="outside 1..80"):
        _classes.num_classes(argparse.Namespace(num_classes=81))
    cats = make_cocoann.categories(["cat", "dog", "zebra"])
    assert [c["id"] for c in cats] == [1, 2, 3] and cats[2]["name"] == "zebra"
    assert make_cocoann.categories()[19] == {"supercategory": "none", "id": 20, "name": "tvmonitor"}


# ------------------------------------------------------------------------------------------------
# scores from 81-class matrices
# ------------------------------------------------------------------------------------------------
def _maps(seed, nc=81):
    rng = np.random.RandomState(seed)
    preds, gts = [], []
    for _ in range(3):
        gt = rng.randint(0, nc, (40, 50)).astype(np.int32)
        gt[rng.rand(40, 50) < 0.1] = -1
        pred = np.where(rng.rand(40, 50) < 0.6, np.maximum(gt, 0), rng.randint(0, nc, (40, 50))).astype(np.int32)
        gt[gt == 17] = 5                                  # a class that occurs in no ground truth
        preds.append(pred)
        gts.append(gt)
    return preds, gts


def test_sem_seg_scores_take_their_size_from_the_matrix():
    from irn_amd.misc import evaluation
    preds, gts = _maps(0)
    conf = R.calc_semantic_segmentation_confusion(preds, gts)
    assert conf.shape == (81, 81)
    void = np.zeros(81, np.int64)
    for p, g in zip(preds, gts):
        void += np.bincount(p[g < 0], minlength=81)
    s = evaluation.sem_seg_scores(conf, void)
    gtj, resj, diag = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(s["iou"], diag / (gtj + resj - diag), equal_nan=True)
        assert np.array_equal(s["fp"], 1. - gtj / (gtj + resj - diag), equal_nan=True)
    assert s["iou"].shape == (81,) and np.array_equal(s["iou"], R.iou_of(conf), equal_nan=True)
    assert np.isfinite(s["iou"][21:]).sum() > 50                                 # the classes above 20 are scored
    # a 21-class matrix keeps scoring as before
    preds, gts = _maps(1, 21)
    conf21 = R.calc_semantic_segmentation_confusion(preds, gts)
    assert np.array_equal(evaluation.sem_seg_scores(conf21)["iou"], R.iou_of(conf21), equal_nan=True)


def test_ir_label_scores_take_their_size_from_the_histogram():
    from irn_amd.misc import evaluation
    rng = np.random.RandomState(2)
    nc = 81
    hist = rng.randint(0, 50, (nc + 1, nc + 1)).astype(np.int64)
    hist[:, 30] = 0                                       # a label that is never given
    hist[44, :] = 0                                       # a class without ground truth
    s = evaluation.ir_label_scores(hist)
    conf = hist[:nc, :nc]
    diag = np.diag(conf)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = diag / (conf.sum(axis=1) + conf.sum(axis=0) - diag)
        iou_all = diag / (hist[:nc, :].sum(axis=1) + conf.sum(axis=0) - diag)
    assert np.array_equal(s["iou"], iou, equal_nan=True) and np.array_equal(s["iou_all"], iou_all, equal_nan=True)
    assert s["coverage"] == conf.sum() / hist[:nc, :].sum()
    assert s["miou"] == R.nanmean(iou) and s["miou_all"] == R.nanmean(iou_all)


# ------------------------------------------------------------------------------------------------
# networks and data
# ------------------------------------------------------------------------------------------------
def test_classifier_width_and_refusal_of_another_width(tmp_path):
    from irn_amd.net import resnet50_cam, weights
    from irn_amd.step import _pool
    with torch.device("meta"):
        assert resnet50_cam.Net().classifier.weight.shape == (20, 2048, 1, 1)
        assert resnet50_cam.CAM(n_classes=80).classifier.weight.shape == (80, 2048, 1, 1)
        assert resnet50_cam.Net(n_classes=1).classifier.weight.shape[0] == 1
        with pytest.raises(ValueError, match="n_classes"):
            resnet50_cam.Net(n_classes=81)
    s20, s80 = weights.random_cam_state(1), weights.random_cam_state(1, n_classes=80)
    assert s20["classifier.weight"].shape[0] == 20 and s80["classifier.weight"].shape[0] == 80
    assert set(s20) == set(s80)
    assert torch.equal(s20["classifier.weight"], weights.random_cam_state(1, n_classes=20)["classifier.weight"])
    torch.save(s20, tmp_path / "cam20.pth")
    torch.save(s80, tmp_path / "cam80.pth")
    for strict in (True, False):
        with pytest.raises(ValueError, match="20 classes.* 80 "):
            _pool.ModelSpec("net.resnet50_cam", "CAM", str(tmp_path / "cam20.pth"), strict=strict, n_classes=80).build()
    with pytest.raises(ValueError, match="80 classes.* 20 "):
        _pool.ModelSpec("net.resnet50_cam", "CAM", str(tmp_path / "cam80.pth"), strict=True).build()
    net = _pool.ModelSpec("net.resnet50_cam", "CAM", str(tmp_path / "cam80.pth"), strict=True, n_classes=80).build()
    assert torch.equal(net.classifier.weight, s80["classifier.weight"])
    a = _pool.ModelSpec("net.resnet50_cam", "CAM", str(tmp_path / "cam80.pth"), strict=True, n_classes=80).key()
    b = _pool.ModelSpec("net.resnet50_cam", "CAM", str(tmp_path / "cam80.pth"), strict=True).key()
    assert a != b and a[:3] == b[:3]


def test_cls_labels_of_another_width_are_refused_by_name(tmp_path):
    from PIL import Image
    from irn_amd.voc12 import dataloader
    (tmp_path / "JPEGImages").mkdir()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "JPEGImages" / "2008_000001.jpg")
    (tmp_path / "train.txt").write_text("2008_000001\n")
    np.save(tmp_path / "cls_labels.npy", {2008000001: np.ones(20, np.float32)})
    lst = str(tmp_path / "train.txt")
    for cls in (dataloader.VOC12ClassificationDatasetMSF, dataloader.VOC12ClassificationDataset):
        assert cls(lst, voc12_root=str(tmp_path), n_classes=20).label_list.shape == (1, 20)
        assert cls(lst, voc12_root=str(tmp_path)).label_list.shape == (1, 20)
        with pytest.raises(ValueError, match=r"cls_labels\.npy.*2008_000001.*20 entries.*80"):
            cls(lst, voc12_root=str(tmp_path), n_classes=80)


def test_instance_label_takes_the_class_count(tmp_path):
    from irn_amd.voc12 import eval_data
    for d in ("SegmentationClass", "SegmentationObject"):
        (tmp_path / d).mkdir()
    cls = np.zeros((6, 7), np.uint8)
    cls[:3] = 80
    obj = (cls > 0).astype(np.uint8)
    R.save_p_png(tmp_path / "SegmentationClass" / "a.png", cls)
    R.save_p_png(tmp_path / "SegmentationObject" / "a.png", obj)
    with pytest.raises(ValueError, match="class 79"):
        eval_data.instance_label(str(tmp_path), "a")
    inst_map, inst_class = eval_data.instance_label(str(tmp_path), "a", n_fg=80)
    assert inst_class.tolist() == [79] and np.array_equal(inst_map, obj)


# ------------------------------------------------------------------------------------------------
# make_cls_labels
# ------------------------------------------------------------------------------------------------
def _xml(objects):
    return "<annotation><filename>x.jpg</filename>%s</annotation>" % "".join(
        "<object><name>%s</name><bndbox><xmin>1</xmin></bndbox></object>" % o for o in objects)


def test_make_cls_labels_on_a_three_image_tree(tmp_path):
    from irn_amd.voc12 import make_cls_labels
    ann = tmp_path / "Annotations"
    ann.mkdir()
    (ann / "2008_000001.xml").write_text(_xml(["zebra", "cat", "zebra"]))
    (ann / "2008_000002.xml").write_text(_xml([]))
    (ann / "2008_000003.xml").write_text(_xml(["dog"]))
    names = tmp_path / "names.txt"
    names.write_text("cat\ndog\nzebra\n")
    out = tmp_path / "cls_labels.npy"
    make_cls_labels.main(["--voc12_root", str(tmp_path), "--class_names", str(names), "--out", str(out)])
    got = np.load(out, allow_pickle=True).item()
    assert sorted(got) == [2008000001, 2008000002, 2008000003]
    assert all(v.dtype == np.float32 and v.shape == (3,) for v in got.values())
    assert got[2008000001].tolist() == [1, 0, 1] and got[2008000002].tolist() == [0, 0, 0] and got[2008000003].tolist() == [0, 1, 0]
    lst = tmp_path / "list.txt"
    lst.write_text("2008_000003\n")
    make_cls_labels.main(["--voc12_root", str(tmp_path), "--class_names", str(names), "--out", str(out), "--img_list", str(lst)])
    assert sorted(np.load(out, allow_pickle=True).item()) == [2008000003]
    (ann / "2008_000004.xml").write_text(_xml(["cat", "unicorn"]))
    with pytest.raises(ValueError, match="2008_000004.*unicorn"):
        make_cls_labels.main(["--voc12_root", str(tmp_path), "--class_names", str(names), "--out", str(out)])
    lst.write_text("2008_000009\n")
    with pytest.raises(FileNotFoundError, match="2008_000009"):
        make_cls_labels.main(["--voc12_root", str(tmp_path), "--class_names", str(names), "--out", str(out), "--img_list", str(lst)])


# ------------------------------------------------------------------------------------------------
# C entries: bad class counts are refused before any device work
# ------------------------------------------------------------------------------------------------
def test_new_entries_refuse_bad_class_counts_without_a_gpu():
    from irn_amd import _lib
    L = _lib.lib
    one = C.c_void_p(64)                                  # never dereferenced on these paths
    idx = (C.c_int32 * 1)(0)
    i32 = (C.c_int32 * 1)(4)
    ptrs = (C.c_void_p * 1)(64)
    for nc in (1, 82, 0, -5):
        assert L.irn_cam_confusion(one, one, 1, one, 4, 4, one, 1, nc, one, one, None) == 1
        assert b"irn_cam_confusion" in L.irn_last_error() and b"n_classes" in L.irn_last_error()
        assert L.irn_cam_confusion_reduce(one, 1, nc, one, one, None) == 1
        assert b"irn_cam_confusion_reduce" in L.irn_last_error() and b"n_classes" in L.irn_last_error()
        assert L.irn_label_confusion(one, one, 4, 4, 0, nc, one, one, one, None) == 1
        assert b"irn_label_confusion" in L.irn_last_error() and b"n_classes" in L.irn_last_error()
        assert L.irn_ir_label_confusion(one, 1, idx, 1, idx, 1, one, 4, 4, nc, one, one, None) == 1
        assert b"irn_ir_label_confusion" in L.irn_last_error() and b"n_classes" in L.irn_last_error()
        assert L.irn_label_sweep_confusion(1, ptrs, i32, i32, i32, i32, i32, ptrs, ptrs, one, 1, nc, one, one, one, None) == 1
        assert b"irn_label_sweep_confusion" in L.irn_last_error() and b"n_classes" in L.irn_last_error()
    # channel counts above nc - 1, and a 255 mapped to a class that does not exist
    assert L.irn_cam_confusion(one, one, 2, one, 4, 4, one, 1, 2, one, one, None) == 1 and b"k=2" in L.irn_last_error()
    assert L.irn_cam_confusion(one, one, 81, one, 4, 4, one, 1, 81, one, one, None) == 1
    assert L.irn_label_confusion(one, one, 4, 4, 2, 2, one, one, one, None) == 1
    two = (C.c_int32 * 1)(2)
    assert L.irn_label_sweep_confusion(1, ptrs, two, i32, i32, i32, i32, ptrs, ptrs, one, 1, 2, one, one, one, None) == 1
    assert b"at most 1" in L.irn_last_error()
    # the loss: ignore_from is a byte value below 255's void
    for bad in (0, 256, -1):
        assert L.irn_aff_loss_forward(one, one, one, 1, 12, 21, 5, bad, one, one, one, 1 << 20, None) == 1
        assert b"ignore_from" in L.irn_last_error()
        assert L.irn_aff_loss_backward(one, one, one, 1, 12, 21, 5, bad, one, one, one, one, 1 << 20, None) == 1
        assert L.irn_aff_loss_backward_ordered(one, one, one, 1, 12, 21, 5, bad, one, one, one, one, 1 << 20, None) == 1
        assert b"irn_aff_loss_backward_ordered" in L.irn_last_error()
