"""`--num_classes 80` through the steps, on a small synthetic VOC-layout tree (4 images of 96 x 128 and 113 x 150, 80 classes,
every image with a class key >= 20 and one with key 79, SegmentationObject included, random 80-class CAM and IRNet weights).
make_cam runs once for the module; every test then runs at most three steps through run_sample.main and compares what they
print or write with a numpy restatement of the reference's scoring at 81 classes, exactly.  Not vacuous: labels >= 21 must
occur in the written maps and detections.  The last test is one training step of run_train.py on a tree whose only classes
are >= 21: without the class count the loss ignores every such label and counts no foreground or unequal pair."""
import json
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

C = 80
KEYS = ([20, 45, 79], [3, 33], [25, 60, 70], [7, 21])          # every image has a key >= 20; the first has 79


def _make_voc(tmp):
    """JPEGs and ground truth (class and object maps) of four images from Gaussian blobs, a void band where they fade."""
    from irn_amd import synth
    rng = np.random.RandomState(0)
    specs = []
    for i, keys in enumerate(KEYS):
        h, w = ((96, 128), (113, 150))[i % 2]
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8)
        keys = np.asarray(keys, np.int64)
        cam = synth.cam_blobs(len(keys), *synth.grid_of((h, w)), seed=40 + i)
        gt, obj = synth.blob_ground_truth(synth.upsample4(cam, (h, w)), keys, 0.45, 0.35, obj_ids=np.arange(len(keys)) + 1)
        specs.append({"name": "2008_%06d" % (i + 1), "photo": np.asarray(Image.fromarray(img).resize((w, h), Image.BICUBIC)),
                      "quality": 95, "keys": keys, "cls": gt, "obj": obj})
    return tmp / "voc", synth.write_voc_tree(tmp / "voc", specs, tmp / "lists" / "train.txt", cls_labels=C)


def _run(tree, passes, extra=()):
    """run_sample.main with exactly the passes named."""
    tmp, lst = tree["tmp"], str(tree["tmp"] / "lists" / "train.txt")
    argv = ["--voc12_root", str(tree["root"]), "--train_list", lst, "--infer_list", lst, "--num_workers", "2",
            "--worker_devices", "0", "--num_classes", str(C), "--cam_scales", "1.0", "0.5",
            "--cam_weights_name", str(tmp / "res50_cam"), "--irn_weights_name", str(tmp / "res50_irn.pth"),
            "--cam_out_dir", str(tmp / "cam"), "--ir_label_out_dir", str(tmp / "ir_label"), "--sem_seg_out_dir", str(tmp / "sem"),
            "--ins_seg_out_dir", str(tmp / "ins"), "--cocoann_out", str(tmp / "coco.json"), "--log_name", str(tmp / "log")]
    for name in ("make_cam", "make_ins_seg", "make_sem_seg"):                  # the passes that default to True
        argv += ["--%s_pass" % name, str(name in passes)]
    for name in passes:
        if name not in ("make_cam", "make_ins_seg", "make_sem_seg"):
            argv += ["--%s_pass" % name, "True"]
    return S.run_sample_main(argv + list(extra))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from irn_amd.net import weights
    tmp = tmp_path_factory.mktemp("c80")
    root, names = _make_voc(tmp)
    torch.save(weights.random_cam_state(1, n_classes=C), tmp / "res50_cam.pth")
    torch.save(weights.random_irn_state(2), tmp / "res50_irn.pth")
    t = {"tmp": tmp, "root": root, "names": names}
    _run(t, ["make_cam"])
    return t


def _gt(tree, name):
    return np.asarray(Image.open(tree["root"] / "SegmentationClass" / (name + ".png")))


def _iou81(preds, gts):
    """step/eval_sem_seg.py:10-31 with its 21 read as 81."""
    conf = R.calc_semantic_segmentation_confusion(preds, gts)[:C + 1, :C + 1]
    gtj, resj, diag = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return diag / (gtj + resj - diag)


def test_make_cam_writes_the_keys_of_the_image_label(tree):
    for name, keys in zip(tree["names"], KEYS):
        d = np.load(tree["tmp"] / "cam" / (name + ".npy"), allow_pickle=True).item()
        assert np.asarray(d["keys"]).tolist() == keys
        assert d["high_res"].shape == (len(keys),) + _gt(tree, name).shape and np.isfinite(d["high_res"]).all()


def test_ir_labels_and_their_tuning_histogram(tree):
    res = _run(tree, ["cam_to_ir_label", "tune_ir_label"])["tune_ir_label"]
    want = np.zeros((C + 2, C + 2), np.int64)
    seen = set()
    for name, keys in zip(tree["names"], KEYS):
        lab = np.asarray(Image.open(tree["tmp"] / "ir_label" / (name + ".png")))
        gt = _gt(tree, name)
        assert lab.shape == gt.shape and set(np.unique(lab).tolist()) <= {0, 255} | {k + 1 for k in keys}
        seen |= set(np.unique(lab).tolist())
        row = np.where(gt == 255, C + 1, gt.astype(np.int64))
        col = np.where(lab == 255, C + 1, lab.astype(np.int64))
        np.add.at(want, (row.reshape(-1), col.reshape(-1)), 1)
    assert any(21 <= v <= C for v in seen), seen
    hist = np.asarray(res["hist"])
    assert hist.shape == (1, 1, C + 2, C + 2)
    assert np.array_equal(hist[0, 0], want)


def test_sem_seg_labels_scores_and_tuning(tree):
    res = _run(tree, ["make_sem_seg", "eval_sem_seg", "tune_sem_seg"])
    preds, gts, seen = [], [], set()
    for name in tree["names"]:
        p = np.asarray(Image.open(tree["tmp"] / "sem" / (name + ".png"))).astype(np.uint8).copy()
        seen |= set(np.unique(p).tolist())
        p[p == 255] = 0
        preds.append(p)
        gts.append(R.read_label(str(tree["root"]), name))
    assert any(21 <= v <= C for v in seen), seen
    want = _iou81(preds, gts)
    assert np.array_equal(res["eval_sem_seg"]["iou"], want, equal_nan=True)
    assert np.array_equal(res["tune_sem_seg"]["iou"], want, equal_nan=True)
    assert res["tune_sem_seg"]["miou"] == res["eval_sem_seg"]["miou"] == R.nanmean(want)


def test_ins_seg_labels_scores_and_coco_export(tree):
    res = _run(tree, ["make_ins_seg", "eval_ins_seg", "make_cocoann"])
    want = R.eval_ins_seg(str(tree["root"]), "train", str(tree["tmp"] / "ins"))
    assert np.array_equal(res["eval_ins_seg"]["ap"], want["ap"], equal_nan=True)
    classes = set()
    for name in tree["names"]:
        classes |= set(np.load(tree["tmp"] / "ins" / (name + ".npy"), allow_pickle=True).item()["class"].tolist())
    assert any(c >= 20 for c in classes), classes
    coco = json.load(open(tree["tmp"] / "coco.json"))
    assert [c["id"] for c in coco["categories"]] == list(range(1, C + 1))
    assert [c["name"] for c in coco["categories"]] == ["class_%d" % i for i in range(1, C + 1)]
    ids = {a["category_id"] for a in coco["annotations"]}
    assert ids and ids <= {c + 1 for c in classes} and 80 in ids, ids


def test_train_irn_counts_pairs_of_classes_above_twenty(tmp_path):
    """One step (crop 96, batch 2, two images) on IR labels from {0, 30, 80, 255}: foreground and unequal pairs are counted."""
    import run_train
    root = str(tmp_path)
    rng = np.random.RandomState(3)
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "ir_label"))
    names = []
    for i in range(2):
        name = "2007_%06d" % (i + 1)
        names.append(name)
        img = rng.randint(0, 255, (16, 19, 3)).repeat(8, 0).repeat(8, 1)[:120, :140]
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=92)
        lab = rng.choice(np.asarray([0, 30, 80, 255], np.uint8), (8, 9)).repeat(16, 0).repeat(16, 1)[:120, :140]
        Image.fromarray(lab).save(os.path.join(root, "ir_label", name + ".png"))
    lst = os.path.join(root, "train.txt")
    with open(lst, "w") as f:
        f.write("\n".join(names) + "\n")
    argv = ["--voc12_root", root, "--train_list", lst, "--infer_list", lst, "--ir_label_out_dir", os.path.join(root, "ir_label"),
            "--irn_crop_size", "96", "--irn_batch_size", "2", "--irn_num_epoches", "1", "--num_workers", "2",
            "--irn_weights_name", os.path.join(root, "sess", "res50_irn.pth"), "--log_name", os.path.join(root, "log"),
            "--train_irn_pass", "True", "--seed", "4", "--num_classes", str(C)]
    stdout = sys.stdout
    try:
        res = run_train.main(argv)["train_irn"]
    finally:
        sys.stdout = stdout
    print("\nfirst-step pair counts (bg, fg, neg):", res["first_counts"])
    assert res["steps"] == 1 and np.isfinite(res["first_losses"]).all()
    bg, fg, neg = res["first_counts"]
    assert fg > 0 and neg > 0 and bg > 0
