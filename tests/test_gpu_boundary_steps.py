"""--boundary_iou_ratio through run_sample.py: eval_sem_seg's Boundary IoU and eval_ins_seg's Boundary AP on a small synthetic
VOC tree, against the plain-loop restatement (tests/_boundary_ref.py) applied to the same files; and, with the flag at 0,
the output and the returned keys the two steps had before the flag existed."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _boundary_ref as B  # noqa: E402
import _steps as S  # noqa: E402

pytestmark = pytest.mark.gpu

RATIO = 0.02
SIZES = ((96, 128), (113, 150), (70, 130))               # d = 3, 4 and 3 at ratio 0.02


def _rle_counts(mask):
    """COCO's uncompressed run lengths: column-major pixels, the first run counts zeros."""
    flat = np.asarray(mask, bool).T.reshape(-1)
    edges = np.flatnonzero(np.diff(flat.astype(np.int8))) + 1
    runs = np.diff(np.concatenate(([0], edges, [flat.size])))
    return np.concatenate(([0], runs)) if flat[0] else runs


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """GT of Gaussian-blob objects with VOC's void ring, label PNGs that miss it by a few pixels, and detections (dense and as
    run lengths) that are the objects shifted, one of them twice."""
    from irn_amd import synth
    tmp = tmp_path_factory.mktemp("boundary")
    root = tmp / "voc"
    sem, ins, rle = tmp / "sem", tmp / "ins", tmp / "rle"
    for d in (sem, ins, rle):
        d.mkdir()
    specs, files = [], []
    for i, (h, w) in enumerate(SIZES):
        name = "2008_%06d" % (i + 1)
        k = 2 + i % 2
        keys = synth.voc_keys(k, i)
        cam = synth.cam_blobs(k, h, w, seed=i)
        cls, obj = synth.blob_ground_truth(cam, keys, 0.5, 0.35, obj_ids=np.arange(1, k + 1))
        specs.append({"name": name, "photo": synth.photo(h, w, i), "quality": 90, "keys": keys, "cls": cls, "obj": obj})
        plain = np.where(cls == 255, 0, cls)
        pred = np.roll(plain, (2, -3), axis=(0, 1))
        pred[:2, :] = 255                                 # read as background by the step
        synth.save_palette_png(str(sem / (name + ".png")), pred)
        masks, classes, scores = [], [], []
        for j in range(k):
            m = obj == j + 1
            if not m.any():
                continue
            masks += [np.roll(m, (1, 2), axis=(0, 1)), np.roll(m, (4 + j, -5), axis=(0, 1))]
            classes += [int(keys[j])] * 2
            scores += [0.9 - 0.1 * j, 0.4 + 0.1 * j]
        det = {"score": np.asarray(scores, np.float32), "mask": np.stack(masks), "class": np.asarray(classes, np.int64)}
        np.save(ins / (name + ".npy"), det)
        counts = [_rle_counts(m) for m in masks]
        np.savez(rle / (name + ".rle.npz"), size=np.asarray([h, w]), counts=np.concatenate(counts).astype(np.uint32),
                 offsets=np.concatenate(([0], np.cumsum([len(c) for c in counts]))).astype(np.int64), score=det["score"],
                 **{"class": det["class"]})
        files.append((name, pred, det))
    lst = str(tmp / "lists" / "train.txt")
    synth.write_voc_tree(str(root), specs, lst, cls_labels=20)
    return {"tmp": tmp, "root": root, "list": lst, "sem": sem, "ins": ins, "rle": rle, "files": files}


def _run(tree, tag, ins_dir, ratio):
    t = tree["tmp"]
    got = S.run_sample_main(["--voc12_root", str(tree["root"]), "--train_list", tree["list"], "--infer_list", tree["list"],
                             "--num_workers", "2", "--cam_out_dir", str(t / tag / "cam"), "--sem_seg_out_dir", str(tree["sem"]),
                             "--ins_seg_out_dir", str(ins_dir), "--log_name", str(t / tag), "--make_cam_pass", "False",
                             "--make_ins_seg_pass", "False", "--make_sem_seg_pass", "False", "--eval_ins_seg_pass", "True",
                             "--eval_sem_seg_pass", "True"] + (["--boundary_iou_ratio", str(ratio)] if ratio is not None else []))
    with open(str(t / tag) + ".log") as f:
        lines = f.read().splitlines(keepends=True)
    # the steps' own output: not the argument dump of run_sample.main, not the timers' "step.<name>: <date>" lines
    return got, "".join(l for l in lines[1:] if not l.startswith("step."))


@pytest.fixture(scope="module")
def runs(tree):
    return {"off": _run(tree, "off", tree["ins"], None), "zero": _run(tree, "zero", tree["ins"], 0),
            "on": _run(tree, "on", tree["ins"], RATIO), "rle": _run(tree, "rle", tree["rle"], RATIO)}


def test_eval_sem_seg_biou_equals_the_restatement(tree, runs):
    from irn_amd.misc import evaluation
    from irn_amd.voc12 import eval_data
    got = runs["on"][0]["eval_sem_seg"]
    assert set(got) == {"iou", "miou", "biou", "mbiou"}
    counts = np.zeros((21, 3), np.int64)
    for name, pred, _ in tree["files"]:
        gt = eval_data.class_label(str(tree["root"]), name)
        on_disk = np.asarray(Image.open(tree["sem"] / (name + ".png")), np.uint8)
        assert np.array_equal(on_disk, pred)
        c, bad = B.semantic_counts(on_disk, gt, B.boundary_distance(gt.shape[0], gt.shape[1], RATIO), 21, 0)
        assert bad == 0
        counts += c
    with np.errstate(divide="ignore", invalid="ignore"):
        want = counts[:, 0] / (counts[:, 1] + counts[:, 2] - counts[:, 0])
    np.testing.assert_array_equal(got["biou"], want)
    assert got["mbiou"] == np.nanmean(want) and 0 < got["mbiou"] < 1
    assert np.isfinite(want).sum() >= 3                   # the background and at least two classes have a band
    off = runs["off"][0]["eval_sem_seg"]
    np.testing.assert_array_equal(got["iou"], off["iou"])
    assert got["miou"] == off["miou"]
    assert got["mbiou"] < got["miou"]                     # a shift of 2-3 pixels costs the band far more than the region
    assert evaluation.boundary_iou_scores(counts)["mbiou"] == got["mbiou"]


def test_eval_ins_seg_bap_equals_the_restatement(tree, runs):
    from irn_amd.misc import evaluation
    from irn_amd.voc12 import eval_data
    got = runs["on"][0]["eval_ins_seg"]
    assert set(got) == {"ap", "map", "bap", "bmap"}
    records = []
    for name, _, det in tree["files"]:
        inst, inst_class = eval_data.instance_label(str(tree["root"]), name)
        g = len(inst_class)
        d = B.boundary_distance(inst.shape[0], inst.shape[1], RATIO)
        inter_b, band_pred, band_gt, bad = B.instance_counts(det["mask"], inst, g, d)
        assert bad == 0
        m = det["mask"].astype(bool)
        records.append({"pred_class": det["class"], "pred_score": det["score"], "gt_class": inst_class,
                        "inter": np.array([[(mk & (inst == j + 1)).sum() for j in range(g)] for mk in m], np.int64).reshape(len(m), g),
                        "area_pred": m.reshape(len(m), -1).sum(1), "area_gt": np.array([(inst == j + 1).sum() for j in range(g)]),
                        "inter_b": inter_b, "band_pred": band_pred, "band_gt": band_gt})
    want = evaluation.instance_ap_voc(records, iou_thresh=0.5, boundary=True)
    np.testing.assert_array_equal(got["bap"], want["ap"])
    np.testing.assert_array_equal(got["bmap"], want["map"])
    plain = evaluation.instance_ap_voc(records, iou_thresh=0.5)
    np.testing.assert_array_equal(got["ap"], plain["ap"])
    off = runs["off"][0]["eval_ins_seg"]
    np.testing.assert_array_equal(got["ap"], off["ap"])
    assert got["bmap"] <= got["map"]                      # a minimum cannot raise a match
    rle = runs["rle"][0]["eval_ins_seg"]
    np.testing.assert_array_equal(rle["bap"], got["bap"])
    np.testing.assert_array_equal(rle["ap"], got["ap"])
    assert rle["bmap"] == got["bmap"] or (np.isnan(rle["bmap"]) and np.isnan(got["bmap"]))


def test_flag_off_output_and_keys_are_unchanged(tree, runs):
    """Without the flag, and with it at 0, the steps print the reference's lines and nothing else, and return the reference's
    keys: the text is rebuilt here from the returned dicts and a numpy confusion matrix."""
    from irn_amd.misc import evaluation
    from irn_amd.voc12 import eval_data
    conf = np.zeros((21, 21), np.int64)
    for name, pred, _ in tree["files"]:
        gt = eval_data.class_label(str(tree["root"]), name)
        p = np.where(pred == 255, 0, pred)
        keep = gt != 255
        conf += np.bincount(gt[keep].astype(int) * 21 + p[keep], minlength=441).reshape(21, 21)
    s = evaluation.sem_seg_scores(conf)
    for tag in ("off", "zero"):
        got, text = runs[tag]
        assert set(got) == {"eval_ins_seg", "eval_sem_seg"}
        assert set(got["eval_sem_seg"]) == {"iou", "miou"} and set(got["eval_ins_seg"]) == {"ap", "map"}
        np.testing.assert_array_equal(got["eval_sem_seg"]["iou"], s["iou"])
        want = "0.5iou: %s\n" % got["eval_ins_seg"]
        want += "%s %s\n%s %s\n%s\n" % (s["fp"][0], s["fn"][0], evaluation.mean(s["fp"][1:]), evaluation.mean(s["fn"][1:]),
                                        got["eval_sem_seg"])
        assert text == want, tag
    on, text_on = runs["on"]
    ins, sem = on["eval_ins_seg"], on["eval_sem_seg"]
    want = "0.5iou: %s\n0.5biou: %s\n" % ({"ap": ins["ap"], "map": ins["map"]}, {"ap": ins["bap"], "map": ins["bmap"]})
    want += "%s %s\n%s %s\n%s\n%s\n" % (s["fp"][0], s["fn"][0], evaluation.mean(s["fp"][1:]), evaluation.mean(s["fn"][1:]),
                                        {"iou": sem["iou"], "miou": sem["miou"]}, {"biou": sem["biou"], "mbiou": sem["mbiou"]})
    assert text_on == want


def test_a_band_wider_than_the_kernels_take_names_the_image_and_the_ratio(tree):
    with pytest.raises(ValueError, match=r"2008_000001: --boundary_iou_ratio 0.5 gives a band of 80 pixels"):
        _run(tree, "wide", tree["ins"], 0.5)
