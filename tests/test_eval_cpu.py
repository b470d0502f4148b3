"""Host side of the evaluation steps (irn_amd/voc12/eval_data.py, irn_amd/misc/evaluation.py, the run_sample.py flags)
against the chainercv restatement tests/_eval_ref.py.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_ref as R  # noqa: E402


def _voc(tmp_path, cls, obj=None, id="2008_000001"):
    for d in ("SegmentationClass", "SegmentationObject"):
        (tmp_path / d).mkdir(exist_ok=True)
    R.save_p_png(tmp_path / "SegmentationClass" / (id + ".png"), cls)
    if obj is not None:
        R.save_p_png(tmp_path / "SegmentationObject" / (id + ".png"), obj)
    return str(tmp_path), id


def test_seg_ids_in_file_order(tmp_path):
    from irn_amd.voc12 import eval_data
    d = tmp_path / "ImageSets" / "Segmentation"
    d.mkdir(parents=True)
    (d / "train.txt").write_text("2008_000009\n2007_000001\n\n2010_000123\n")
    assert eval_data.seg_ids(str(tmp_path), "train") == ["2008_000009", "2007_000001", "2010_000123"]


def test_class_label_palette_indices_and_l_mode(tmp_path):
    from PIL import Image
    from irn_amd.voc12 import eval_data
    cls = np.array([[0, 0, 255, 15], [3, 3, 255, 20]], np.uint8)
    root, id = _voc(tmp_path, cls)
    got = eval_data.class_label(root, id)
    assert got.dtype == np.uint8 and np.array_equal(got, cls)
    Image.fromarray(cls, mode="L").save(tmp_path / "SegmentationClass" / "l.png")
    assert np.array_equal(eval_data.class_label(root, "l"), cls)


def test_instance_label_chainercv_semantics(tmp_path):
    from irn_amd.voc12 import eval_data
    cls = np.array([[0, 5, 5, 255, 12, 12],
                    [0, 5, 5, 255, 12, 12],
                    [0, 0, 255, 255, 7, 7]], np.uint8)
    obj = np.array([[0, 9, 9, 255, 2, 2],          # non-contiguous ids 2, 7, 9; 255 and 0 are not instances
                    [0, 9, 9, 255, 2, 2],
                    [0, 0, 255, 255, 7, 7]], np.uint8)
    root, id = _voc(tmp_path, cls, obj)
    inst, inst_cls = eval_data.instance_label(root, id)
    assert inst.dtype == np.uint8
    # ascending object id -> 1..G: 2 -> 1 (class 12), 7 -> 2 (class 7), 9 -> 3 (class 5); classes 0-based
    assert np.array_equal(inst_cls, [11, 6, 4])
    assert np.array_equal(inst, np.where(obj == 2, 1, np.where(obj == 7, 2, np.where(obj == 9, 3, 0))))
    masks, labels = R.read_instances(root, id)
    assert np.array_equal(labels, inst_cls)
    for g in range(len(labels)):
        assert np.array_equal(masks[g], inst == g + 1)


def test_instance_on_background_is_an_error(tmp_path):
    from irn_amd.voc12 import eval_data
    cls = np.array([[0, 0, 3], [0, 3, 3]], np.uint8)
    obj = np.array([[1, 0, 2], [1, 2, 2]], np.uint8)         # object 1 lies on background
    root, id = _voc(tmp_path, cls, obj)
    with pytest.raises(ValueError, match="background"):
        eval_data.instance_label(root, id)


# ---------------------------------------------------------------------------------------------------------------------
# instance AP from counts vs chainercv from masks
# ---------------------------------------------------------------------------------------------------------------------
def _random_case(rng):
    n_img = rng.randint(1, 5)
    h, w = rng.randint(2, 7), rng.randint(2, 7)
    n_cls = rng.randint(1, 5)
    cases = []
    for _ in range(n_img):
        g = rng.randint(0, 4)
        gt_masks = rng.rand(g, h, w) < 0.4
        gt_labels = rng.randint(0, n_cls, g).astype(np.int32)
        n = 0 if rng.rand() < 0.15 else rng.randint(1, 7)
        pred = []
        for _ in range(n):
            r = rng.rand()
            if g and r < 0.35:                           # a copy of a GT instance (duplicates of one instance happen)
                pred.append(gt_masks[rng.randint(g)].copy())
            elif g and r < 0.5:                          # a GT instance with pixels flipped
                m = gt_masks[rng.randint(g)].copy()
                m[rng.rand(h, w) < 0.2] ^= True
                pred.append(m)
            else:
                pred.append(rng.rand(h, w) < rng.rand())
        pred_masks = np.array(pred, bool).reshape(n, h, w)
        pred_labels = rng.randint(0, n_cls + 1, n).astype(np.int64)      # class n_cls: only in predictions
        pred_scores = rng.choice(np.float32([0.0, 0.25, 0.5, 0.9, 1.0]), n) if rng.rand() < 0.5 else rng.rand(n).astype(np.float32)
        cases.append((pred_masks, pred_labels, pred_scores, gt_masks, gt_labels))
    return cases


def _records(cases):
    recs = []
    for pm, pl, ps, gm, gl in cases:
        recs.append({"pred_class": pl, "pred_score": ps, "gt_class": gl,
                     "inter": (pm[:, None] & gm[None]).sum(axis=(2, 3)).astype(np.int64),
                     "area_pred": pm.sum(axis=(1, 2)), "area_gt": gm.sum(axis=(1, 2))})
    return recs


def _check(cases):
    from irn_amd.misc import evaluation
    try:
        want = R.eval_instance_segmentation_voc(*[[c[i] for c in cases] for i in range(5)])
    except ValueError:                                     # no class anywhere: chainercv's max() of nothing
        with pytest.raises(ValueError):
            evaluation.instance_ap_voc(_records(cases))
        return
    got = evaluation.instance_ap_voc(_records(cases))
    np.testing.assert_array_equal(got["ap"], want["ap"])
    np.testing.assert_array_equal(got["map"], want["map"])


def test_instance_ap_vs_restatement_random():
    rng = np.random.RandomState(0)
    for _ in range(300):
        _check(_random_case(rng))


def test_instance_ap_edge_cases():
    h, w = 1, 4
    a = np.array([[[1, 0, 0, 0]]], bool)
    b = np.array([[[1, 1, 0, 0]]], bool)                   # iou(a, b) = 1 / 2 exactly: a match at 0.5
    cases = [(a, np.array([0]), np.float32([0.5]), b, np.array([0], np.int32))]
    _check(cases)
    from irn_amd.misc import evaluation
    assert evaluation.instance_ap_voc(_records(cases))["ap"][0] == 1.0
    # one GT matched twice (the second detection is a false positive), equal scores, a class only in predictions, a
    # class only in the ground truth and an image without predictions
    two = np.concatenate([b, b, a])
    cases = [(two, np.array([0, 0, 2]), np.float32([0.7, 0.7, 0.7]), b, np.array([0], np.int32)),
             (np.zeros((0, h, w), bool), np.zeros(0, np.int64), np.zeros(0, np.float32), np.concatenate([a, b]),
              np.array([1, 0], np.int32))]
    _check(cases)
    ap = evaluation.instance_ap_voc(_records(cases))["ap"]
    assert np.isnan(ap[2]) and ap[1] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# semantic confusion: iou length and values
# ---------------------------------------------------------------------------------------------------------------------
def _counts(preds, gts):
    conf = np.zeros((21, 21), np.int64)
    void = np.zeros(21, np.int64)
    for p, g in zip(preds, gts):
        m = g >= 0
        np.add.at(conf, (g[m], p[m]), 1)
        np.add.at(void, p[~m], 1)
    return conf, void


def test_iou_from_confusion_vs_restatement():
    from irn_amd.misc import evaluation
    rng = np.random.RandomState(1)
    for it in range(200):
        top = rng.randint(0, 21)
        preds, gts = [], []
        for _ in range(rng.randint(1, 4)):
            h, w = rng.randint(1, 6), rng.randint(1, 6)
            p = rng.randint(0, top + 1, (h, w))
            g = rng.randint(-1, top + 1, (h, w))
            if it % 5 == 0:                                # the largest label only where the GT is void
                g[:] = np.minimum(g, max(top - 3, 0))
                g[0, 0] = -1
                p[0, 0] = top
            preds.append(p)
            gts.append(g)
        want = R.calc_semantic_segmentation_confusion(preds, gts)
        conf, void = _counts(preds, gts)
        got, iou = evaluation.iou_from_confusion(conf, void)
        assert got.shape == want.shape and np.array_equal(got, want)
        np.testing.assert_array_equal(iou, R.iou_of(want))
        s = evaluation.sem_seg_scores(conf, void)
        w21 = want[:21, :21]
        np.testing.assert_array_equal(s["iou"], R.iou_of(w21))
        with np.errstate(divide="ignore", invalid="ignore"):
            den = w21.sum(1) + w21.sum(0) - np.diag(w21)
            np.testing.assert_array_equal(s["fp"], 1. - w21.sum(1) / den)
            np.testing.assert_array_equal(s["fn"], 1. - w21.sum(0) / den)


# ---------------------------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_parser_eval_passes_and_sweep():
    import run_sample
    p = run_sample.build_parser()
    a = p.parse_args(["--voc12_root", "x"])
    for name in ("eval_cam_pass", "eval_ins_seg_pass", "eval_sem_seg_pass"):
        assert getattr(a, name) is False
        assert name not in run_sample.OUT_OF_SCOPE
    assert a.cam_eval_thres == 0.15 and a.cam_eval_thres_sweep == []
    assert set(run_sample.OUT_OF_SCOPE) == {"train_cam_pass", "train_irn_pass"}
    a = p.parse_args(["--voc12_root", "x", "--eval_cam_pass", "True", "--eval_sem_seg_pass", "1",
                      "--cam_eval_thres_sweep", "0.05", "0.1", "0.6"])
    assert a.eval_cam_pass is True and a.eval_sem_seg_pass is True and a.eval_ins_seg_pass is False
    assert a.cam_eval_thres_sweep == [0.05, 0.1, 0.6]
    help_text = p.format_help()
    i = help_text.index("--cam_eval_thres ")
    assert "ignored" not in help_text[i:help_text.index("--cam_eval_thres_sweep")]


def test_train_passes_still_refuse(tmp_path):
    import run_sample
    for name in ("--train_cam_pass", "--train_irn_pass"):
        with pytest.raises(SystemExit):
            run_sample.main(["--voc12_root", str(tmp_path), name, "True", "--log_name", str(tmp_path / "log")])


def test_eval_thresholds_validation():
    torch = pytest.importorskip("torch")
    from irn_amd import ops
    with pytest.raises(ValueError):
        ops.eval_thresholds([0.2, 0.1], torch.device("cpu"))
    with pytest.raises(ValueError):
        ops.eval_thresholds(np.linspace(0, 1, 257), torch.device("cpu"))
    assert ops.eval_thresholds([0.15], torch.device("cpu")).dtype == torch.float32


def test_c_entries_reject_bad_arguments():
    """Argument checks run before anything touches the GPU: IRN_ERR_ARG on a machine without one too."""
    from irn_amd._lib import lib
    p = 16                                                  # any non-null pointer value: never dereferenced here
    assert lib.irn_cam_confusion(p, p, 1, p, 4, 4, p, 0, 21, p, p, None) == 1              # t < 1
    assert lib.irn_cam_confusion(p, p, 1, p, 4, 4, p, 257, 21, p, p, None) == 1            # t over the cap
    assert lib.irn_cam_confusion(p, p, 21, p, 4, 4, p, 1, 21, p, p, None) == 1             # k over 20
    assert lib.irn_cam_confusion(None, None, 1, p, 4, 4, p, 1, 21, p, p, None) == 1        # k > 0 without planes
    assert lib.irn_cam_confusion(p, p, 1, p, 0, 4, p, 1, 21, p, p, None) == 1              # empty image
    assert lib.irn_cam_confusion(p, p, 1, p, 4, 4, p, 1, 21, None, p, None) == 1           # no accumulator
    assert lib.irn_cam_confusion_reduce(p, 0, 21, p, None, None) == 1
    assert lib.irn_cam_confusion_reduce(None, 1, 21, p, None, None) == 1
    assert lib.irn_label_confusion(p, p, 4, -1, 0, 21, p, None, p, None) == 1
    assert lib.irn_label_confusion(p, None, 4, 4, 0, 21, p, None, p, None) == 1
    assert lib.irn_label_confusion(p, p, 4, 4, 21, 21, p, None, p, None) == 1
    assert lib.irn_mask_overlap(p, -1, p, 1, 4, 4, p, p, p, p, None) == 1
    assert lib.irn_mask_overlap(p, 1, p, 256, 4, 4, p, p, p, p, None) == 1
    assert lib.irn_mask_overlap(None, 2, p, 1, 4, 4, p, p, p, p, None) == 1
    assert lib.irn_mask_overlap(p, 1, p, 1, 4, 4, p, p, p, None, None) == 1
    assert b"irn_mask_overlap" in lib.irn_last_error()
