"""infer_sem_seg's multi-scale and CRF modes (irn_amd/step/infer_sem_seg.py, --seg_infer_scales and --seg_crf_iters) on the GPU:
a seeded random-weight checkpoint, four synthetic images of 104x88 and 96x120, every run a fresh process.  The default flags
write the bytes they always wrote; the new modes write, bit for bit, what `ops.seg_fuse` and `ops.crf_prob` give when driven by
hand (tests/_infer_ms_child.py) on the same model and inputs, and the same bytes on a second run."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _train_cases import run_child  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = ["0.75", "1.0", "1.25"]


def _write_tree(root, n=4):
    from irn_amd import synth
    specs = []
    for i in range(n):
        h, w = (96, 120) if i % 2 else (104, 88)
        keys = [2 + i, 11]
        cls, _ = synth.blob_ground_truth(synth.cam_blobs(2, h, w, seed=40 + i), keys, 0.5, 0.35)
        specs.append({"name": "2007_%06d" % (i + 1), "photo": synth.photo(h, w, seed=i), "quality": 92, "keys": keys, "cls": cls})
    lst = os.path.join(root, "lists", "train.txt")
    return lst, synth.write_voc_tree(root, specs, lst), {s["name"]: s["cls"].shape for s in specs}


def _read(pred, names):
    return {n: open(os.path.join(pred, n + ".png"), "rb").read() for n in names}


def _maps(pred, names):
    return {n: np.asarray(Image.open(os.path.join(pred, n + ".png"))) for n in names}


@pytest.fixture(scope="module")
def runs(tmp_path_factory, request):
    """Every child process of this file, once: {tag: (what run_train_seg.main returned, the PNG bytes, the label maps)}."""
    from irn_amd.net import weights
    root = str(tmp_path_factory.mktemp("seg_ms"))
    lst, names, sizes = _write_tree(root)
    ckpt = os.path.join(root, "sess", "res50_seg")
    os.makedirs(os.path.dirname(ckpt))
    torch.save(weights.random_seg_state(seed=11), ckpt + ".pth")
    out = {"root": root, "lst": lst, "names": names, "sizes": sizes, "ckpt": ckpt}

    def infer(tag, extra):
        pred = os.path.join(root, "pred_" + tag)
        argv = ["--voc12_root", root, "--infer_list", lst, "--train_list", lst, "--seg_weights_name", ckpt, "--num_workers", "0",
                "--log_name", os.path.join(root, "log_" + tag), "--train_sem_seg_pass", "False", "--infer_sem_seg_pass", "True",
                "--seg_pred_dir", pred] + extra
        res, _ = run_child("run_train_seg", argv, os.path.join(root, tag + ".json"))
        assert sorted(os.listdir(pred)) == sorted(n + ".png" for n in names), tag
        out[tag] = (res, _read(pred, names), _maps(pred, names))

    infer("default", [])
    infer("one", ["--seg_infer_scales", "1.0"])
    infer("ms_a", ["--seg_infer_scales"] + SCALES)
    infer("ms_b", ["--seg_infer_scales"] + SCALES + ["--eval_seg_pass", "True"])
    infer("crf", ["--seg_crf_iters", "2"])
    env_path = os.environ.get("PYTHONPATH")
    os.environ["PYTHONPATH"] = os.path.dirname(os.path.abspath(__file__)) + (os.pathsep + env_path if env_path else "")
    try:
        out["hand"], _ = run_child("_infer_ms_child", [root, lst, ckpt + ".pth", ",".join(SCALES), "2"], os.path.join(root, "hand.json"))
    finally:
        if env_path is None:
            del os.environ["PYTHONPATH"]
        else:
            os.environ["PYTHONPATH"] = env_path
    return out


def test_scale_one_alone_is_the_default_path(runs):
    assert runs["default"][0]["infer_sem_seg"] == {"images": len(runs["names"])} == runs["one"][0]["infer_sem_seg"]
    assert runs["default"][1] == runs["one"][1], "--seg_infer_scales 1.0 wrote other bytes than no flag"
    for n, lab in runs["default"][2].items():
        assert lab.dtype == np.uint8 and lab.shape == runs["sizes"][n] and lab.max() <= 20


def test_multi_scale_runs_repeat_and_equal_seg_fuse_driven_by_hand(runs):
    res = runs["ms_a"][0]["infer_sem_seg"]
    assert res == {"images": len(runs["names"]), "scales": [0.75, 1.0, 1.25], "crf_iters": 0}
    assert runs["ms_a"][1] == runs["ms_b"][1], "a second multi-scale run wrote other bytes"
    for n in runs["names"]:
        want = np.asarray(runs["hand"][n]["fused"], np.uint8)
        got = runs["ms_a"][2][n]
        assert got.dtype == np.uint8 and got.shape == runs["sizes"][n] == want.shape
        assert np.array_equal(got, want), "%s: %d pixels differ from ops.seg_fuse driven by hand" % (n, int((got != want).sum()))
    differing = [n for n in runs["names"] if not np.array_equal(runs["ms_a"][2][n], runs["default"][2][n])]
    assert differing, "the random network gives the same map at one scale and at three: this test shows nothing about the fusion"


def test_the_crf_mode_writes_crf_prob_of_the_fusion(runs):
    assert runs["crf"][0]["infer_sem_seg"] == {"images": len(runs["names"]), "scales": [1.0], "crf_iters": 2}
    for n in runs["names"]:
        want = np.asarray(runs["hand"][n]["crf"], np.uint8)
        got = runs["crf"][2][n]
        assert np.array_equal(got, want), "%s: %d pixels differ from ops.crf_prob driven by hand" % (n, int((got != want).sum()))


def test_more_than_31_classes_with_the_crf_are_refused_before_the_first_image(runs):
    import run_train_seg
    from irn_amd.step import infer_sem_seg
    pred = os.path.join(runs["root"], "pred_refused")
    args = run_train_seg.build_parser().parse_args(
        ["--voc12_root", runs["root"], "--infer_list", runs["lst"], "--seg_weights_name", os.path.join(runs["root"], "no_such_checkpoint"),
         "--seg_pred_dir", pred, "--num_classes", "40", "--seg_crf_iters", "1"])
    with pytest.raises(ValueError, match=r"--seg_crf_iters 1 with --num_classes 40.*32 labels"):
        infer_sem_seg.run(args)                                             # ... before the checkpoint is even looked for
    assert not os.path.exists(pred)


def test_the_directory_is_scored_as_before(runs):
    scores = runs["ms_b"][0]["eval_sem_seg"]
    assert set(scores) == {"iou", "miou"} and 2 <= len(scores["iou"]) <= 21 and 0.0 <= scores["miou"] <= 1.0
