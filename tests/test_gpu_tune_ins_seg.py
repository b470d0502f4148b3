"""step/tune_ins_seg.py end to end through run_sample.py on a small synthetic VOC tree: the scores of a grid point are
EXACTLY those eval_ins_seg prints for the files make_ins_seg_labels writes at that point — at the configured point and at
a second one — and the step writes no file.  Both sides are the same integer counts through the same host AP code, so the
comparison has no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

os.environ.setdefault("MIOPEN_FIND_MODE", "2")     # fast find: the backbone is plumbing here, not the subject

N_IMAGES = 6


def _make_voc(tmp):
    """JPEGs, CAM files and ground truth of N_IMAGES images; CAMs and GT come from the same Gaussian blobs (2-3 classes per
    image, a void band where the blobs fade; one GT instance per class), so that detections meet instances whatever the
    random IRNet does."""
    from irn_amd import synth
    root = tmp / "voc"
    for d in ("JPEGImages", "SegmentationClass", "SegmentationObject", "ImageSets/Segmentation"):
        (root / d).mkdir(parents=True)
    (tmp / "cam").mkdir()
    (tmp / "lists").mkdir()
    rng = np.random.RandomState(0)
    names, labels = [], {}
    for i in range(N_IMAGES):
        name = "2008_%06d" % (i + 1)
        h, w = ((96, 128), (113, 150))[i % 2]
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8)
        Image.fromarray(img).resize((w, h), Image.BICUBIC).save(root / "JPEGImages" / (name + ".jpg"), quality=95)
        k = 2 + i % 2
        keys = np.sort(rng.choice(20, k, replace=False)).astype(np.int64)
        gh, gw = synth.grid_of((h, w))
        cam = synth.cam_blobs(k, gh, gw, seed=40 + i)
        np.save(tmp / "cam" / (name + ".npy"), {"keys": torch.from_numpy(keys), "cam": torch.from_numpy(cam)})
        up = np.repeat(np.repeat(cam, 4, axis=1), 4, axis=2)[:, :h, :w]
        top = up.max(axis=0)
        cls = np.where(top > 0.45, keys[up.argmax(axis=0)] + 1, 0).astype(np.uint8)
        obj = np.where(top > 0.45, 2 * up.argmax(axis=0) + 3, 0).astype(np.uint8)         # object ids 3, 5, 7: one per class
        cls[(top > 0.35) & (top <= 0.45)] = 255
        obj[(top > 0.35) & (top <= 0.45)] = 255
        R.save_p_png(root / "SegmentationClass" / (name + ".png"), cls)
        R.save_p_png(root / "SegmentationObject" / (name + ".png"), obj)
        lab = np.zeros(20, np.float32)
        lab[keys] = 1
        labels[int(name.replace("_", ""))] = lab
        names.append(name)
    (root / "ImageSets" / "Segmentation" / "train.txt").write_text("\n".join(names) + "\n")
    (tmp / "lists" / "train.txt").write_text("\n".join(names) + "\n")
    np.save(tmp / "lists" / "cls_labels.npy", labels)
    return root, names


def _run(tmp_path, root, ins_dir, extra):
    import run_sample
    from irn_amd.misc import pyutils
    from irn_amd.step import _common
    lst = str(tmp_path / "lists" / "train.txt")
    stdout = sys.stdout
    try:
        return run_sample.main(["--voc12_root", str(root), "--infer_list", lst, "--num_workers", "2", "--worker_devices", "0",
                                "--irn_weights_name", str(tmp_path / "res50_irn.pth"), "--cam_out_dir", str(tmp_path / "cam"),
                                "--sem_seg_out_dir", str(tmp_path / "sem"), "--ins_seg_out_dir", str(ins_dir),
                                "--log_name", str(tmp_path / "log"), "--make_cam_pass", "False", "--make_sem_seg_pass", "False"] + extra)
    finally:
        if isinstance(sys.stdout, pyutils.Logger):
            sys.stdout.close()
        sys.stdout = stdout
        _common.shutdown_workers()


def test_grid_points_equal_the_label_and_eval_steps(tmp_path, capsys):
    from irn_amd.net import weights
    from irn_amd.step import _common
    root, names = _make_voc(tmp_path)
    torch.save(weights.random_irn_state(2), tmp_path / "res50_irn.pth")
    first = (10.0, 8, 0.25)
    second = (6.0, 5, 0.4)
    want = {}
    for tag, (beta, exp_times, thres) in (("a", first), ("b", second)):
        ins = tmp_path / ("ins_" + tag)
        want[tag] = _run(tmp_path, root, ins, ["--eval_ins_seg_pass", "True", "--beta", str(beta), "--exp_times", str(exp_times),
                                               "--ins_seg_bg_thres", str(thres)])["eval_ins_seg"]
        print(tag, want[tag])
        # every image has a detection file: eval_ins_seg could not have run otherwise
        assert sorted(os.listdir(ins)) == [n + ".npy" for n in names]
    # not vacuous: the configured point scores, and the two points score differently
    assert np.isfinite(want["a"]["map"]) and want["a"]["map"] > 0
    assert not np.array_equal(want["a"]["ap"], want["b"]["ap"], equal_nan=True)
    # the step computes its own boundary maps (the label step's are dropped) and must still agree
    _common.EDGE_STORE.clear()
    capsys.readouterr()
    ins = tmp_path / "ins_tune"
    got = _run(tmp_path, root, ins, ["--make_ins_seg_pass", "False", "--tune_ins_seg_pass", "True", "--tune_beta", "6",
                                     "--tune_exp_times", "5", "--tune_ins_bg_thres", "0.4", "0.1"])
    assert set(got) == {"tune_ins_seg"}
    got = got["tune_ins_seg"]
    printed = capsys.readouterr().out
    print(got["grid"])
    assert os.listdir(ins) == []
    assert set(got) == {"ap", "map", "grid", "aps", "best"}
    assert set(got["grid"]) == set(got["aps"]) == {(b, e, t) for b in (6.0, 10.0) for e in (5, 8) for t in (0.1, 0.25, 0.4)}
    assert np.array_equal(got["ap"], want["a"]["ap"], equal_nan=True) and got["map"] == want["a"]["map"]
    assert np.array_equal(got["aps"][first], want["a"]["ap"], equal_nan=True) and got["grid"][first] == want["a"]["map"]
    assert np.array_equal(got["aps"][second], want["b"]["ap"], equal_nan=True) and got["grid"][second] == want["b"]["map"]
    assert len({np.asarray(v).tobytes() for v in got["aps"].values()}) >= 4
    assert got["grid"][got["best"]] == max(got["grid"].values())
    lines = [l for l in printed.split("\n") if l.startswith(("beta ", "best "))]
    assert len(lines) == 13 and lines[-1] == "best beta %g exp_times %d thres %g map %.6f" % (got["best"] + (got["grid"][got["best"]],))
    assert "beta 6 exp_times 5 thres 0.4 map %.6f" % want["b"]["map"] in lines
    assert "0.5iou: %s" % (want["a"],) in printed


def test_image_without_class_keys_is_refused_by_name(tmp_path):
    from irn_amd.net import weights
    root, names = _make_voc(tmp_path)
    torch.save(weights.random_irn_state(2), tmp_path / "res50_irn.pth")
    np.save(tmp_path / "cam" / (names[1] + ".npy"), {"keys": torch.zeros(0, dtype=torch.int64), "cam": torch.zeros(0, 29, 38)})
    with pytest.raises(ValueError, match=names[1]):
        _run(tmp_path, root, tmp_path / "ins", ["--make_ins_seg_pass", "False", "--tune_ins_seg_pass", "True"])
