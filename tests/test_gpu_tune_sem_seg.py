"""step/tune_sem_seg.py end to end through run_sample.py on a small synthetic VOC tree: the scores of a grid point are
EXACTLY those eval_sem_seg prints for the files make_sem_seg_labels writes at that point — at the configured point and
at a second one — and the step writes no file."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _steps as S  # noqa: E402

pytestmark = pytest.mark.gpu

os.environ.setdefault("MIOPEN_FIND_MODE", "2")     # fast find: the backbone is plumbing here, not the subject

N_IMAGES = 6


def _make_voc(tmp):
    """JPEGs, CAM files and ground truth of N_IMAGES images; CAMs and GT come from the same Gaussian blobs (2-3 classes per
    image, a void band where the blobs fade), so that labels of several classes exist whatever the random IRNet does."""
    from irn_amd import synth
    rng = np.random.RandomState(0)
    specs = []
    for i in range(N_IMAGES):
        h, w = ((96, 128), (113, 150))[i % 2]
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8)
        k = 2 + i % 2
        keys = np.sort(rng.choice(20, k, replace=False)).astype(np.int64)
        cam = synth.cam_blobs(k, *synth.grid_of((h, w)), seed=40 + i)
        specs.append({"name": "2008_%06d" % (i + 1), "photo": np.asarray(Image.fromarray(img).resize((w, h), Image.BICUBIC)),
                      "quality": 95, "keys": keys, "cls": synth.blob_ground_truth(synth.upsample4(cam, (h, w)), keys, 0.45, 0.35)[0],
                      "cam": {"keys": torch.from_numpy(keys), "cam": torch.from_numpy(cam)}})
    return tmp / "voc", synth.write_voc_tree(tmp / "voc", specs, tmp / "lists" / "train.txt", cam_dir=tmp / "cam", cls_labels=20)


def _run(tmp_path, root, sem_dir, extra):
    lst = str(tmp_path / "lists" / "train.txt")
    return S.run_sample_main(["--voc12_root", str(root), "--infer_list", lst, "--num_workers", "2", "--worker_devices", "0",
                              "--irn_weights_name", str(tmp_path / "res50_irn.pth"), "--cam_out_dir", str(tmp_path / "cam"),
                              "--sem_seg_out_dir", str(sem_dir), "--ins_seg_out_dir", str(tmp_path / "ins"),
                              "--log_name", str(tmp_path / "log"), "--make_cam_pass", "False", "--make_ins_seg_pass", "False"] + extra)


def test_grid_points_equal_the_label_and_eval_steps(tmp_path, capsys):
    from irn_amd.net import weights
    from irn_amd.step import _common
    root, names = _make_voc(tmp_path)
    torch.save(weights.random_irn_state(2), tmp_path / "res50_irn.pth")
    first = (10.0, 8, 0.25)
    second = (6.0, 5, 0.4)
    want = {}
    for tag, (beta, exp_times, thres) in (("a", first), ("b", second)):
        sem = tmp_path / ("sem_" + tag)
        want[tag] = _run(tmp_path, root, sem, ["--eval_sem_seg_pass", "True", "--beta", str(beta), "--exp_times", str(exp_times),
                                               "--sem_seg_bg_thres", str(thres)])["eval_sem_seg"]
        assert sorted(os.listdir(sem)) == [n + ".png" for n in names]
    # not vacuous: the two points score differently, and the configured one predicts several labels
    assert not np.array_equal(want["a"]["iou"], want["b"]["iou"], equal_nan=True)
    seen = set()
    for n in names:
        seen |= set(np.unique(np.asarray(Image.open(tmp_path / "sem_a" / (n + ".png")))).tolist())
    assert len(seen) >= 3, seen
    # the step computes its own boundary maps (the label step's are dropped) and must still agree
    _common.EDGE_STORE.clear()
    capsys.readouterr()
    sem = tmp_path / "sem_tune"
    got = _run(tmp_path, root, sem, ["--make_sem_seg_pass", "False", "--tune_sem_seg_pass", "True", "--tune_beta", "6",
                                     "--tune_exp_times", "5", "--tune_bg_thres", "0.4", "0.1"])
    assert set(got) == {"tune_sem_seg"}
    got = got["tune_sem_seg"]
    printed = capsys.readouterr().out
    assert os.listdir(sem) == []
    assert set(got["grid"]) == {(b, e, t) for b in (6.0, 10.0) for e in (5, 8) for t in (0.1, 0.25, 0.4)}
    assert np.array_equal(got["iou"], want["a"]["iou"], equal_nan=True) and got["miou"] == want["a"]["miou"]
    assert np.array_equal(got["ious"][first], want["a"]["iou"], equal_nan=True) and got["grid"][first] == want["a"]["miou"]
    assert np.array_equal(got["ious"][second], want["b"]["iou"], equal_nan=True) and got["grid"][second] == want["b"]["miou"]
    assert len({np.asarray(v).tobytes() for v in got["ious"].values()}) >= 6
    assert got["grid"][got["best"]] == max(got["grid"].values())
    lines = [l for l in printed.split("\n") if l.startswith(("beta ", "best "))]
    assert len(lines) == 13 and lines[-1] == "best beta %g exp_times %d thres %g miou %.6f" % (got["best"] + (got["grid"][got["best"]],))
    assert "beta 6 exp_times 5 thres 0.4 miou %.6f" % want["b"]["miou"] in lines


def test_image_without_class_keys_is_refused_by_name(tmp_path):
    from irn_amd.net import weights
    root, names = _make_voc(tmp_path)
    torch.save(weights.random_irn_state(2), tmp_path / "res50_irn.pth")
    np.save(tmp_path / "cam" / (names[1] + ".npy"), {"keys": torch.zeros(0, dtype=torch.int64), "cam": torch.zeros(0, 29, 38)})
    with pytest.raises(ValueError, match=names[1]):
        _run(tmp_path, root, tmp_path / "sem", ["--make_sem_seg_pass", "False", "--tune_sem_seg_pass", "True"])
