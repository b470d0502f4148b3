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
import _steps as S  # noqa: E402

pytestmark = pytest.mark.gpu

os.environ.setdefault("MIOPEN_FIND_MODE", "2")     # fast find: the backbone is plumbing here, not the subject

N_IMAGES = 6


def _make_voc(tmp):
    """JPEGs, CAM files and ground truth of N_IMAGES images; CAMs and GT come from the same Gaussian blobs (2-3 classes per
    image, a void band where the blobs fade; one GT instance per class), so that detections meet instances whatever the
    random IRNet does."""
    from irn_amd import synth
    rng = np.random.RandomState(0)
    specs = []
    for i in range(N_IMAGES):
        h, w = ((96, 128), (113, 150))[i % 2]
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8)
        k = 2 + i % 2
        keys = np.sort(rng.choice(20, k, replace=False)).astype(np.int64)
        cam = synth.cam_blobs(k, *synth.grid_of((h, w)), seed=40 + i)
        cls, obj = synth.blob_ground_truth(synth.upsample4(cam, (h, w)), keys, 0.45, 0.35, obj_ids=2 * np.arange(k) + 3)   # 3, 5, 7
        specs.append({"name": "2008_%06d" % (i + 1), "photo": np.asarray(Image.fromarray(img).resize((w, h), Image.BICUBIC)),
                      "quality": 95, "keys": keys, "cls": cls, "obj": obj,
                      "cam": {"keys": torch.from_numpy(keys), "cam": torch.from_numpy(cam)}})
    return tmp / "voc", synth.write_voc_tree(tmp / "voc", specs, tmp / "lists" / "train.txt", cam_dir=tmp / "cam", cls_labels=20)


def _run(tmp_path, root, ins_dir, extra):
    lst = str(tmp_path / "lists" / "train.txt")
    return S.run_sample_main(["--voc12_root", str(root), "--infer_list", lst, "--num_workers", "2", "--worker_devices", "0",
                              "--irn_weights_name", str(tmp_path / "res50_irn.pth"), "--cam_out_dir", str(tmp_path / "cam"),
                              "--sem_seg_out_dir", str(tmp_path / "sem"), "--ins_seg_out_dir", str(ins_dir),
                              "--log_name", str(tmp_path / "log"), "--make_cam_pass", "False", "--make_sem_seg_pass", "False"] + extra)


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
