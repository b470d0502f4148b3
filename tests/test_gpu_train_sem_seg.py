"""The segmentation steps on the GPU (irn_amd/step/train_sem_seg.py, infer_sem_seg.py, run_train_seg.py) at small shapes:
crop 64, batch 2, one epoch over four synthetic images, random initial weights.  Two fresh processes — the loader with and
without workers, the batch built on the host and on the device — write the same checkpoint and see the same first loss; the
composed loss agrees with the fused one; inference writes one label map per image, the same bytes on a second run, and
eval_sem_seg scores them."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _train_cases import run_child  # noqa: E402

pytestmark = pytest.mark.gpu


def _write_tree(root, n=4):
    """A VOC tree of n photo-like images with blob ground truth, and the same maps as training labels in <root>/sem_seg."""
    from irn_amd import synth
    specs = []
    for i in range(n):
        h, w = (96, 120) if i % 2 else (104, 88)
        keys = [2 + i, 11]
        cam = synth.cam_blobs(2, h, w, seed=40 + i)
        cls, _ = synth.blob_ground_truth(cam, keys, 0.5, 0.35)
        specs.append({"name": "2007_%06d" % (i + 1), "photo": synth.photo(h, w, seed=i), "quality": 92, "keys": keys, "cls": cls})
    lst = os.path.join(root, "lists", "train.txt")
    names = synth.write_voc_tree(root, specs, lst)
    label_dir = os.path.join(root, "sem_seg")
    os.makedirs(label_dir)
    for s in specs:
        Image.fromarray(s["cls"]).save(os.path.join(label_dir, s["name"] + ".png"))
    return lst, label_dir, names, {s["name"]: s["cls"].shape for s in specs}


def _argv(root, lst, label_dir, tag, workers=0, augment="device", loss="fused"):
    out = os.path.join(root, "sess_" + tag, "res50_seg")
    return out, ["--voc12_root", root, "--train_list", lst, "--infer_list", lst, "--seg_label_dir", label_dir,
                 "--seg_crop_size", "64", "--seg_batch_size", "2", "--seg_num_epoches", "1", "--num_workers", str(workers),
                 "--seg_weights_name", out, "--log_name", os.path.join(root, "log_" + tag), "--seed", "4",
                 "--seg_augment", augment, "--seg_loss", loss, "--seg_pred_dir", os.path.join(root, "pred_" + tag),
                 # the seeded random weights give logits far larger than a trained network's: a small rate keeps step 2 finite
                 "--seg_learning_rate", "1e-6"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("seg"))
    return (root,) + _write_tree(root)


@pytest.fixture(scope="module")
def trained(tree):
    """Run a: no loader workers, the batch built on the host.  Run b: two workers, on the device."""
    root, lst, label_dir, _, _ = tree
    runs = {}
    for tag, workers, augment in (("a", 0, "host"), ("b", 2, "device")):
        out, argv = _argv(root, lst, label_dir, tag, workers, augment)
        res, stdout = run_child("run_train_seg", argv, out + ".json")
        runs[tag] = (res["train_sem_seg"], torch.load(out + ".pth", map_location="cpu", weights_only=True), out, stdout)
    return runs


def test_two_processes_write_the_same_checkpoint_and_see_the_same_first_loss(trained):
    from irn_amd.net import weights
    from irn_amd.net.resnet50_seg import Net
    (res0, state0, _, stdout0), (res1, state1, _, _) = trained["a"], trained["b"]
    print("\nfirst loss a (host, 0 workers): %r / b (device, 2 workers): %r" % (res0["first_loss"], res1["first_loss"]))
    assert res0["steps"] == res1["steps"] == 2 and "step:    0/    2 loss:" in stdout0
    assert np.isfinite(res0["first_loss"]) and res0["first_loss"] == res1["first_loss"]
    assert list(state0) == list(state1) == list(Net().state_dict().keys())
    assert all(torch.isfinite(v).all() for v in state0.values()), "the run diverged"
    differing = [k for k in state0 if not torch.equal(state0[k], state1[k])]
    assert not differing, "the two runs differ in %s" % differing
    initial = weights.random_seg_state()
    assert not torch.equal(state0["head.branches.0.weight"], initial["head.branches.0.weight"])          # it trained
    assert not torch.equal(state0["resnet50.layer4.0.conv1.weight"], initial["resnet50.layer4.0.conv1.weight"])
    assert torch.equal(state0["resnet50.layer2.0.conv1.weight"], initial["resnet50.layer2.0.conv1.weight"])


def test_the_composed_loss_agrees_with_the_fused_one(tree, trained):
    """Two fp32 evaluations of one function on the same first batch: a sanity bound, not a precision claim."""
    root, lst, label_dir, _, _ = tree
    out, argv = _argv(root, lst, label_dir, "c", 0, "device", "composed")
    res, _ = run_child("run_train_seg", argv, out + ".json")
    fused, composed = trained["b"][0]["first_loss"], res["train_sem_seg"]["first_loss"]
    print("\nfirst loss fused %r, composed %r" % (fused, composed))
    assert abs(composed - fused) <= 1e-4 * abs(fused)


def test_inference_writes_one_map_per_image_twice_the_same_and_is_scored(tree, trained):
    root, lst, label_dir, names, sizes = tree
    _, argv = _argv(root, lst, label_dir, "a")
    argv += ["--train_sem_seg_pass", "False", "--infer_sem_seg_pass", "True", "--eval_seg_pass", "True"]
    pred = os.path.join(root, "pred_a")
    runs = []
    for i in range(2):
        res, stdout = run_child("run_train_seg", argv, os.path.join(root, "infer_%d.json" % i))
        assert res["infer_sem_seg"] == {"images": len(names)} and "train_sem_seg" not in res
        assert sorted(os.listdir(pred)) == sorted(n + ".png" for n in names)
        runs.append((res, {n: open(os.path.join(pred, n + ".png"), "rb").read() for n in names}))
        for n in names:
            lab = np.asarray(Image.open(os.path.join(pred, n + ".png")))
            assert lab.dtype == np.uint8 and lab.shape == sizes[n] and lab.max() <= 20
    assert runs[0][1] == runs[1][1], "a second run wrote other bytes"
    scores = runs[0][0]["eval_sem_seg"]
    # (eval_sem_seg's dict: one IoU per label up to the highest one that occurs, NaN for a label that never does)
    assert set(scores) == {"iou", "miou"} and 2 <= len(scores["iou"]) <= 21 and 0.0 <= scores["miou"] <= 1.0
    again = runs[1][0]["eval_sem_seg"]
    assert np.array_equal(np.asarray(scores["iou"], float), np.asarray(again["iou"], float), equal_nan=True)
