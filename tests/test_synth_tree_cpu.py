"""irn_amd/synth.py's ground-truth recipe and tree writer, no GPU: the four trees the step tests build through them
(tune_sem_seg, tune_ins_seg, tune_ir_label with one image without keys, 80 classes) hold exactly what the builders held that
each of those tests carried before the writer existed.  The digests below were taken from those earlier builders' trees, not
from the writer; JPEG bytes depend on the libjpeg build and are not part of them."""
import hashlib
import os

import numpy as np
from PIL import Image

import test_gpu_num_classes_steps
import test_gpu_tune_ins_seg
import test_gpu_tune_ir_label
import test_gpu_tune_sem_seg

LISTS = ["lists/cls_labels.npy", "lists/train.txt", "voc/ImageSets/Segmentation/train.txt"]
TREES = {
    "sem": (test_gpu_tune_sem_seg._make_voc, 6, ("cam", "JPEGImages", "SegmentationClass"), LISTS,
            "7a53f8900566124fddd2f59aacc31843a7d405a2633b719f168a5c72e248b279"),
    "ins": (test_gpu_tune_ins_seg._make_voc, 6, ("cam", "JPEGImages", "SegmentationClass", "SegmentationObject"), LISTS,
            "b74d56664d7a727a66a4b112feb29b27a8814507070f30d2d54b07efc73ce0b5"),
    "ir": (lambda tmp: test_gpu_tune_ir_label._make_voc(tmp, 6, no_keys=(4,)), 6, ("cam", "JPEGImages", "SegmentationClass"), LISTS[1:],
           "ccfbe8e898f4f3085f068121d7917a59ba592e28df9e94ab4ab5a64d92b5eebd"),
    "c80": (test_gpu_num_classes_steps._make_voc, 4, ("JPEGImages", "SegmentationClass", "SegmentationObject"), LISTS,
            "fd1c5a58c0c6a2faa9c4ef6149b9d33a96c6c3c01a11eca08b904b2d5a971c18"),
}
EXT = {"cam": ".npy", "JPEGImages": ".jpg"}


def files_of(tmp):
    return sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs)


def digest(tmp, names):
    """SHA-256 over, per name in order: the CAM file's keys (int64) and planes (float32), the decoded class map, the decoded
    object map, the image's cls_labels row — each where the tree has it."""
    tmp = str(tmp)
    h = hashlib.sha256()
    labels = os.path.join(tmp, "lists", "cls_labels.npy")
    labels = np.load(labels, allow_pickle=True).item() if os.path.exists(labels) else None
    for n in sorted(names):
        if os.path.exists(os.path.join(tmp, "cam", n + ".npy")):
            d = np.load(os.path.join(tmp, "cam", n + ".npy"), allow_pickle=True).item()
            h.update(np.asarray(d["keys"], np.int64).tobytes())
            h.update(np.asarray(d["cam"] if "cam" in d else d["high_res"], np.float32).tobytes())
        for d in ("SegmentationClass", "SegmentationObject"):
            if os.path.exists(os.path.join(tmp, "voc", d, n + ".png")):
                h.update(np.asarray(Image.open(os.path.join(tmp, "voc", d, n + ".png")), np.uint8).tobytes())
        if labels is not None:
            h.update(np.asarray(labels[int(n.replace("_", ""))], np.float32).tobytes())
    return h.hexdigest()


def test_the_step_tests_trees_are_the_ones_they_always_ran_on(tmp_path):
    for tag, (make, n, dirs, lists, want) in TREES.items():
        tmp = tmp_path / tag
        tmp.mkdir()
        root, names = make(tmp)
        assert root == tmp / "voc" and names == ["2008_%06d" % (i + 1) for i in range(n)], tag
        per_image = [os.path.join("voc" if d != "cam" else "", d, nm + EXT.get(d, ".png")) for d in dirs for nm in names]
        assert files_of(tmp) == sorted(per_image + lists), tag
        for nm in names:
            labels = set(np.unique(np.asarray(Image.open(root / "SegmentationClass" / (nm + ".png")))).tolist())
            assert {0, 255} <= labels and len(labels - {0, 255}) >= 2, (tag, nm, labels)
        assert digest(tmp, names) == want, tag


def test_ground_truth_recipe_on_a_hand_made_cam():
    from irn_amd import synth
    cam = np.float32([[[0.9, 0.42, 0.3, 0.7, 0.45]],
                      [[0.1, 0.10, 0.2, 0.7, 0.46]]])              # above | in the band | below | a tie | on the cut and just above
    cls, obj = synth.blob_ground_truth(cam, np.int64([4, 11]), 0.45, 0.35)
    assert obj is None and cls.dtype == np.uint8 and cls.tolist() == [[5, 255, 0, 5, 12]]
    cls2, obj = synth.blob_ground_truth(cam, [4, 11], 0.45, 0.35, obj_ids=[3, 7])
    assert np.array_equal(cls2, cls) and obj.dtype == np.uint8 and obj.tolist() == [[3, 255, 0, 3, 7]]
    assert synth.blob_ground_truth(np.float32([[[0.45, 0.35]]]), [0], 0.45, 0.35)[0].tolist() == [[255, 0]]   # a value on a cut falls below it
    up = synth.upsample4(np.arange(6, dtype=np.float32).reshape(1, 2, 3), (5, 9))
    assert up.shape == (1, 5, 9) and up[0, :, 0].tolist() == [0, 0, 0, 0, 3] and up[0, 0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2]
