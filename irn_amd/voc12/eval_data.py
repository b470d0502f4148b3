"""Ground truth of the evaluation steps: the reads chainercv's VOCSemanticSegmentationDataset and
VOCInstanceSegmentationDataset make for step/eval_cam.py, step/eval_sem_seg.py and step/eval_ins_seg.py, without
chainercv.

    seg_ids(voc12_root, split)        ImageSets/Segmentation/<split>.txt, one id per line, in file order
    class_label(voc12_root, id)       SegmentationClass/<id>.png palette indices, uint8 [H,W] (255 = void)
    instance_label(voc12_root, id)    (inst_map uint8 [H,W], inst_class int64 [G]) of SegmentationObject/<id>.png

Instances follow chainercv's `image_wise_to_instance_wise`: object ids 0 and 255 are not instances, the others are
taken in ascending order and renumbered 1..G (0 = no instance), and an instance's class is
`np.unique(class_label[inst == id])[0] - 1` (0-based, 0 = aeroplane).  An instance whose class would be background
(-1) or void is an error, as chainercv asserts.
"""
import os

import numpy as np
from PIL import Image

N_FG = 20                             # VOC; a step with --num_classes passes its own


def seg_ids(voc12_root, split):
    path = os.path.join(voc12_root, "ImageSets", "Segmentation", split + ".txt")
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def _palette_png(path):
    img = Image.open(path)
    if img.mode not in ("P", "L"):
        raise ValueError("%s: a VOC label PNG has mode P or L, not %s" % (path, img.mode))
    return np.array(img, dtype=np.uint8)


def class_label(voc12_root, id):
    return _palette_png(os.path.join(voc12_root, "SegmentationClass", id + ".png"))


def instance_label(voc12_root, id, n_fg=N_FG):
    """`n_fg`: the dataset's foreground classes; an instance's class lies in 0..n_fg-1."""
    obj = _palette_png(os.path.join(voc12_root, "SegmentationObject", id + ".png"))
    cls = class_label(voc12_root, id)
    if obj.shape != cls.shape:
        raise ValueError("%s: SegmentationObject %s and SegmentationClass %s differ in shape" % (id, obj.shape, cls.shape))
    ids = np.unique(obj)
    ids = ids[(ids != 0) & (ids != 255)]
    inst_map = np.zeros(obj.shape, np.uint8)
    inst_class = np.empty(len(ids), np.int64)
    for g, oid in enumerate(ids):
        m = obj == oid
        lbl = int(np.unique(cls[m])[0]) - 1
        if not 0 <= lbl < n_fg:
            raise ValueError("%s: object %d has class %d (background or void)" % (id, int(oid), lbl))
        inst_map[m] = g + 1
        inst_class[g] = lbl
    return inst_map, inst_class
