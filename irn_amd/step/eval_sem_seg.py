"""Semantic-segmentation evaluation step — drop-in for reference step/eval_sem_seg.py (`run(args)`).

Reads  args.voc12_root (ImageSets/Segmentation/<args.chainer_eval_set>.txt, SegmentationClass/<id>.png),
       args.sem_seg_out_dir/<id>.png
Prints fp[0] fn[0], the mean fp / fn of the classes 1..C (C = --num_classes, 20 by default) and {'iou': ..., 'miou': ...} in the reference's format;
returns the {'iou', 'miou'} dict.

Prediction 255 reads as 0 (step/eval_sem_seg.py:14); the confusion is counted per image on the device
(`ops.label_confusion`) into one int64 matrix for the whole split.

With --boundary_iou_ratio R > 0 (not in the reference) every image also adds its Boundary IoU counts
(`ops.label_boundary_counts`, band width `ops.boundary_distance(h, w, R)`) into one int64 [C+1,3] accumulator; the step then
prints {'biou': ..., 'mbiou': ...} after the reference's three lines and returns the dict with those two keys added.
"""
import os

import numpy as np
import torch
from PIL import Image

from .. import ops
from ..misc import evaluation
from ..voc12 import eval_data
from . import _classes, _eval


def run(args):
    ids = eval_data.seg_ids(args.voc12_root, args.chainer_eval_set)
    dev = _eval.device()
    c = _classes.num_classes(args)
    ratio = _eval.boundary_ratio(args)

    def load(id):
        gt = eval_data.class_label(args.voc12_root, id)
        pred = np.asarray(Image.open(os.path.join(args.sem_seg_out_dir, id + ".png")), dtype=np.uint8)
        _eval.check_shape(id, "prediction", pred.shape, gt.shape)
        return {"gt": gt, "pred": pred}

    with torch.cuda.device(dev):
        conf = void = bad = band = None
        for id, it in _eval.items(ids, load, args):
            pred, gt = it["pred"].to(dev, non_blocking=True), it["gt"].to(dev, non_blocking=True)
            conf, void, bad = ops.label_confusion(pred, gt, conf, bad, pred_255_as=0, void=void, n_classes=c + 1)
            if ratio:
                band, bad = ops.label_boundary_counts(pred, gt, _eval.boundary_d(id, gt.shape, ratio), band, bad, pred_255_as=0,
                                                      n_classes=c + 1)
        if conf is None:
            raise ValueError("eval_sem_seg: the split %s lists no images" % args.chainer_eval_set)
        _eval.raise_if_bad(bad, "eval_sem_seg", c)
        conf, void = conf.cpu().numpy(), void.cpu().numpy()

    s = evaluation.sem_seg_scores(conf, void)
    fp, fn, iou = s["fp"], s["fn"], s["iou"]
    print(fp[0], fn[0])
    print(evaluation.mean(fp[1:]), evaluation.mean(fn[1:]))
    out = {"iou": iou, "miou": evaluation.nanmean(iou)}
    print(out)
    if ratio:
        b = evaluation.boundary_iou_scores(band.cpu().numpy())
        print(b)
        out.update(b)
    return out
