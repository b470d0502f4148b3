"""Instance-segmentation evaluation step — drop-in for reference step/eval_ins_seg.py (`run(args)`).

Reads  args.voc12_root (ImageSets/Segmentation/<args.chainer_eval_set>.txt, SegmentationObject/<id>.png,
       SegmentationClass/<id>.png), args.ins_seg_out_dir/<id>.npy ({'score', 'mask', 'class'} of make_ins_seg_labels), or —
       when that file does not exist — <id>.rle.npz (its --ins_seg_format rle), decoded to masks on the host
Prints 0.5iou: {'ap': ..., 'map': ...} as the reference does; returns the dict.

Per image the device counts |mask & instance|, |mask| and |instance| for every predicted mask and GT instance
(`ops.mask_overlap`); the counts of the whole split come back in one copy, and chainercv's matching and VOC AP
(iou_thresh 0.5, not the 07 metric) run on them in split order (`misc.evaluation.instance_ap_voc`).

With --boundary_iou_ratio R > 0 (not in the reference) every image also gets its band counts (`ops.mask_boundary_overlap`, band
width `ops.boundary_distance(h, w, R)`); they ride the same copy, and the step prints 0.5biou: {'ap': ..., 'map': ...} — Boundary
AP, matched on min(mask IoU, boundary IoU) — after the reference's line and returns the dict with 'bap' and 'bmap' added.
"""
import os

import numpy as np
import torch

from .. import ops
from ..misc import evaluation
from ..voc12 import eval_data
from . import _classes, _eval


def load_rle(path):
    """An <id>.rle.npz of make_ins_seg_labels as the {'score', 'mask', 'class'} dict of its <id>.npy."""
    with np.load(path, allow_pickle=False) as z:
        h, w = (int(v) for v in z["size"])
        counts, offsets = z["counts"], z["offsets"]
        if len(offsets) != len(z["class"]) + 1:
            raise ValueError("%d offsets for %d classes" % (len(offsets), len(z["class"])))
        masks = [ops.rle_decode(counts[offsets[i]:offsets[i + 1]], h, w) for i in range(len(offsets) - 1)]
        return {"score": z["score"], "class": z["class"], "mask": np.stack(masks) if masks else np.zeros((0, h, w), bool)}


def run(args):
    ids = eval_data.seg_ids(args.voc12_root, args.chainer_eval_set)
    dev = _eval.device()
    c = _classes.num_classes(args)
    ratio = _eval.boundary_ratio(args)
    fields = (("inter", "ng"), ("area_pred", "n"), ("area_gt", "g")) + ((("inter_b", "ng"), ("band_pred", "n"), ("band_gt", "g")) if ratio else ())

    def load(id):
        inst_map, inst_class = eval_data.instance_label(args.voc12_root, id, n_fg=c)
        path = os.path.join(args.ins_seg_out_dir, id + ".npy")
        rle_path = os.path.join(args.ins_seg_out_dir, id + ".rle.npz")
        if not os.path.exists(path) and os.path.exists(rle_path):
            det = load_rle(rle_path)
        else:
            det = np.load(path, allow_pickle=True).item()
        cls, score = np.asarray(det["class"]).reshape(-1), np.asarray(det["score"]).reshape(-1)
        mask = np.asarray(det["mask"])
        if mask.size == 0 and len(cls) == 0:
            mask = np.zeros((0,) + inst_map.shape, bool)
        _eval.check_shape(id, "masks", mask.shape, (len(cls),) + inst_map.shape)
        if len(score) != len(cls):
            raise ValueError("%d scores for %d classes" % (len(score), len(cls)))
        return {"inst_map": inst_map, "inst_class": inst_class, "mask": np.ascontiguousarray(mask),
                "class": cls, "score": score}

    records, counts = [], []
    with torch.cuda.device(dev):
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        inst_band = None
        for id, it in _eval.items(ids, load, args):
            g = int(it["inst_class"].numel())
            mask, inst_map = it["mask"].to(dev, non_blocking=True), it["inst_map"].to(dev, non_blocking=True)
            inter, area_pred, area_gt = ops.mask_overlap(mask, inst_map, g, bad)
            counts += [inter.reshape(-1), area_pred, area_gt]
            if ratio:
                if inst_band is None or inst_band.numel() < inst_map.numel():
                    inst_band = torch.empty(inst_map.numel(), dtype=torch.uint8, device=dev)
                inter_b, band_pred, band_gt = ops.mask_boundary_overlap(mask, inst_map, g, _eval.boundary_d(id, inst_map.shape, ratio),
                                                                        bad, inst_band)
                counts += [inter_b.reshape(-1), band_pred, band_gt]
            records.append({"pred_class": it["class"].numpy(), "pred_score": it["score"].numpy(),
                            "gt_class": it["inst_class"].numpy()})
        if not records:
            raise ValueError("eval_ins_seg: the split %s lists no images" % args.chainer_eval_set)
        _eval.raise_if_bad(bad, "eval_ins_seg", c)
        flat = torch.cat(counts).cpu().numpy()                 # every image's counts in one copy
    pos = 0
    for rec in records:
        n, g = len(rec["pred_class"]), len(rec["gt_class"])
        for key, shape in fields:
            size = {"ng": n * g, "n": n, "g": g}[shape]
            rec[key] = flat[pos:pos + size].reshape((n, g) if shape == "ng" else (size,))
            pos += size
    out = evaluation.instance_ap_voc(records, iou_thresh=0.5)
    print("0.5iou:", out)
    if ratio:
        b = evaluation.instance_ap_voc(records, iou_thresh=0.5, boundary=True)
        print("0.5biou:", b)
        out = dict(out, bap=b["ap"], bmap=b["map"])
    return out
