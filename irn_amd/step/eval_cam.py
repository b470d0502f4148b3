"""CAM evaluation step — drop-in for reference step/eval_cam.py (`run(args)`).

Reads  args.voc12_root (ImageSets/Segmentation/<args.chainer_eval_set>.txt, SegmentationClass/<id>.png),
       args.cam_out_dir/<id>.npy (`high_res` / `keys` of make_cam), args.cam_eval_thres, args.cam_eval_thres_sweep
Prints {'iou': ..., 'miou': ...} at args.cam_eval_thres as the reference does, then with a sweep one line per threshold
       and the best one; returns the printed dict (+ 'sweep' {thres: miou} and 'best_thres' with a sweep).

Per image, the prediction at threshold t is keys_pad[argmax([t, high_res])] (step/eval_cam.py:14-19).  Every threshold
is counted in the same pass over the CAM (`ops.cam_confusion`: one histogram of (GT, arg-max class, number of thresholds
below the maximum) per image, accumulated on the device).
"""
import os

import numpy as np
import torch

from .. import ops
from ..misc import evaluation
from ..voc12 import eval_data
from . import _classes, _eval


def _thresholds(args):
    req = [float(args.cam_eval_thres)] + [float(t) for t in (getattr(args, "cam_eval_thres_sweep", None) or ())]
    th32 = np.unique(np.asarray(req, np.float32))           # np.pad casts the threshold to the CAM's float32
    return req, th32


def run(args):
    ids = eval_data.seg_ids(args.voc12_root, args.chainer_eval_set)
    req, th32 = _thresholds(args)
    dev = _eval.device()
    c = _classes.num_classes(args)

    def load(id):
        gt = eval_data.class_label(args.voc12_root, id)
        cam = np.load(os.path.join(args.cam_out_dir, id + ".npy"), allow_pickle=True).item()
        keys = np.asarray(cam["keys"], np.int64).reshape(-1)
        if keys.size:
            high_res = np.ascontiguousarray(cam["high_res"], np.float32)
            _eval.check_shape(id, "high_res", high_res.shape, (keys.size,) + gt.shape)
        else:
            high_res = np.zeros((0,) + gt.shape, np.float32)
        return {"gt": gt, "high_res": high_res, "keys": keys}

    with torch.cuda.device(dev):
        th = torch.from_numpy(th32).to(dev)
        hist = bad = None
        for id, it in _eval.items(ids, load, args):
            hist, bad = ops.cam_confusion(it["high_res"].to(dev, non_blocking=True), it["keys"].to(dev),
                                          it["gt"].to(dev, non_blocking=True), th, hist, bad, n_classes=c + 1)
        if hist is None:
            raise ValueError("eval_cam: the split %s lists no images" % args.chainer_eval_set)
        conf, void = ops.cam_confusion_matrices(hist, n_classes=c + 1)
        _eval.raise_if_bad(bad, "eval_cam", c)
        conf, void = conf.cpu().numpy(), void.cpu().numpy()

    mious = {}
    results = {}
    for i, t in enumerate(th32):
        _, iou = evaluation.iou_from_confusion(conf[i], void[i])
        results[float(t)] = {"iou": iou, "miou": evaluation.nanmean(iou)}
    out = dict(results[float(np.float32(req[0]))])
    print(out)
    if len(req) > 1:
        for t in req:
            mious[t] = results[float(np.float32(t))]["miou"]
            print("thres %g miou %.6f" % (t, mious[t]))
        best = max(mious, key=lambda t: (mious[t], -t))
        print("best thres %g miou %.6f" % (best, mious[best]))
        out["sweep"] = mious
        out["best_thres"] = best
    return out
