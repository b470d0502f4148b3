"""Tuning step (not in the reference): score a grid of --conf_fg_thres x --conf_bg_thres against the ground truth in ONE
pass over the split — what cam_to_ir_label and a count of its PNGs give per grid point, without a label file.

Reads  args.voc12_root (ImageSets/Segmentation/<args.chainer_eval_set>.txt, JPEGImages/<id>.jpg, SegmentationClass/<id>.png),
       args.cam_out_dir/<id>.npy (`high_res` / `keys` of make_cam),
       args.conf_fg_thres, args.conf_bg_thres (the configured point: always on the grid),
       args.tune_conf_fg_thres, args.tune_conf_bg_thres (more values per axis)
Prints the configured point's {'iou', 'miou', 'coverage', 'miou_all'}, one `fg .. bg .. miou .. coverage .. miou_all ..` line
       per grid point and the best one (highest miou_all); returns the configured point's dict + 'grid' {(fg, bg): miou_all},
       'scores' {(fg, bg): dict of evaluation.ir_label_scores}, 'hist' (numpy int64 [F,B,22,22]; [F,B,C+2,C+2] with --num_classes C) and 'best'.  Writes nothing.

IR labels are mined on args.train_list, but ground truth exists only for the segmentation split, so the ids of
args.chainer_eval_set are scored (eval_cam makes the same choice).  The IR label of a pixel is fg if fg != 0, else 0 if bg == 0,
else 255, where fg / bg are the CRF label maps seeded at the two thresholds (step/cam_to_ir_label.py:26-39), and a CRF label
map depends on ONE threshold only: an F x B grid needs the CRF at the T distinct thresholds of both axes, not 2*F*B of them,
and all T share the image's two lattices.  Per image `ops.crf_label_sweep` runs them (chunks of one filter each) and
`ops.ir_label_confusion` counts every pair from the T planes; the histogram stays on the device and comes back once
(DESIGN.md §23).  A plane is bit-equal to what `ops.crf_ir_label` computes for that threshold, so a grid point's counts are
those of the PNGs cam_to_ir_label would write there.  An image without class keys contributes its all-zero map, as
cam_to_ir_label writes it.  Runs in the calling process on its current device like the evaluation steps (step/_eval.py).
The axis rules, the tie-breaking of `best` and the split reader are step/_tune.py's, shared with the walk tuners."""
import functools
import os

import numpy as np
import torch

from .. import ops
from ..misc import evaluation
from ..voc12 import eval_data
from . import _classes, _eval, _io, _tune

MAX_AXIS = 16                         # values per axis (irn_ir_label_confusion)
MAX_THRES = ops.CRF_MAX_SWEEP         # distinct thresholds over both axes together: CRFs per image
# ties go to the smaller fg, then the smaller bg
pick_best = functools.partial(_tune.pick_best, tie_order=(0, 1))


def grid_axes(args):
    """-> (fg values as requested, bg values as requested, all distinct thresholds ascending float32, fg plane numbers, bg
    plane numbers): each axis is a `_tune.threshold_axis` that holds its configured value."""
    (fgs, fg32), (bgs, bg32) = (
        _tune.threshold_axis(getattr(args, "conf_%s_thres" % a), getattr(args, "tune_conf_%s_thres" % a, None), what, MAX_AXIS,
                             "tune_ir_label") for a, what in (("fg", "foreground"), ("bg", "background")))
    th32 = np.unique(np.concatenate([fg32, bg32]))
    if th32.size > MAX_THRES:
        raise ValueError("tune_ir_label: %d distinct thresholds over both axes (at most %d: each is one CRF per image)"
                         % (th32.size, MAX_THRES))
    return fgs, bgs, th32, np.searchsorted(th32, fg32).astype(np.int32), np.searchsorted(th32, bg32).astype(np.int32)


def report(hist, fgs, bgs, configured):
    """Scores of every grid point from hist int64 [F,B,nc+1,nc+1], printed in the step's format; returns the step's dict."""
    scores = {(fg, bg): evaluation.ir_label_scores(hist[i, j]) for i, fg in enumerate(fgs) for j, bg in enumerate(bgs)}
    grid = {point: s["miou_all"] for point, s in scores.items()}
    here = scores[configured]
    out = {k: here[k] for k in ("iou", "miou", "coverage", "miou_all")}
    print(out)
    for (fg, bg), s in scores.items():
        print("fg %g bg %g miou %.6f coverage %.6f miou_all %.6f" % (fg, bg, s["miou"], s["coverage"], s["miou_all"]))
    best = pick_best(grid)
    s = scores[best]
    print("best fg %g bg %g miou %.6f coverage %.6f miou_all %.6f" % (best + (s["miou"], s["coverage"], s["miou_all"])))
    out.update(grid=grid, scores=scores, hist=hist, best=best)
    return out


def run(args):
    fgs, bgs, th32, fg_idx, bg_idx = grid_axes(args)          # refusals before any image is read
    configured = (_tune.configured(fgs, th32[fg_idx], args.conf_fg_thres), _tune.configured(bgs, th32[bg_idx], args.conf_bg_thres))
    ids = _tune.split_ids(args)
    _tune.refuse_empty(ids, args, "tune_ir_label")
    dev = _eval.device()
    c = _classes.num_classes(args)

    def load(id):
        gt = eval_data.class_label(args.voc12_root, id)
        img = _tune.jpeg(args, id, gt.shape)
        cam = np.load(os.path.join(args.cam_out_dir, id + ".npy"), allow_pickle=True).item()
        keys = np.asarray(cam["keys"], np.int64).reshape(-1)
        if keys.size:
            high_res = np.ascontiguousarray(cam["high_res"], np.float32)
            _eval.check_shape(id, "high_res", high_res.shape, (keys.size,) + gt.shape)
        else:
            high_res = np.zeros((0,) + gt.shape, np.float32)
        return {"gt": gt, "image": img, "high_res": high_res, "keys": keys}

    with torch.cuda.device(dev):
        hist = bad = None
        for id, it in _eval.items(ids, load, args):
            planes = ops.crf_label_sweep(_io.upload(it["image"]), _io.upload(it["high_res"]), _io.upload(it["keys"]), th32)
            hist, bad = ops.ir_label_confusion(planes, fg_idx, bg_idx, _io.upload(it["gt"]), hist, bad, n_classes=c + 1)
        _eval.raise_if_bad(bad, "tune_ir_label", c)
        hist = hist.cpu().numpy()
    return report(hist, fgs, bgs, configured)
