"""Host side of the evaluation steps: chainercv's scores from the integer counts the GPU returns (irn_amd/eval_counts.py
cam_confusion / label_confusion / mask_overlap).

    observed_classes(conf, void)      the size chainercv's growing confusion matrix reaches
    iou_from_confusion(conf, void)    calc_semantic_segmentation_confusion + the iou of step/eval_cam.py:22-28
    sem_seg_scores(conf, void)        step/eval_sem_seg.py:19-31 (fp / fn / iou of the [:nc, :nc] matrix; the reference has nc = 21)
    ir_label_scores(hist)             step/tune_ir_label.py: accuracy, coverage and all-pixel iou of one IR-label grid point
    instance_ap_voc(records)          eval_instance_segmentation_voc(iou_thresh=0.5): calc_instance_segmentation_voc_prec_rec
                                      + calc_detection_voc_ap(use_07_metric=False), from per-image overlap counts; with
                                      boundary=True matched on min(mask IoU, boundary IoU): Boundary AP (not in the reference)
    boundary_iou_scores(counts)       Boundary IoU per class from the band counts of ops.label_boundary_counts (not in the reference)

Everything here is numpy in the order of operations chainercv uses, so the floats equal what it computes from the masks.
"""
import warnings
from collections import defaultdict

import numpy as np


def observed_classes(conf, void=None):
    """1 + the largest label chainercv sees: it grows its matrix to max(pred.max(), gt.max()) + 1 per image, and the
    prediction at a void GT pixel counts for that maximum though not for the matrix.  conf [C,C] (row = GT), void [C]."""
    conf = np.asarray(conf)
    seen = np.flatnonzero(conf.sum(axis=1) + conf.sum(axis=0) + (0 if void is None else np.asarray(void)))
    return int(seen[-1]) + 1 if seen.size else 0


def iou_from_confusion(conf, void=None):
    """(confusion int64 [n,n], iou float64 [n]) with n = observed_classes(conf, void), as step/eval_cam.py computes them:
    iou = diag / (row sums + column sums - diag) (nan for a class that occurs nowhere in the trimmed range)."""
    n = observed_classes(conf, void)
    conf = np.asarray(conf, np.int64)[:n, :n]
    gtj = conf.sum(axis=1)
    resj = conf.sum(axis=0)
    gtjresj = np.diag(conf)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = gtjresj / (gtj + resj - gtjresj)
    return conf, iou


def sem_seg_scores(conf, void=None):
    """step/eval_sem_seg.py:19-29 on the [:nc, :nc] matrix -> dict fp, fn, iou (float64 arrays) and the matrix.  nc is the
    size of the matrix given (the class count it was counted with, background included; 21 in the reference)."""
    nc = np.asarray(conf).shape[0]
    conf, _ = iou_from_confusion(conf, void)
    conf = conf[:nc, :nc]
    gtj = conf.sum(axis=1)
    resj = conf.sum(axis=0)
    gtjresj = np.diag(conf)
    denominator = gtj + resj - gtjresj
    with np.errstate(divide="ignore", invalid="ignore"):
        fp = 1. - gtj / denominator
        fn = 1. - resj / denominator
        iou = gtjresj / denominator
    return {"fp": fp, "fn": fn, "iou": iou, "confusion": conf}


def ir_label_scores(hist):
    """Scores of one (fg, bg) point of step/tune_ir_label.py from hist int64 [nc+1,nc+1] of ops.ir_label_confusion (row =
    GT, nc = void; column = IR label, nc = 255 unsure; nc = 21 by default, taken from the histogram's size) -> dict
      iou, miou     sem_seg_scores of the [:nc, :nc] matrix: the accuracy on the confident pixels
      coverage      the share of the non-void pixels that get a label
      iou_all, miou_all   per class diag / (GT pixels, unsure ones included, + labelled pixels - diag): unsure pixels count
                    as misses."""
    hist = np.asarray(hist, np.int64)
    nc = hist.shape[0] - 1
    conf, void = hist[:nc, :nc], hist[nc, :nc]
    s = sem_seg_scores(conf, void)
    diag = np.diag(conf)
    with np.errstate(divide="ignore", invalid="ignore"):
        coverage = conf.sum() / hist[:nc, :].sum()
        iou_all = diag / (hist[:nc, :].sum(axis=1) + conf.sum(axis=0) - diag)
    return {"iou": s["iou"], "miou": nanmean(s["iou"]), "coverage": float(coverage), "iou_all": iou_all,
            "miou_all": nanmean(iou_all)}


def mask_iou_from_counts(inter, area_a, area_b):
    """chainercv's mask_iou from counts: |a & b| / |a | b| with |a | b| = |a| + |b| - |a & b|, divided in float64 and stored
    into a float32 array as mask_iou stores it."""
    inter = np.asarray(inter, np.int64)
    union = np.asarray(area_a, np.int64)[:, None] + np.asarray(area_b, np.int64)[None, :] - inter
    iou = np.empty(inter.shape, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou[...] = inter / union
    return iou


def boundary_iou_scores(counts):
    """Boundary IoU (Cheng et al., CVPR 2021) from counts int64 [nc,3] of ops.label_boundary_counts summed over a split
    (per class: both bands and the same class, prediction band, GT band) -> {'biou': float64 [nc], 'mbiou'}:
    biou = inter / (pband + gband - inter), nan for a class with no band pixel in either map; mbiou = nanmean."""
    counts = np.asarray(counts, np.int64)
    inter, pband, gband = counts[:, 0], counts[:, 1], counts[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        biou = inter / (pband + gband - inter)
    return {"biou": biou, "mbiou": nanmean(biou)}


def instance_ap_voc(records, iou_thresh=0.5, boundary=False):
    """eval_instance_segmentation_voc(..., iou_thresh, use_07_metric=False) from counts -> {'ap': float64 [n_fg], 'map'}.

    records: one dict per image, in the split's order (the argsort tie order depends on it), with
      'pred_class' int [N], 'pred_score' [N] (as the detection file holds it), 'gt_class' int [G],
      'inter' int [N,G], 'area_pred' int [N], 'area_gt' int [G]  (ops.mask_overlap).
    boundary: Boundary AP — a detection is matched on np.minimum(mask IoU, boundary IoU), the second from the records'
      'inter_b' int [N,G], 'band_pred' int [N], 'band_gt' int [G]  (ops.mask_boundary_overlap); nothing else changes."""
    n_pos = defaultdict(int)
    score = defaultdict(list)
    match = defaultdict(list)
    for rec in records:
        pred_label = np.asarray(rec["pred_class"])
        pred_score = np.asarray(rec["pred_score"])
        gt_label = np.asarray(rec["gt_class"])
        inter = np.asarray(rec["inter"], np.int64).reshape(len(pred_label), len(gt_label))
        area_pred = np.asarray(rec["area_pred"], np.int64)
        area_gt = np.asarray(rec["area_gt"], np.int64)
        if boundary:
            inter_b = np.asarray(rec["inter_b"], np.int64).reshape(len(pred_label), len(gt_label))
            band_pred = np.asarray(rec["band_pred"], np.int64)
            band_gt = np.asarray(rec["band_gt"], np.int64)
        for l in np.unique(np.concatenate((pred_label, gt_label)).astype(int)):
            keep = np.flatnonzero(pred_label == l)
            ps = pred_score[keep]
            order = ps.argsort()[::-1]
            keep, ps = keep[order], ps[order]
            gsel = np.flatnonzero(gt_label == l)
            n_pos[l] += len(gsel)
            score[l].extend(ps)
            if len(keep) == 0:
                continue
            if len(gsel) == 0:
                match[l].extend((0,) * len(keep))
                continue
            iou = mask_iou_from_counts(inter[np.ix_(keep, gsel)], area_pred[keep], area_gt[gsel])
            if boundary:
                iou = np.minimum(iou, mask_iou_from_counts(inter_b[np.ix_(keep, gsel)], band_pred[keep], band_gt[gsel]))
            gt_index = iou.argmax(axis=1)
            gt_index[iou.max(axis=1) < iou_thresh] = -1
            del iou
            selec = np.zeros(len(gsel), dtype=bool)
            for gt_idx in gt_index:
                if gt_idx >= 0:
                    match[l].append(0 if selec[gt_idx] else 1)
                    selec[gt_idx] = True
                else:
                    match[l].append(0)

    n_fg_class = max(n_pos.keys()) + 1
    prec = [None] * n_fg_class
    rec_ = [None] * n_fg_class
    for l in n_pos.keys():
        score_l = np.array(score[l])
        match_l = np.array(match[l], dtype=np.int8)
        order = score_l.argsort()[::-1]
        match_l = match_l[order]
        tp = np.cumsum(match_l == 1)
        fp = np.cumsum(match_l == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            prec[l] = tp / (fp + tp)
        if n_pos[l] > 0:
            rec_[l] = tp / n_pos[l]

    ap = np.empty(n_fg_class)
    for l in range(n_fg_class):
        if prec[l] is None or rec_[l] is None:
            ap[l] = np.nan
            continue
        mpre = np.concatenate(([0], np.nan_to_num(prec[l]), [0]))
        mrec = np.concatenate(([0], rec_[l], [1]))
        mpre = np.maximum.accumulate(mpre[::-1])[::-1]
        i = np.where(mrec[1:] != mrec[:-1])[0]
        ap[l] = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return {"ap": ap, "map": nanmean(ap)}


def mean(a):
    """np.mean without its warning for an empty array (the value, nan, is the same)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.mean(a)


def nanmean(a):
    """np.nanmean without its warning for an all-nan array (the value, nan, is the same)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(a)
