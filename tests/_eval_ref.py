"""Numpy restatement of the chainercv 0.13 evaluation functions the reference's eval steps call, mask by mask and pixel by
pixel, with no counting shortcuts: the independent check of irn_amd/misc/evaluation.py and the counting kernels.

    calc_semantic_segmentation_confusion(preds, gts)     (gts with void = -1)
    mask_iou(a, b)
    calc_instance_segmentation_voc_prec_rec(...), calc_detection_voc_ap(prec, rec), eval_instance_segmentation_voc(...)
    eval_cam / eval_sem_seg / eval_ins_seg: the reference's step/eval_*.py bodies over a VOC-layout directory
"""
import os
from collections import defaultdict

import numpy as np
from PIL import Image


def calc_semantic_segmentation_confusion(preds, gts):
    n_class = 0
    confusion = np.zeros((n_class, n_class), dtype=np.int64)
    for pred_label, gt_label in zip(preds, gts):
        if pred_label.ndim != 2 or gt_label.ndim != 2 or pred_label.shape != gt_label.shape:
            raise ValueError("shape mismatch")
        pred_label = pred_label.astype(np.int64).ravel()
        gt_label = gt_label.astype(np.int64).ravel()
        lb_max = np.max((pred_label, gt_label))
        if lb_max >= n_class:
            expanded = np.zeros((lb_max + 1, lb_max + 1), dtype=np.int64)
            expanded[0:n_class, 0:n_class] = confusion
            n_class = lb_max + 1
            confusion = expanded
        mask = gt_label >= 0
        confusion += np.bincount(n_class * gt_label[mask] + pred_label[mask],
                                 minlength=n_class ** 2).reshape((n_class, n_class))
    return confusion


def iou_of(confusion):
    gtj = confusion.sum(axis=1)
    resj = confusion.sum(axis=0)
    gtjresj = np.diag(confusion)
    with np.errstate(divide="ignore", invalid="ignore"):
        return gtjresj / (gtj + resj - gtjresj)


def nanmean(a):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(a)


def mask_iou(mask_a, mask_b):
    iou = np.empty((len(mask_a), len(mask_b)), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for n, m_a in enumerate(mask_a):
            for k, m_b in enumerate(mask_b):
                intersect = np.bitwise_and(m_a, m_b).sum()
                union = np.bitwise_or(m_a, m_b).sum()
                iou[n, k] = intersect / union
    return iou


def calc_instance_segmentation_voc_prec_rec(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, iou_thresh=0.5):
    n_pos = defaultdict(int)
    score = defaultdict(list)
    match = defaultdict(list)
    for pred_mask, pred_label, pred_score, gt_mask, gt_label in zip(pred_masks, pred_labels, pred_scores, gt_masks,
                                                                    gt_labels):
        for l in np.unique(np.concatenate((pred_label, gt_label)).astype(int)):
            pred_keep_l = pred_label == l
            pred_mask_l = pred_mask[pred_keep_l]
            pred_score_l = pred_score[pred_keep_l]
            order = pred_score_l.argsort()[::-1]
            pred_mask_l = pred_mask_l[order]
            pred_score_l = pred_score_l[order]
            gt_keep_l = gt_label == l
            gt_mask_l = gt_mask[gt_keep_l]
            n_pos[l] += gt_keep_l.sum()
            score[l].extend(pred_score_l)
            if len(pred_mask_l) == 0:
                continue
            if len(gt_mask_l) == 0:
                match[l].extend((0,) * pred_mask_l.shape[0])
                continue
            iou = mask_iou(pred_mask_l, gt_mask_l)
            gt_index = iou.argmax(axis=1)
            gt_index[iou.max(axis=1) < iou_thresh] = -1
            del iou
            selec = np.zeros(gt_mask_l.shape[0], dtype=bool)
            for gt_idx in gt_index:
                if gt_idx >= 0:
                    if not selec[gt_idx]:
                        match[l].append(1)
                    else:
                        match[l].append(0)
                    selec[gt_idx] = True
                else:
                    match[l].append(0)
    n_fg_class = max(n_pos.keys()) + 1
    prec = [None] * n_fg_class
    rec = [None] * n_fg_class
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
            rec[l] = tp / n_pos[l]
    return prec, rec


def calc_detection_voc_ap(prec, rec):
    n_fg_class = len(prec)
    ap = np.empty(n_fg_class)
    for l in range(n_fg_class):
        if prec[l] is None or rec[l] is None:
            ap[l] = np.nan
            continue
        mpre = np.concatenate(([0], np.nan_to_num(prec[l]), [0]))
        mrec = np.concatenate(([0], rec[l], [1]))
        mpre = np.maximum.accumulate(mpre[::-1])[::-1]
        i = np.where(mrec[1:] != mrec[:-1])[0]
        ap[l] = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return ap


def eval_instance_segmentation_voc(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, iou_thresh=0.5):
    prec, rec = calc_instance_segmentation_voc_prec_rec(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels,
                                                        iou_thresh)
    ap = calc_detection_voc_ap(prec, rec)
    return {"ap": ap, "map": nanmean(ap)}


# ---------------------------------------------------------------------------------------------------------------------
# the reference steps over a VOC-layout directory
# ---------------------------------------------------------------------------------------------------------------------
def ids_of(root, split):
    with open(os.path.join(root, "ImageSets", "Segmentation", split + ".txt")) as f:
        return [line.strip() for line in f if line.strip()]


def read_label(root, id):
    lab = np.asarray(Image.open(os.path.join(root, "SegmentationClass", id + ".png"))).astype(np.int32)
    lab[lab == 255] = -1
    return lab


def read_instances(root, id):
    """image_wise_to_instance_wise: (masks bool [G,H,W], labels int32 [G]); the class of an instance is taken from the
    uint8 class map (void = 255), as the issue of this step specifies."""
    cls = np.asarray(Image.open(os.path.join(root, "SegmentationClass", id + ".png")))
    inst = np.asarray(Image.open(os.path.join(root, "SegmentationObject", id + ".png"))).astype(np.int32)
    inst[inst == 0] = -1
    inst[inst == 255] = -1
    masks, labels = [], []
    ids = np.unique(inst)
    for inst_id in ids[ids != -1]:
        msk = inst == inst_id
        lbl = int(np.unique(cls[msk])[0]) - 1
        assert lbl != -1
        masks.append(msk)
        labels.append(lbl)
    h, w = cls.shape
    return (np.array(masks, bool).reshape(-1, h, w), np.array(labels, np.int32))


def eval_cam(root, split, cam_dir, thres):
    labels = [read_label(root, id) for id in ids_of(root, split)]
    preds = []
    for id in ids_of(root, split):
        cam_dict = np.load(os.path.join(cam_dir, id + ".npy"), allow_pickle=True).item()
        cams = cam_dict["high_res"]
        cams = np.pad(cams, ((1, 0), (0, 0), (0, 0)), mode="constant", constant_values=thres)
        keys = np.pad(cam_dict["keys"] + 1, (1, 0), mode="constant")
        cls_labels = np.argmax(cams, axis=0)
        cls_labels = keys[cls_labels]
        preds.append(cls_labels.copy())
    confusion = calc_semantic_segmentation_confusion(preds, labels)
    iou = iou_of(confusion)
    return {"iou": iou, "miou": nanmean(iou)}


def eval_sem_seg(root, split, sem_dir):
    labels = [read_label(root, id) for id in ids_of(root, split)]
    preds = []
    for id in ids_of(root, split):
        cls_labels = np.asarray(Image.open(os.path.join(sem_dir, id + ".png"))).astype(np.uint8).copy()
        cls_labels[cls_labels == 255] = 0
        preds.append(cls_labels)
    confusion = calc_semantic_segmentation_confusion(preds, labels)[:21, :21]
    gtj = confusion.sum(axis=1)
    resj = confusion.sum(axis=0)
    gtjresj = np.diag(confusion)
    denominator = gtj + resj - gtjresj
    with np.errstate(divide="ignore", invalid="ignore"):
        fp = 1. - gtj / denominator
        fn = 1. - resj / denominator
        iou = gtjresj / denominator
    return {"iou": iou, "miou": nanmean(iou)}, fp, fn


def eval_ins_seg(root, split, ins_dir):
    gts = [read_instances(root, id) for id in ids_of(root, split)]
    pred_class, pred_mask, pred_score = [], [], []
    for id in ids_of(root, split):
        ins_out = np.load(os.path.join(ins_dir, id + ".npy"), allow_pickle=True).item()
        pred_class.append(ins_out["class"])
        pred_mask.append(ins_out["mask"])
        pred_score.append(ins_out["score"])
    return eval_instance_segmentation_voc(pred_mask, pred_class, pred_score, [g[0] for g in gts], [g[1] for g in gts],
                                          iou_thresh=0.5)


from irn_amd.synth import save_palette_png as save_p_png  # noqa: E402,F401  (the fixtures' writer, not a restatement)
