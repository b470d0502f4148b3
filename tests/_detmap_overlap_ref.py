"""numpy restatement of detect_instance (reference step/make_ins_seg_labels.py:82-105) followed by the mask_iou counts of
step/eval_ins_seg.py, for the tests of ops.detection_overlap_batch: 4-connected components per channel in skimage's label
order (raster order of each component's first pixel), channel ascending, then the pixel counts against a GT instance map."""
import numpy as np


def label4(mask):
    """int32 labels of the 4-connected components of a bool [H,W] mask, numbered from 1 by first pixel in raster order."""
    h, w = mask.shape
    lab = np.zeros((h, w), np.int32)
    n = 0
    for y0, x0 in zip(*np.nonzero(mask)):
        if lab[y0, x0]:
            continue
        n += 1
        lab[y0, x0] = n
        stack = [(y0, x0)]
        while stack:
            y, x = stack.pop()
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < h and 0 <= xx < w and mask[yy, xx] and not lab[yy, xx]:
                    lab[yy, xx] = n
                    stack.append((yy, xx))
    return lab, n


def detections(rw_up, argmax, n_channels, min_area):
    """-> (score f32 [N], channel i32 [N], masks bool [N,H,W]) in detect_instance's order."""
    score, channel, masks = [], [], []
    for c in range(n_channels):
        lab, n = label4(argmax == c + 1)
        for k in range(1, n + 1):
            m = lab == k
            s = np.float32(0) if m.sum() < min_area else max(np.float32(0), np.max(rw_up[c] * m))
            score.append(s); channel.append(c); masks.append(m)
    h, w = argmax.shape
    return (np.asarray(score, np.float32), np.asarray(channel, np.int32),
            np.stack(masks) if masks else np.zeros((0, h, w), bool))


def overlap(rw_up, argmax, n_channels, min_area, inst, g):
    """-> the record of ops.detection_overlap_batch (with `channel` in place of `pred_class`) and the count of bad GT ids."""
    score, channel, masks = detections(rw_up, argmax, n_channels, min_area)
    # |mask & (inst == j + 1)| for j < g: the GT ids under each mask, counted
    inter = np.zeros((len(masks), g), np.int64)
    for d, m in enumerate(masks):
        inter[d] = np.bincount(inst[m], minlength=256)[1:g + 1]
    rec = {"channel": channel, "pred_score": score, "inter": inter, "area_pred": masks.sum(axis=(1, 2)).astype(np.int64),
           "area_gt": np.bincount(inst.reshape(-1), minlength=256)[1:g + 1].astype(np.int64)}
    return rec, int((inst > g).sum())
