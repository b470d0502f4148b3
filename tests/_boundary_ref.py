"""Boundary IoU (Cheng et al., CVPR 2021) restated in plain loops: the contract of irn_label_band,
irn_label_boundary_counts and irn_mask_boundary_overlap (DESIGN.md "Boundary IoU").

    boundary_distance(h, w, ratio)   d = max(1, int(round(ratio * sqrt(h*h + w*w)))): Python doubles, Python's round
    band_at(L, d, y, x)              the definition for one pixel: the square window |dy| <= d, |dx| <= d around (y, x)
                                     leaves the image or holds a byte other than L[y, x]
    band(L, d)                       the same for every pixel, one loop over the (2d+1)^2 window offsets
    mask_band(m, d)                  a mask read as a two-valued map, the band kept where the mask is set
    semantic_counts(...)             counts [nc,3] = (inter, pband, gband) per class, and bad
    instance_counts(...)             inter_b [N,G], band_pred [N], band_gt [G], and bad
All 256 byte values are labels; no value stands for "outside" or "mixed"."""
import numpy as np


def boundary_distance(h, w, ratio):
    return max(1, int(round(ratio * (h * h + w * w) ** 0.5)))


def band_at(L, d, y, x):
    h, w = L.shape
    for dy in range(-d, d + 1):
        for dx in range(-d, d + 1):
            yy, xx = y + dy, x + dx
            if yy < 0 or yy >= h or xx < 0 or xx >= w or L[yy, xx] != L[y, x]:
                return 1
    return 0


def band(L, d):
    L = np.asarray(L, np.uint8)
    h, w = L.shape
    out = np.zeros((h, w), bool)
    for dy in range(-d, d + 1):
        y0, y1 = max(0, -dy), min(h, h - dy)              # the pixels whose neighbour at (dy, dx) is inside the image
        for dx in range(-d, d + 1):
            x0, x1 = max(0, -dx), min(w, w - dx)
            hit = np.ones((h, w), bool)                   # outside the image: band
            if y1 > y0 and x1 > x0:
                hit[y0:y1, x0:x1] = L[y0 + dy:y1 + dy, x0 + dx:x1 + dx] != L[y0:y1, x0:x1]
            out |= hit
    return out.astype(np.uint8)


def mask_band(m, d):
    m = np.asarray(m) != 0
    return band(m.astype(np.uint8), d) & m


def semantic_counts(pred, gt, d, nc, pred_255_as=0):
    """-> (counts int64 [nc,3], bad).  pred 255 reads as pred_255_as first (None: it stays 255, out of range)."""
    pred = np.asarray(pred, np.uint8).copy()
    gt = np.asarray(gt, np.uint8)
    if pred_255_as is not None:
        pred[pred == 255] = pred_255_as
    P, G = band(pred, d), band(gt, d)
    counts = np.zeros((nc, 3), np.int64)
    bad = 0
    h, w = gt.shape
    for y in range(h):
        for x in range(w):
            p, g = int(pred[y, x]), int(gt[y, x])
            if p >= nc or (g >= nc and g != 255):
                bad += 1
                continue
            if g == 255:
                continue
            if G[y, x]:
                counts[g, 2] += 1
            if P[y, x]:
                counts[p, 1] += 1
            if P[y, x] and G[y, x] and p == g:
                counts[g, 0] += 1
    return counts, bad


def instance_counts(masks, inst_map, n_inst, d):
    """-> (inter_b int64 [N,G], band_pred int64 [N], band_gt int64 [G], bad)."""
    masks = np.asarray(masks)
    inst_map = np.asarray(inst_map, np.uint8)
    n, g = len(masks), int(n_inst)
    gb = band(inst_map, d).astype(bool) & (inst_map != 0)
    inter_b = np.zeros((n, g), np.int64)
    band_pred = np.zeros(n, np.int64)
    band_gt = np.zeros(g, np.int64)
    for j in range(g):
        band_gt[j] = int((gb & (inst_map == j + 1)).sum())
    for i in range(n):
        mb = mask_band(masks[i], d).astype(bool)
        band_pred[i] = int(mb.sum())
        for j in range(g):
            inter_b[i, j] = int((mb & gb & (inst_map == j + 1)).sum())
    return inter_b, band_pred, band_gt, int((inst_map > g).sum())
