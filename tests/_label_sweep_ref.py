"""Numpy restatement of irn_label_sweep_confusion (irn_amd/csrc/label.hip): per output pixel the pair (first arg-max
channel c*, its normalised score m) and the NaN rule, from the oracle's own upsample and division; the histogram
[22][21][T+1] they are counted into; and its reduction to T confusion matrices as `k_cam_reduce` (eval.hip) does it.
Shared by tests/test_label_sweep_cpu.py (which proves it against the oracle's epilogue + the chainercv confusion) and
tests/test_gpu_label_sweep.py (which holds the kernel to it).  Plain numpy, deterministic by seed."""
import numpy as np

from oracle import irn_oracle as O

F32 = np.float32
NC = 21


def pixel_pairs(rw, out_hw):
    """-> (c* int [H,W], m float32 [H,W], nan bool [H,W]): `nan` where some channel's score is NaN (c* is then the first
    such channel), else c* = the first channel that reaches the maximum m."""
    up = O.upsample_bilinear(rw, 4, out_hw)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = up / up.max()                                   # oracle.sem_seg_epilogue's division
    isnan = np.isnan(v)
    nan = isnan.any(axis=0)
    first_nan = np.argmax(isnan, axis=0)
    safe = np.where(isnan, F32(-np.inf), v)
    cstar = np.argmax(safe, axis=0)                         # first maximum
    m = np.take_along_axis(v, cstar[None], axis=0)[0]
    return np.where(nan, first_nan, cstar), m.astype(F32), nan


def histogram(rw, out_hw, keys, gt, thres):
    """-> (hist int64 [22,21,T+1], bad int): GT 21..254 and pixels whose c* has a key outside 0..19 are skipped and counted;
    every NaN threshold and every descending neighbour pair counts once."""
    th = np.asarray(thres, F32).reshape(-1)
    t = th.size
    keys = np.asarray(keys, np.int64).reshape(-1)
    cstar, m, nan = pixel_pairs(rw, out_hw)
    hist = np.zeros((NC + 1, NC, t + 1), np.int64)
    bad = int(np.isnan(th).sum() + sum(1 for i in range(1, t) if not th[i - 1] <= th[i]))
    j = np.where(nan, t, np.searchsorted(th, m, side="left"))            # number of thresholds < m
    gt = np.asarray(gt, np.uint8)
    row = np.where(gt <= 20, gt.astype(np.int64), np.where(gt == 255, NC, -1))
    col = keys[cstar] + 1
    ok = (row >= 0) & (col >= 1) & (col <= 20)
    bad += int((~ok).sum())
    np.add.at(hist, (row[ok], col[ok], j[ok]), 1)
    return hist, bad


def reduce(hist):
    """hist [22,21,T+1] -> (conf int64 [T,21,21], void int64 [T,21]): a pixel of column c >= 1 and count j predicts c at
    thresholds 0..j-1 and 0 from j on."""
    t = hist.shape[2] - 1
    conf = np.zeros((t, NC, NC), np.int64)
    void = np.zeros((t, NC), np.int64)
    for i in range(t):
        above = hist[:, :, i + 1:].sum(axis=2)              # maximum above thres[i]
        below = hist[:, :, :i + 1].sum(axis=2)
        full = above.copy()
        full[:, 0] = hist[:, 0].sum(axis=1) + below[:, 1:].sum(axis=1)
        conf[i], void[i] = full[:NC], full[NC]
    return conf, void


def ground_truth(out_hw, seed):
    """uint8 [H,W] with every value of 0..20 and 255 wherever the map has room for them (blocks, so that classes meet the
    label regions), deterministic by seed."""
    rng = np.random.RandomState(seed)
    h, w = out_hw
    vals = np.concatenate([np.arange(21), [255]]).astype(np.uint8)
    coarse = vals[rng.randint(0, 22, ((h + 3) // 4, (w + 5) // 6))]
    gt = np.repeat(np.repeat(coarse, 4, axis=0), 6, axis=1)[:h, :w].copy()
    flat = gt.reshape(-1)
    pos = rng.permutation(flat.size)[:22]
    flat[pos] = vals[:pos.size]
    return gt


def thresholds(rw, out_hw, t, seed):
    """t ascending float32 thresholds: the EXACT scores of several pixels (so `thres == m` happens), then 0.25, a negative
    value and one above 1, then seeded values in (0, 1.2) up to t."""
    rng = np.random.RandomState(seed)
    _, m, nan = pixel_pairs(rw, out_hw)
    scores = np.unique(m[~nan & np.isfinite(m)])
    picks = list(scores[rng.permutation(scores.size)[:4]]) if scores.size else []
    out = []
    for v in picks[:1] + [F32(0.25), F32(-0.5), F32(1.5)] + picks[1:]:
        if len(out) < t and F32(v) not in out:
            out.append(F32(v))
    while len(out) < t:
        v = F32(rng.uniform(0.0, 1.2))
        if v not in out:
            out.append(v)
    return np.sort(np.asarray(out, F32))
