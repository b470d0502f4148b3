"""numpy restatement of "all run-length codes from one id map": what the rle_* kernels of irn_amd/csrc/instance.hip
compute for the detections of one image.  Test infrastructure; nothing here is shared with irn_amd/instance.py.

The masks of an image's detections are disjoint, so one int map (`idmap[y, x]` = detection 0..n-1 of the pixel, -1 =
background) holds all of them.  In pycocotools' column-major order j = x*h + y, a pixel whose id differs from its
predecessor's (the first pixel follows the background) is an event: it ends a run of ones of the predecessor's detection
and starts one of its own.  Every event becomes the key (id << 32 | j), every detection adds the key of the map's end
(id << 32 | h*w), the keys are sorted, and the run lengths of a detection are the differences of its neighbouring
positions, the first taken from 0."""
import numpy as np


def rle_from_idmap(idmap, n):
    """-> (counts uint32 [total], offsets int64 [n+1], area int64 [n], bbox int32 [n,4]) — what `_cocomask_ref.mask_rle`
    gives for the n one-hot planes `idmap == d`.  Every id 0..n-1 must occur."""
    idmap = np.asarray(idmap).astype(np.int64)
    h, w = idmap.shape
    flat = idmap.T.reshape(-1)                                   # j = x*h + y
    prev = np.concatenate([[-1], flat[:-1]])
    pos = np.flatnonzero(flat != prev)
    a, b = prev[pos], flat[pos]
    keys = np.concatenate([(a[a >= 0] << 32) | pos[a >= 0],      # the runs that end here ...
                           (b[b >= 0] << 32) | pos[b >= 0],      # ... and the ones that start
                           (np.arange(n, dtype=np.int64) << 32) | (h * w)])
    keys.sort()
    ids, at = keys >> 32, keys & 0xffffffff
    first = np.concatenate([[True], ids[1:] != ids[:-1]]) if len(keys) else np.zeros(0, bool)
    before = np.concatenate([[0], at[:-1]]) if len(keys) else np.zeros(0, np.int64)
    counts = (at - np.where(first, 0, before)).astype(np.uint32)
    n_runs = np.bincount(ids, minlength=n) if len(keys) else np.zeros(n, np.int64)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(n_runs, out=offsets[1:])
    area, bbox = np.zeros(n, np.int64), np.zeros((n, 4), np.int32)
    ys, xs = np.nonzero(idmap >= 0)
    d = idmap[ys, xs]
    np.add.at(area, d, 1)
    x0, y0 = np.full(n, w), np.full(n, h)
    x1, y1 = np.full(n, -1), np.full(n, -1)
    np.minimum.at(x0, d, xs), np.maximum.at(x1, d, xs), np.minimum.at(y0, d, ys), np.maximum.at(y1, d, ys)
    bbox[:] = np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1], 1)
    return counts, offsets, area, bbox
