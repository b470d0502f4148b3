"""Yardstick of the (image, label) training-input pipeline of the IRNet step (irn_amd/csrc/augment.hip's label kernel,
ops.nearest_plan / augment_label_tables / augment_pair_batch): the host pipeline of `VOC12AffinityDataset.__getitem__` for
EXPLICIT draws (hs, ws, flip, box) — `imutils.pil_resize` with Pillow's NEAREST, fliplr, the box into a container of 255,
`pil_rescale(label, 1 / reduce, 0)` — a numpy emulation of the label kernel that reads only what the kernel reads, and the
cases both test files share."""
import numpy as np

from irn_amd.misc import imutils

from _augment_ref import augment_ref, box_for, image  # noqa: F401  (the image half's yardstick)

LABEL_VALUES = np.asarray([0, 1, 20, 255], np.uint8)


def label(h, w, seed):
    """Per-pixel random labels: a wrong source cell shows with probability 3/4 per cell."""
    return LABEL_VALUES[np.random.default_rng([13, h, w, seed]).integers(0, 4, (h, w))]


def label_ref(lab, params, crop, reduce):
    """uint8 [h, w] -> uint8 [crop / reduce, crop / reduce] as voc12/dataloader.py:251-267 does it on the host."""
    hs, ws, flip, (c_top, c_left, i_top, i_left, rows, cols) = params
    m = imutils.pil_resize(lab, (hs, ws), 0)
    if flip:
        m = np.fliplr(m)
    cont = np.full((crop, crop), 255, np.uint8)
    cont[c_top:c_top + rows, c_left:c_left + cols] = m[i_top:i_top + rows, i_left:i_left + cols]
    return np.array(imutils.pil_rescale(np.ascontiguousarray(cont), 1.0 / reduce, 0))


def emulate_label(tables, labels, crop, reduce):
    """The label kernel in numpy, reading ONLY the packed label bytes and `tables.meta`.  -> int64 [B, g, g], -1 where no
    cell was written (there is none: every cell is assigned)."""
    meta = tables.meta.astype(np.int64)
    packed = np.zeros(max(tables.labels_bytes, 1), np.uint8)
    for lb, off in zip(labels, tables.src_offsets):
        packed[off:off + lb.size] = lb.reshape(-1)
    g = crop // reduce
    out = np.full((len(labels), g, g), -1, np.int64)
    for i in range(len(labels)):
        h, w, c_top, c_left, rows, cols, src, rtab, ctab = meta[i * 12:i * 12 + 9]
        for y in range(g):
            yy = reduce * y + reduce // 2 - c_top
            for x in range(g):
                xx = reduce * x + reduce // 2 - c_left
                if 0 <= yy < rows and 0 <= xx < cols:
                    out[i, y, x] = packed[src + meta[rtab + yy] * w + meta[ctab + xx]]
                else:
                    out[i, y, x] = 255
    return out


def scaled(h, w, scale):
    return int(np.round(h * scale)), int(np.round(w * scale))


# (h, w, crop): images from 5x7 to 120x140 against crops 8 (grid 2x2 at reduce 4) and 96
SHAPES = [
    (5, 7, 8),         # smaller than the crop in both axes at 0.5 and 1.0, larger in one at 1.5 (8 x 10 -> 8 == crop, 10 > crop)
    (6, 13, 8),        # smaller in one axis, larger in the other
    (13, 6, 8),        # the same, portrait
    (20, 27, 8),       # larger in both
    (70, 90, 96),      # 0.5: smaller in both; 1.0: smaller in both; 1.5: 105 x 135 larger in both
    (120, 140, 96),    # 0.5: 60 x 70 smaller in both; 1.0 and 1.5 larger in both
    (50, 137, 96),     # smaller in one axis, larger in the other at 1.0 and 1.5
]
SCALES = [0.5, 1.5, 1.0]           # both ends of the range, and hs, ws == h, w


def cases(shapes=SHAPES):
    """Every (h, w, crop, params): shapes x scales x mirror {0, 1} x the box at its four extreme positions (offsets 0 / max
    per axis: the box against every edge of the image where it is a window, of the container where it is padded)."""
    out = []
    for h, w, crop in shapes:
        for scale in SCALES:
            hs, ws = scaled(h, w, scale)
            for flip in (0, 1):
                for left in sorted({0, abs(ws - crop)}):
                    for top in sorted({0, abs(hs - crop)}):
                        out.append((h, w, crop, (hs, ws, flip, box_for(hs, ws, crop, left, top))))
    return out
