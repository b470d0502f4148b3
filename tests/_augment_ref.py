"""Yardstick of the batched training-input pipeline (irn_amd/csrc/augment.hip, ops.augment_tables / augment_batch): the
PIL / numpy pipeline of the CAM training dataset for EXPLICIT draws (hs, ws, flip, box), a numpy emulation of the two
device passes driven by the host tables, the shapes both test files share, and a small synthetic VOC tree."""
import os

import numpy as np

from irn_amd.misc import imutils
from irn_amd.voc12.dataloader import TorchvisionNormalize

# (h, w, crop, (min_long, max_long)): the smallest shapes at which each branch of the kernels exists
SHAPES = [
    (20, 27, 32, (16, 48)),        # padded on both axes; upscale (ksize 5) and downscale (ksize >= 7)
    (50, 37, 32, (20, 64)),        # portrait; window on one axis, pad on the other
    (70, 90, 32, (40, 120)),       # window on both axes
    (3, 100, 32, (90, 110)),       # the vertical plan is the identity while the horizontal is not; extreme aspect
    (300, 280, 260, (200, 400)),   # an output row crosses a 256-thread block seam
]
TRAIN_SHAPES = [(375, 500, 512, (320, 640)), (500, 333, 512, (320, 640))]       # the training shape


def image(h, w, seed):
    return np.random.default_rng([7, h, w, seed]).integers(0, 256, (h, w, 3), dtype=np.uint8)


def box_for(hs, ws, crop, left, top):
    """`imutils._crop_box` for chosen offsets instead of drawn ones."""
    c_left, i_left = (0, left) if ws > crop else (left, 0)
    c_top, i_top = (0, top) if hs > crop else (top, 0)
    return c_top, c_left, i_top, i_left, min(crop, hs), min(crop, ws)


def params_for(h, w, crop, target, flip, corner, rng=None):
    """(hs, ws, flip, box) for a long side `target` and the box at `corner` = "zero", "max" or "drawn" offsets."""
    hs, ws = imutils.resize_long_size(h, w, target)
    max_left, max_top = abs(ws - crop), abs(hs - crop)
    if corner == "zero":
        left, top = 0, 0
    elif corner == "max":
        left, top = max_left, max_top
    else:
        left, top = int(rng.integers(max_left + 1)), int(rng.integers(max_top + 1))
    return hs, ws, flip, box_for(hs, ws, crop, left, top)


def cases(shapes):
    """Every (h, w, crop, params) of the shape list x {both ends of the long-side range, target == long side, one drawn
    value} x mirror {0, 1} x box {offsets 0, offsets at their maximum, drawn}."""
    out = []
    for h, w, crop, (lo, hi) in shapes:
        rng = np.random.default_rng([11, h, w])
        targets = sorted({lo, hi, max(h, w), int(rng.integers(lo, hi + 1))})
        for target in targets:
            for flip in (0, 1):
                for corner in ("zero", "max", "drawn"):
                    out.append((h, w, crop, params_for(h, w, crop, target, flip, corner, rng)))
    return out


def augment_ref(img, params, crop, normal=TorchvisionNormalize()):
    """uint8 [h, w, 3] -> float32 [3, crop, crop]: PIL bicubic resize to (hs, ws) -> TorchvisionNormalize -> fliplr -> box
    into zeros -> CHW."""
    hs, ws, flip, (c_top, c_left, i_top, i_left, rows, cols) = params
    f = normal(imutils.pil_resize(img, (hs, ws), 3))
    if flip:
        f = np.fliplr(f)
    out = np.zeros((crop, crop, 3), np.float32)
    out[c_top:c_top + rows, c_left:c_left + cols] = f[i_top:i_top + rows, i_left:i_left + cols]
    return np.ascontiguousarray(imutils.HWC_to_CHW(out))


def _clip8(acc):
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def emulate(tables, images, crop, lut):
    """The two device passes in numpy, reading ONLY what the kernels read: the packed pixels, `tables.meta`, `lut`
    [3, 256].  -> float32 [B, 3, crop, crop] (NaN where no cell was written)."""
    meta = tables.meta.astype(np.int64)
    pixels = np.zeros(tables.pixels_bytes, np.uint8)
    for im, off in zip(images, tables.src_offsets):
        pixels[off:off + im.size] = im.reshape(-1)
    mid = np.zeros(max(tables.scratch_bytes, 1), np.uint8)
    out = np.full((len(images), 3, crop, crop), np.nan, np.float32)
    for i in range(len(images)):
        h, w, c_top, c_left, rows, cols, r0, nrows, kx, ky, src, moff, xtab, ytab = meta[i * 16:i * 16 + 14]
        img = pixels[src:src + h * w * 3].reshape(h, w, 3).astype(np.int64)
        lo, cnt, k = meta[xtab:xtab + cols], meta[xtab + cols:xtab + 2 * cols], meta[xtab + 2 * cols:xtab + 2 * cols + cols * kx].reshape(cols, kx)
        m = mid[moff:moff + nrows * cols * 3].reshape(nrows, cols, 3)
        for x in range(cols):
            acc = np.full((nrows, 3), 1 << 21, np.int64)
            for t in range(cnt[x]):
                acc += img[r0:r0 + nrows, lo[x] + t] * k[x, t]
            m[:, x] = _clip8(acc)
        lo, cnt, k = meta[ytab:ytab + rows], meta[ytab + rows:ytab + 2 * rows], meta[ytab + 2 * rows:ytab + 2 * rows + rows * ky].reshape(rows, ky)
        out[i] = 0.0
        m64 = m.astype(np.int64)
        for y in range(rows):
            acc = np.full((cols, 3), 1 << 21, np.int64)
            for t in range(cnt[y]):
                acc += m64[lo[y] + t] * k[y, t]
            v = _clip8(acc)
            for c in range(3):
                out[i, c, c_top + y, c_left:c_left + cols] = lut[c][v[:, c]]
    return out


def write_voc(root, n, h=120, w=140, seed=0):
    """n synthetic JPEGs under root/JPEGImages, a list file and `cls_labels.npy` beside it; returns the list's path."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "JPEGImages"), exist_ok=True)
    names, labels = [], {}
    for i in range(n):
        name = "2007_%06d" % (i + 1)
        names.append(name)
        img = np.clip(rng.randint(0, 255, (h // 8 + 1, w // 8 + 1, 3)).repeat(8, 0).repeat(8, 1)[:h, :w] + rng.randint(-9, 9, (h, w, 3)), 0, 255)
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=92)
        lab = np.zeros(20, np.float32)
        lab[rng.choice(20, 1 + i % 2, replace=False)] = 1
        labels[int(name.replace("_", ""))] = lab
    lst = os.path.join(root, "train.txt")
    with open(lst, "w") as f:
        f.write("\n".join(names) + "\n")
    np.save(os.path.join(root, "cls_labels.npy"), labels, allow_pickle=True)
    return lst
