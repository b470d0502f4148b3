"""Image helpers the hot path needs (API mirror of the corresponding reference misc/imutils.py
functions; the colouring helpers of that file are out of scope).  The augmentations of the training step
(`random_resize_long`, `random_scale`, `random_lr_flip`, `random_crop`, `top_left_crop`) take their random source as an argument, a
`numpy.random.Generator` or a `random.Random`, instead of the reference's global `random` module: a seed fixes a run.
"""
import numpy as np
from PIL import Image


def pil_resize(img, size, order):
    """misc/imutils.py:8-17 — PIL bicubic (order 3) or nearest (order 0) resize to (h, w)."""
    if size[0] == img.shape[0] and size[1] == img.shape[1]:
        return img
    resample = {3: Image.BICUBIC, 0: Image.NEAREST}[order]
    return np.asarray(Image.fromarray(img).resize(size[::-1], resample))


def pil_rescale(img, scale, order):
    """misc/imutils.py:19-22."""
    h, w = img.shape[:2]
    return pil_resize(img, (int(np.round(h * scale)), int(np.round(w * scale))), order)


def _uniform(rng):
    return float(rng.random())


def _below(rng, n):
    """An integer in [0, n) from either kind of random source."""
    return int(rng.integers(n)) if hasattr(rng, "integers") else rng.randrange(n)


def random_scale(pair, scale_range, order, rng):
    """misc/imutils.py:36-43 for an (image, label) pair: one scale drawn uniformly from `scale_range`, each member
    rescaled with its own `order` (3 for the image, 0 for the label)."""
    scale = scale_range[0] + _uniform(rng) * (scale_range[1] - scale_range[0])
    return tuple(pil_rescale(m, scale, o) for m, o in zip(pair, order))


def resize_long_size(h, w, target_long):
    """Size `random_resize_long` resizes an h x w image to for a drawn long side (misc/imutils.py:27-34: the scale is
    taken from the longer side, then both sides are rounded as `pil_rescale` rounds them)."""
    scale = target_long / h if w < h else target_long / w
    return int(np.round(h * scale)), int(np.round(w * scale))


def random_resize_long(img, min_long, max_long, rng):
    """misc/imutils.py:25-34: the long side drawn from min_long..max_long, both ends included (`random.randint`), bicubic."""
    target_long = min_long + _below(rng, max_long - min_long + 1)
    h, w = img.shape[:2]
    return pil_rescale(img, target_long / h if w < h else target_long / w, 3)


def random_lr_flip(pair, rng):
    """misc/imutils.py:45-53: with probability 1/2 every member is mirrored left-right.  A single array comes back as one."""
    if isinstance(pair, np.ndarray):
        return random_lr_flip((pair,), rng)[0]
    return tuple(np.fliplr(m) for m in pair) if _below(rng, 2) else tuple(pair)


def _crop_box(size, cropsize, rng):
    """misc/imutils.py:55-78: where an h x w image lands in a cropsize^2 container, per axis: a random window of the image
    where it is larger, a random offset inside the container where it is smaller.  Returns (container top, left, image top,
    left, rows, cols).  The horizontal position is drawn first, as in the reference."""
    h, w = size
    left = _below(rng, abs(w - cropsize) + 1)
    top = _below(rng, abs(h - cropsize) + 1)
    c_left, i_left = (0, left) if w > cropsize else (left, 0)
    c_top, i_top = (0, top) if h > cropsize else (top, 0)
    return c_top, c_left, i_top, i_left, min(cropsize, h), min(cropsize, w)


def random_crop(pair, cropsize, fill, rng):
    """misc/imutils.py:80-101: the same random box for every member; what the image does not cover holds the member's
    fill value ((0, 255) for an image and its label).  A single array (with a single fill value) comes back as one."""
    if isinstance(pair, np.ndarray):
        return random_crop((pair,), cropsize, (fill,), rng)[0]
    c_top, c_left, i_top, i_left, rows, cols = _crop_box(pair[0].shape[:2], cropsize, rng)
    out = []
    for m, f in zip(pair, fill):
        cont = np.full((cropsize, cropsize) + m.shape[2:], f, m.dtype)
        cont[c_top:c_top + rows, c_left:c_left + cols] = m[i_top:i_top + rows, i_left:i_left + cols]
        out.append(cont)
    return tuple(out)


def top_left_crop(img, cropsize, fill):
    """misc/imutils.py:103-117: the image's top-left cropsize^2 corner in a container of `fill`."""
    rows, cols = min(cropsize, img.shape[0]), min(cropsize, img.shape[1])
    cont = np.full((cropsize, cropsize) + img.shape[2:], fill, img.dtype)
    cont[:rows, :cols] = img[:rows, :cols]
    return cont


def HWC_to_CHW(img):
    return np.transpose(img, (2, 0, 1))


def get_strided_size(orig_size, stride):
    """misc/imutils.py:173-174: ceil(size / stride) per axis."""
    return ((orig_size[0] - 1) // stride + 1, (orig_size[1] - 1) // stride + 1)


def get_strided_up_size(orig_size, stride):
    """misc/imutils.py:177-179."""
    s = get_strided_size(orig_size, stride)
    return s[0] * stride, s[1] * stride


def compress_range(arr):
    """misc/imutils.py:182-190: renumber the distinct values to 0..K-1 in ascending order."""
    uniq = np.unique(arr)
    lut = np.zeros(int(uniq.max()) + 1, np.int32)
    lut[uniq] = np.arange(uniq.shape[0])
    out = lut[arr]
    return out - np.min(out)


def crf_inference_label(img, labels, t=10, n_labels=21, gt_prob=0.7):
    """misc/imutils.py:156-170 — dense CRF (pydensecrf's numerics) on the GPU (irn_amd/csrc/crf.hip, no CPU fallback).
    img uint8 [H,W,3] RGB, labels int [H,W] in [0, n_labels).  Returns the argmax labels int64 [H,W] (numpy)."""
    import torch
    from .. import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    img = torch.from_numpy(np.ascontiguousarray(img, dtype=np.uint8)).to(dev)
    lab = torch.from_numpy(np.ascontiguousarray(labels).astype(np.int32)).to(dev)
    return ops.crf_inference_label(img, lab, t=t, n_labels=n_labels, gt_prob=gt_prob).cpu().numpy().astype(np.int64)
