"""Multi-scale inference dataset of the hot path — API mirror of the reference
voc12/dataloader.py pieces the label-generation steps use:

    decode_int_filename (:24-26), load_img_name_list (:56-60), TorchvisionNormalize (:65-78),
    VOC12ClassificationDatasetMSF (:175-205)

JPEGs are decoded with PIL (the reference's imageio call decodes through PIL as well).  The
image-level labels come from ``cls_labels.npy`` ({int id -> float32[C]}, C = 20 for VOC; ``n_classes=C`` checks the rows); pass ``cls_labels=`` or
keep the file next to the image lists as the reference does.

The two datasets of the IRNet training step are here as well: ``VOC12ImageDataset`` (:109-156, the top-left crops of
the displacement-mean pass) and ``VOC12AffinityDataset`` (:207-273), which hands over the reduced IR label map instead
of the reference's three [|S|, N] float tensors: the fused loss classifies the pairs on the GPU from that map.
Both have a ``raw=True`` form: the decoded bytes and the augmentation's draws, for `irn_amd.ops.augment_pair_batch` and
`augment_batch`.
``VOC12ClassificationDataset`` (:158-173) is the CAM training step's: the reference's augmented item, or (``raw=True``) the
decoded bytes and the augmentation's draws for `irn_amd.ops.augment_batch`.
Nothing here touches the GPU, so the datasets are safe in loader worker processes.
"""
import os

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

from ..misc import imutils

IMG_FOLDER_NAME = "JPEGImages"
N_CAT = 20


def decode_int_filename(int_filename):
    s = str(int(int_filename))
    return s[:4] + "_" + s[4:]


def load_img_name_list(dataset_path):
    """Reads '2007_000032'-style ids as integers 2007000032.  (The reference's
    np.loadtxt(dtype=int32) rejects the underscore under numpy >= 2; parse explicitly.)"""
    with open(dataset_path) as f:
        return np.asarray([int(line.strip().replace("_", "")) for line in f if line.strip()], np.int64)


def load_label_list(img_name_list_path, img_name_list, cls_labels=None, n_classes=None):
    """float32 [N, C]: the image-level labels of the list, from `cls_labels` or from cls_labels.npy beside the list file.
    With `n_classes` every row must have that length: a label file made for another class list is an error that names the
    file and both numbers."""
    path = "cls_labels"
    if cls_labels is None:
        path = os.path.join(os.path.dirname(os.path.abspath(img_name_list_path)), "cls_labels.npy")
        cls_labels = np.load(path, allow_pickle=True).item()
    rows = [np.asarray(cls_labels[int(n)], np.float32).reshape(-1) for n in img_name_list]
    if n_classes is not None:
        for n, row in zip(img_name_list, rows):
            if row.size != int(n_classes):
                raise ValueError("%s: the label of image %s has %d entries, --num_classes is %d"
                                 % (path, decode_int_filename(n), row.size, int(n_classes)))
    return np.array(rows, np.float32)


def get_img_path(img_name, voc12_root):
    if not isinstance(img_name, str):
        img_name = decode_int_filename(img_name)
    return os.path.join(voc12_root, IMG_FOLDER_NAME, img_name + ".jpg")


class TorchvisionNormalize:
    def __init__(self, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.mean = mean
        self.std = std

    def __call__(self, img):
        arr = np.asarray(img)
        out = np.empty_like(arr, np.float32)
        for c in range(3):
            out[..., c] = (arr[..., c] / 255. - self.mean[c]) / self.std[c]
        return out


class VOC12ClassificationDataset(Dataset):
    """item -> {'name': str, 'img': float32 [3, crop, crop], 'label': float32[20]} (voc12/dataloader.py:109-173 as
    step/train_cam.py:44-52 configures it): the long side resized to a length drawn from ``resize_long`` (both ends
    included), normalised, mirrored with probability 1/2 when ``hor_flip``, then a random ``crop_size`` box
    (``crop_method="random"``) or the top-left one, zeros around a smaller image.  The draws of item ``idx`` come from a
    generator seeded with (seed, epoch, idx), in the reference's order — long side, mirror, box (horizontal, vertical): a run
    is fixed by its seed whatever the number of loader workers; call ``set_epoch`` before each pass.

    ``raw=True`` makes no resize and no float array in the worker: the item is {'name', 'img': uint8 [H,W,3], 'size': (H, W),
    'label', 'aug': (hs, ws, flip, box)} with the same draws, and `irn_amd.ops.augment_batch` builds the same floats on the
    GPU for the whole batch (0.4 MB per image cross to the device instead of 3 MB).  Batch such items with
    `classification_collate`: the images are ragged."""

    def __init__(self, img_name_list_path, voc12_root, resize_long=None, hor_flip=False, crop_size=None, crop_method=None,
                 cls_labels=None, raw=False, seed=0, img_normal=TorchvisionNormalize(), n_classes=None):
        self.img_name_list = load_img_name_list(img_name_list_path)
        self.voc12_root = voc12_root
        self.resize_long = resize_long
        self.hor_flip = hor_flip
        self.crop_size = crop_size
        self.crop_method = crop_method
        self.raw = raw
        self.img_normal = img_normal
        self.seed = int(seed)
        self.epoch = 0
        if raw and not crop_size:
            raise ValueError("VOC12ClassificationDataset: raw items are made for a fixed crop_size")
        self.label_list = load_label_list(img_name_list_path, self.img_name_list, cls_labels, n_classes)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.img_name_list)

    def _rng(self, idx):
        return np.random.default_rng([self.seed, self.epoch, int(idx)])

    def draw(self, idx, size):
        """(hs, ws, flip, box) of item `idx` for an image of `size` = (h, w): what the item's augmentation draws."""
        rng = self._rng(idx)
        hs, ws = int(size[0]), int(size[1])
        if self.resize_long:
            lo, hi = self.resize_long
            hs, ws = imutils.resize_long_size(hs, ws, lo + imutils._below(rng, hi - lo + 1))
        flip = imutils._below(rng, 2) if self.hor_flip else 0
        crop = self.crop_size
        if self.crop_method == "random":
            box = imutils._crop_box((hs, ws), crop, rng)
        else:
            box = (0, 0, 0, 0, min(crop, hs), min(crop, ws))
        return hs, ws, flip, box

    def __getitem__(self, idx):
        name_str = decode_int_filename(self.img_name_list[idx])
        img = np.asarray(Image.open(get_img_path(name_str, self.voc12_root)).convert("RGB"))
        label = torch.from_numpy(self.label_list[idx])
        if self.raw:
            size = (img.shape[0], img.shape[1])
            return {"name": name_str, "img": torch.from_numpy(np.array(img)), "size": size, "label": label,
                    "aug": self.draw(idx, size)}
        rng = self._rng(idx)
        if self.resize_long:
            img = imutils.random_resize_long(img, self.resize_long[0], self.resize_long[1], rng)
        if self.img_normal:
            img = self.img_normal(img)
        if self.hor_flip:
            img = imutils.random_lr_flip(img, rng)
        if self.crop_size:
            if self.crop_method == "random":
                img = imutils.random_crop(img, self.crop_size, 0, rng)
            else:
                img = imutils.top_left_crop(img, self.crop_size, 0)
        return {"name": name_str, "img": np.ascontiguousarray(imutils.HWC_to_CHW(img)), "label": label}


def classification_collate(items):
    """Batch of VOC12ClassificationDataset items: labels stacked; the images stacked too when they are the reference's
    [3, crop, crop] floats, kept as a list (with 'size' and 'aug') when they are raw and ragged."""
    out = {"name": [it["name"] for it in items], "label": torch.stack([it["label"] for it in items])}
    if "aug" in items[0]:
        out["img"] = [it["img"] for it in items]
        out["size"] = [it["size"] for it in items]
        out["aug"] = [it["aug"] for it in items]
    else:
        out["img"] = torch.stack([torch.as_tensor(it["img"]) for it in items])
    return out


class VOC12ClassificationDatasetMSF(Dataset):
    """item -> {'name': str, 'img': [scales x [2,3,Hs,Ws]] (image + h-flip; a bare array when there
    is a single scale), 'size': (H, W), 'label': float32[20]}  (voc12/dataloader.py:175-205).

    ``raw=True`` hands over the decoded image as a uint8 tensor [H,W,3] instead: the steps then build the
    per-scale pairs on the GPU (`irn_amd.ops.msf_pack`, bit-identical to the PIL/numpy loop below), which
    cuts the host-to-device traffic of a 4-scale item from 47 MB of floats to 0.8 MB of bytes and frees the
    loader workers of the bicubic resizes."""

    def __init__(self, img_name_list_path, voc12_root, img_normal=TorchvisionNormalize(), scales=(1.0,),
                 cls_labels=None, raw=False, skip_image=None, n_classes=None):
        self.img_name_list = load_img_name_list(img_name_list_path)
        self.voc12_root = voc12_root
        self.img_normal = img_normal
        self.scales = scales
        self.raw = raw
        # raw mode only: `skip_image(name) -> bool` lets a step say that it will not need an image's pixels (the label step that
        # runs second takes the boundary / displacement maps from device memory): the item then carries an EMPTY uint8 tensor
        # and the size read from the file header — no JPEG decode, no upload
        self.skip_image = skip_image
        self.label_list = load_label_list(img_name_list_path, self.img_name_list, cls_labels, n_classes)

    def __len__(self):
        return len(self.img_name_list)

    def __getitem__(self, idx):
        name_str = decode_int_filename(self.img_name_list[idx])
        if self.raw and self.skip_image is not None and self.skip_image(name_str):
            with Image.open(get_img_path(name_str, self.voc12_root)) as im:
                w, h = im.size                       # header only
            return {"name": name_str, "img": torch.empty((0, 0, 3), dtype=torch.uint8), "size": (h, w),
                    "label": torch.from_numpy(self.label_list[idx])}
        img = np.asarray(Image.open(get_img_path(name_str, self.voc12_root)).convert("RGB"))
        if self.raw:
            return {"name": name_str, "img": torch.from_numpy(np.array(img)),
                    "size": (img.shape[0], img.shape[1]), "label": torch.from_numpy(self.label_list[idx])}
        ms = []
        for s in self.scales:
            s_img = img if s == 1 else imutils.pil_rescale(img, s, order=3)
            s_img = imutils.HWC_to_CHW(self.img_normal(s_img))
            ms.append(np.stack([s_img, np.flip(s_img, -1)], axis=0))
        if len(self.scales) == 1:
            ms = ms[0]
        return {"name": name_str, "img": ms, "size": (img.shape[0], img.shape[1]),
                "label": torch.from_numpy(self.label_list[idx])}


class VOC12ImageDataset(Dataset):
    """item -> {'name': str, 'img': float32 [3, crop, crop]}: the normalised image, top-left cropped with zeros around
    it (voc12/dataloader.py:109-156 as step/train_irn.py:87-90 configures it).

    ``raw=True`` hands over {'name', 'img': uint8 [H,W,3], 'size': (H, W), 'aug': (H, W, 0, top-left box)} instead: no
    resize, no mirror, and `irn_amd.ops.augment_batch` builds the same floats on the GPU (its bicubic plan of equal sizes is
    the identity).  Batch such items with `affinity_collate`."""

    def __init__(self, img_name_list_path, voc12_root, crop_size, img_normal=TorchvisionNormalize(), raw=False):
        self.img_name_list = load_img_name_list(img_name_list_path)
        self.voc12_root = voc12_root
        self.crop_size = crop_size
        self.img_normal = img_normal
        self.raw = raw

    def __len__(self):
        return len(self.img_name_list)

    def __getitem__(self, idx):
        name_str = decode_int_filename(self.img_name_list[idx])
        img = np.asarray(Image.open(get_img_path(name_str, self.voc12_root)).convert("RGB"))
        if self.raw:
            h, w = img.shape[:2]
            box = (0, 0, 0, 0, min(self.crop_size, h), min(self.crop_size, w))
            return {"name": name_str, "img": torch.from_numpy(np.array(img)), "size": (h, w), "aug": (h, w, 0, box)}
        img = imutils.top_left_crop(self.img_normal(img), self.crop_size, 0)
        return {"name": name_str, "img": np.ascontiguousarray(imutils.HWC_to_CHW(img))}


class VOC12AffinityDataset(Dataset):
    """item -> {'name': str, 'img': float32 [3, crop, crop], 'label': uint8 [crop/4, crop/4]} (voc12/dataloader.py:207-273):
    image and IR label (``label_dir/<name>.png``) rescaled together by a factor from ``rescale`` (bicubic / nearest), the
    image normalised, both mirrored with probability 1/2 and cropped by one random box (fill 0 / 255), the label then
    reduced by ``pil_rescale(label, 0.25, 0)``.  The draws of item ``idx`` come from a generator seeded with
    (seed, epoch, idx): a run is fixed by its seed whatever the number of loader workers; call ``set_epoch`` before each
    pass.

    ``raw=True`` makes no resize and no float array in the worker: the item is {'name', 'img': uint8 [H,W,3], 'label_map':
    uint8 [H,W], 'size': (H, W), 'aug': (hs, ws, flip, box)} with the same draws, and `irn_amd.ops.augment_pair_batch` builds
    the same floats and the same reduced map on the GPU for the whole batch.  Batch such items with `affinity_collate`.

    ``reduce`` (default 4, the IRNet's grid): the factor the cropped label is reduced by; 1 keeps the label at the crop's size
    (segmentation training) — hand `augment_pair_batch` the same value."""

    def __init__(self, img_name_list_path, label_dir, crop_size, voc12_root, rescale=None,
                 img_normal=TorchvisionNormalize(), hor_flip=False, crop_method="random", seed=0, raw=False, reduce=4):
        self.img_name_list = load_img_name_list(img_name_list_path)
        self.voc12_root = voc12_root
        self.label_dir = label_dir
        self.reduce = int(reduce)
        self.crop_size = crop_size
        self.rescale = rescale
        self.img_normal = img_normal
        self.hor_flip = hor_flip
        self.crop_method = crop_method
        self.seed = int(seed)
        self.epoch = 0
        self.raw = raw

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.img_name_list)

    def _rng(self, idx):
        return np.random.default_rng([self.seed, self.epoch, int(idx)])

    def draw(self, idx, size):
        """(hs, ws, flip, box) of item `idx` for an image of `size` = (h, w): what the item's augmentation draws, in the order
        of `__getitem__` — scale, mirror, box (horizontal, vertical)."""
        rng = self._rng(idx)
        hs, ws = int(size[0]), int(size[1])
        if self.rescale:
            scale = self.rescale[0] + imutils._uniform(rng) * (self.rescale[1] - self.rescale[0])
            hs, ws = int(np.round(hs * scale)), int(np.round(ws * scale))          # as pil_rescale rounds them
        flip = imutils._below(rng, 2) if self.hor_flip else 0
        crop = self.crop_size
        if self.crop_method == "random":
            box = imutils._crop_box((hs, ws), crop, rng)
        else:
            box = (0, 0, 0, 0, min(crop, hs), min(crop, ws))
        return hs, ws, flip, box

    def __getitem__(self, idx):
        name_str = decode_int_filename(self.img_name_list[idx])
        img = np.asarray(Image.open(get_img_path(name_str, self.voc12_root)).convert("RGB"))
        label = np.asarray(Image.open(os.path.join(self.label_dir, name_str + ".png")))
        if self.raw:
            size = (img.shape[0], img.shape[1])
            if label.dtype != np.uint8 or label.shape != size:
                raise ValueError("VOC12AffinityDataset: %s: a %s %s label map for a %dx%d image" % ((name_str, label.dtype, label.shape) + size))
            return {"name": name_str, "img": torch.from_numpy(np.array(img)), "label_map": torch.from_numpy(np.array(label)),
                    "size": size, "aug": self.draw(idx, size)}
        rng = self._rng(idx)
        if self.rescale:
            img, label = imutils.random_scale((img, label), self.rescale, (3, 0), rng)
        if self.img_normal:
            img = self.img_normal(img)
        if self.hor_flip:
            img, label = imutils.random_lr_flip((img, label), rng)
        if self.crop_method == "random":
            img, label = imutils.random_crop((img, label), self.crop_size, (0, 255), rng)
        else:
            img, label = imutils.top_left_crop(img, self.crop_size, 0), imutils.top_left_crop(label, self.crop_size, 255)
        reduced = imutils.pil_rescale(np.ascontiguousarray(label), 1.0 / self.reduce, 0)
        return {"name": name_str, "img": np.ascontiguousarray(imutils.HWC_to_CHW(img)), "label": np.array(reduced)}       # (a copy: PIL hands out read-only memory)


def affinity_collate(items):
    """Batch of raw VOC12AffinityDataset / VOC12ImageDataset items: the ragged images (and label maps) stay lists, with
    'size' and 'aug' beside them; items of the reference's form go through torch's default collate."""
    if "aug" not in items[0]:
        return torch.utils.data.default_collate(items)
    out = {k: [it[k] for it in items] for k in ("name", "img", "size", "aug")}
    if "label_map" in items[0]:
        out["label_map"] = [it["label_map"] for it in items]
    return out
