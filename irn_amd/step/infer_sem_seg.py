"""Segmentation inference with the network train_sem_seg wrote (not in the reference), in the calling process on its device.

Reads  args.seg_weights_name + '.pth', args.infer_list, args.voc12_root, args.num_workers, args.num_classes
Writes args.seg_pred_dir/<name>.png  uint8 [H,W] (0 = background, class + 1 otherwise): the format of make_sem_seg_labels,
       which eval_sem_seg reads

Per image and scale: normalise, pad with zeros at the bottom and the right to multiples of 16, run the image and its mirror in
one pass of two rows and add the mirrored-back logits.

Default (--seg_infer_scales 1.0, --seg_crf_iters 0): the arg-max of the logits' bilinear upsampling at the image's size
(`ops.seg_argmax`, irn_amd/csrc/seg_loss.hip: the upsampled [C, H, W] tensor is never written).

--seg_infer_scales S ...: DeepLab's multi-scale protocol.  The image is resized to `ops.rescale_size(h, w, s)` with the
Pillow-exact bicubic kernel (`ops.bicubic_resize`; scale 1 is the image itself), every scale gives the map
0.5 * (logits + mirrored-back logits of the mirror), and one launch (`ops.seg_fuse`, irn_amd/csrc/seg_fuse.hip)
upsamples all of them to the image's size, takes each one's softmax, averages and takes the arg-max: no [C, H, W] tensor is
written.
--seg_crf_iters T > 0: the same launch also writes the averaged probabilities, and a dense CRF seeded with them
(`ops.crf_prob`, T mean-field iterations over the image) gives the map that is written.  At most 31 classes (32 labels).

In the reproducible mode (IRN_DETERMINISTIC, default 1) two runs write the same bytes in every mode.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from .. import _tuned, ops
from ..net import weights
from ..net.resnet50_seg import OUTPUT_STRIDE, Net
from ..voc12 import dataloader
from . import _classes, _eval, _io

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _save_png(path, label):
    Image.fromarray(label).save(path)


def network_input(img, device):
    """uint8 [H,W,3] (host) -> fp32 [2,3,Hp,Wp] on the device: the normalised image, zero-padded at the bottom and the right to
    multiples of 16, and its mirror."""
    x = img.to(device, non_blocking=True).permute(2, 0, 1).float()
    mean = torch.tensor(MEAN, device=device).view(3, 1, 1)
    std = torch.tensor(STD, device=device).view(3, 1, 1)
    x = (x / 255.0 - mean) / std
    h, w = x.shape[1:]
    x = F.pad(x, (0, -w % OUTPUT_STRIDE, 0, -h % OUTPUT_STRIDE))
    return torch.stack([x, x.flip(-1)]).contiguous()


def predict(model, img, device):
    """uint8 [H,W,3] -> uint8 [H,W] on the device."""
    h, w = int(img.shape[0]), int(img.shape[1])
    with torch.no_grad():
        a = model(network_input(img, device))
        logits = (a[0] + a[1].flip(-1))[None].contiguous()
    return ops.seg_argmax(logits, OUTPUT_STRIDE, (h, w))[0]


def scale_maps(model, img, scales, device):
    """uint8 [H,W,3] (host or device) -> (maps, sizes) for `ops.seg_fuse`: per scale the fp32 [C,h,w] mean of the logits of the
    rescaled image and of its mirror, and the rescaled image's (Hs, Ws)."""
    h, w = int(img.shape[0]), int(img.shape[1])
    img = img.to(device, non_blocking=True)
    maps, sizes = [], []
    with torch.no_grad():
        for s in scales:
            size = (h, w) if s == 1.0 else ops.rescale_size(h, w, s)
            if min(size) < 1:
                raise ValueError("infer_sem_seg: scale %g leaves nothing of an image of %dx%d" % (s, h, w))
            a = model(network_input(img if size == (h, w) else ops.bicubic_resize(img, size), device))
            maps.append((0.5 * (a[0] + a[1].flip(-1))).contiguous())
            sizes.append(size)
    return maps, sizes


def predict_fused(model, img, scales, crf_iters, device):
    """uint8 [H,W,3] -> uint8 [H,W] on the device: the multi-scale fusion, and with `crf_iters` > 0 the CRF over its
    probabilities."""
    h, w = int(img.shape[0]), int(img.shape[1])
    img = img.to(device, non_blocking=True)
    maps, sizes = scale_maps(model, img, scales, device)
    label, prob = ops.seg_fuse(maps, sizes, OUTPUT_STRIDE, (h, w), want_label=crf_iters == 0, want_prob=crf_iters > 0)
    if crf_iters == 0:
        return label
    return ops.crf_prob(img, prob, t=crf_iters)


def modes(args, c):
    """(scales, crf_iters) of --seg_infer_scales and --seg_crf_iters, checked before the first image; `c` foreground classes."""
    scales = getattr(args, "seg_infer_scales", None)
    scales = [1.0] if scales is None else [float(s) for s in (scales if isinstance(scales, (list, tuple)) else [scales])]
    if not 1 <= len(scales) <= ops.SEG_FUSE_MAX_MAPS or not all(0.0 < s <= 4.0 for s in scales):
        raise ValueError("--seg_infer_scales %s: 1..%d values in (0, 4]" % (scales, ops.SEG_FUSE_MAX_MAPS))
    crf_iters = int(getattr(args, "seg_crf_iters", 0) or 0)
    if crf_iters < 0:
        raise ValueError("--seg_crf_iters %d: 0 (off) or a number of mean-field iterations" % crf_iters)
    if crf_iters > 0 and c + 1 > 32:
        raise ValueError("--seg_crf_iters %d with --num_classes %d: the dense CRF takes at most 32 labels (31 classes and the "
                         "background)" % (crf_iters, c))
    return scales, crf_iters


def run(args):
    """Returns {'images': the number of files written}, and with --seg_infer_scales or --seg_crf_iters away from their defaults
    also 'scales' and 'crf_iters'."""
    with _tuned.process_mode():
        return _run(args)


def _run(args):
    device = _eval.device()
    c = _classes.num_classes(args)
    scales, crf_iters = modes(args, c)
    default = scales == [1.0] and crf_iters == 0
    model = weights.load_checkpoint(lambda: Net(n_classes=c), args.seg_weights_name + ".pth", strict=True).to(device)
    names = [dataloader.decode_int_filename(n) for n in dataloader.load_img_name_list(args.infer_list)]
    os.makedirs(args.seg_pred_dir, exist_ok=True)

    def load(name):
        return {"img": np.array(Image.open(dataloader.get_img_path(name, args.voc12_root)).convert("RGB"))}

    writer = _io.AsyncWriter()
    try:
        with torch.cuda.device(device):
            for name, item in _eval.items(names, load, args):
                if default:
                    label = predict(model, item["img"], device)
                else:
                    label = predict_fused(model, item["img"], scales, crf_iters, device)
                writer.submit(_save_png, os.path.join(args.seg_pred_dir, name + ".png"), label.cpu().numpy())
    finally:
        writer.close()
    torch.cuda.empty_cache()
    if default:
        return {"images": len(names)}
    return {"images": len(names), "scales": scales, "crf_iters": crf_iters}
