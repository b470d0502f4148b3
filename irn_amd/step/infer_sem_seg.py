"""Segmentation inference with the network train_sem_seg wrote (not in the reference), in the calling process on its device.

Reads  args.seg_weights_name + '.pth', args.infer_list, args.voc12_root, args.num_workers, args.num_classes
Writes args.seg_pred_dir/<name>.png  uint8 [H,W] (0 = background, class + 1 otherwise): the format of make_sem_seg_labels,
       which eval_sem_seg reads

Per image: normalise, pad with zeros at the bottom and the right to multiples of 16, run the image and its mirror in one pass
of two rows, add the mirrored-back logits, and take the arg-max of their bilinear upsampling at the image's size
(`ops.seg_argmax`, irn_amd/csrc/seg_loss.hip: the upsampled [C, H, W] tensor is never written).  Single scale: no multi-scale
pass, no CRF.  In the reproducible mode (IRN_DETERMINISTIC, default 1) two runs write the same bytes.
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


def run(args):
    """Returns {'images': the number of files written}."""
    with _tuned.process_mode():
        return _run(args)


def _run(args):
    device = _eval.device()
    c = _classes.num_classes(args)
    model = weights.load_checkpoint(lambda: Net(n_classes=c), args.seg_weights_name + ".pth", strict=True).to(device)
    names = [dataloader.decode_int_filename(n) for n in dataloader.load_img_name_list(args.infer_list)]
    os.makedirs(args.seg_pred_dir, exist_ok=True)

    def load(name):
        return {"img": np.array(Image.open(dataloader.get_img_path(name, args.voc12_root)).convert("RGB"))}

    writer = _io.AsyncWriter()
    try:
        with torch.cuda.device(device):
            for name, item in _eval.items(names, load, args):
                label = predict(model, item["img"], device)
                writer.submit(_save_png, os.path.join(args.seg_pred_dir, name + ".png"), label.cpu().numpy())
    finally:
        writer.close()
    torch.cuda.empty_cache()
    return {"images": len(names)}
