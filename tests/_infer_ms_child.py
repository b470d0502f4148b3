"""Child process of tests/test_gpu_infer_sem_seg_ms.py: `ops.seg_fuse` and `ops.crf_prob` driven by hand on the model and the images
that infer_sem_seg reads, in a fresh process in the step's own mode (MIOpen keeps the solver it resolved for a problem, so the
process the tests run in is no place to repeat the step's convolutions bit for bit)."""
import os

import numpy as np
import torch
from PIL import Image


def main(argv):
    """argv: VOC root, image list, checkpoint, scales (comma-separated), CRF iterations.  -> {name: {"fused": the label map of the
    multi-scale fusion, "crf": the CRF of the single-scale fusion's probabilities}} as nested lists."""
    from irn_amd import _tuned, ops
    from irn_amd.net import weights
    from irn_amd.net.resnet50_seg import OUTPUT_STRIDE, Net
    from irn_amd.step import _eval
    from irn_amd.step.infer_sem_seg import network_input
    from irn_amd.voc12 import dataloader
    root, lst, ckpt, scales, crf_iters = argv[0], argv[1], argv[2], [float(s) for s in argv[3].split(",")], int(argv[4])
    out = {}
    with _tuned.process_mode():
        device = _eval.device()
        model = weights.load_checkpoint(lambda: Net(n_classes=20), ckpt, strict=True).to(device)

        def scale_map(img, size):
            with torch.no_grad():
                a = model(network_input(img if size == tuple(img.shape[:2]) else ops.bicubic_resize(img, size), device))
            return (0.5 * (a[0] + a[1].flip(-1))).contiguous()

        for name in [dataloader.decode_int_filename(n) for n in dataloader.load_img_name_list(lst)]:
            img = torch.from_numpy(np.array(Image.open(os.path.join(root, "JPEGImages", name + ".jpg")).convert("RGB"))).to(device)
            h, w = int(img.shape[0]), int(img.shape[1])
            sizes = [(h, w) if s == 1.0 else (int(np.round(h * s)), int(np.round(w * s))) for s in scales]
            fused, _ = ops.seg_fuse([scale_map(img, size) for size in sizes], sizes, OUTPUT_STRIDE, (h, w))
            _, prob = ops.seg_fuse([scale_map(img, (h, w))], [(h, w)], OUTPUT_STRIDE, (h, w), want_label=False, want_prob=True)
            out[name] = {"fused": fused.cpu().numpy(), "crf": ops.crf_prob(img, prob, t=crf_iters).cpu().numpy()}
    return out
