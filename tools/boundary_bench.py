#!/usr/bin/env python3
"""Cost of --boundary_iou_ratio (Boundary IoU in eval_sem_seg, Boundary AP in eval_ins_seg) on the 64 synthetic VOC-size
images of tools/eval_bench.py, at the published ratio 0.02 (a band of 10 to 14 pixels on these sizes):

  - the three entries alone on resident inputs: one pass over the split per sample, device events around it, the median of
    --reps samples (label_band over the instance maps, label_boundary_counts, mask_boundary_overlap);
  - eval_sem_seg and eval_ins_seg with the flag off and on, images/s (files read and decoded in both);
  - the same counts on the host from scipy.ndimage.binary_erosion per class / instance, the form of the published code, on
    the first --cpu-images images (their counts are checked against the device's while at it).
Prints one JSON line.

    python tools/boundary_bench.py [--images 64] [--cpu-images 16] [--reps 20] [--ratio 0.02]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_bench  # noqa: E402


def load_split(root, ids, ratio, dev):
    """Every image's inputs on the device: (pred, gt, masks, inst_map, n_inst, d)."""
    from PIL import Image
    from irn_amd import ops
    from irn_amd.voc12 import eval_data
    items = []
    for id in ids:
        gt = eval_data.class_label(root, id)
        pred = np.array(Image.open(os.path.join(root, "sem", id + ".png")), dtype=np.uint8)
        inst, inst_class = eval_data.instance_label(root, id)
        det = np.load(os.path.join(root, "ins", id + ".npy"), allow_pickle=True).item()
        items.append({"pred": torch.from_numpy(pred).to(dev), "gt": torch.from_numpy(gt).to(dev),
                      "masks": torch.from_numpy(np.ascontiguousarray(det["mask"])).to(dev), "inst": torch.from_numpy(inst).to(dev),
                      "g": len(inst_class), "d": ops.boundary_distance(gt.shape[0], gt.shape[1], ratio)})
    return items


def event_ms(fn, reps):
    """Median and extremes of `reps` samples of fn() in device time, after two warm-up calls."""
    fn()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def scipy_counts(pred, gt, masks, inst, g, d, nc=21):
    """The published form on the host: one erosion per class present and per mask / instance."""
    from scipy import ndimage as ndi
    k = np.ones((3, 3))

    def bnd(m):
        return m & ~ndi.binary_erosion(m, structure=k, iterations=d, border_value=0)
    pred = np.where(pred == 255, 0, pred)
    counts = np.zeros((nc, 3), np.int64)
    valid = gt != 255
    P = np.zeros(gt.shape, bool)
    G = np.zeros(gt.shape, bool)
    for c in np.unique(pred):
        P |= bnd(pred == c)
    for c in np.unique(gt):                               # 255 included: the void ring bounds the classes it touches
        G |= bnd(gt == c)
    for c in range(nc):
        counts[c] = ((valid & P & G & (pred == c) & (gt == c)).sum(), (valid & P & (pred == c)).sum(), (G & (gt == c)).sum())
    gb = [bnd(inst == j + 1) for j in range(g)]
    mb = [bnd(m != 0) for m in masks]
    inter_b = np.array([[(a & b).sum() for b in gb] for a in mb], np.int64).reshape(len(mb), g)
    return counts, inter_b, np.array([a.sum() for a in mb], np.int64), np.array([b.sum() for b in gb], np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--cpu-images", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ratio", type=float, default=0.02)
    a = ap.parse_args()
    from irn_amd import ops
    from irn_amd.step import eval_ins_seg, eval_sem_seg
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"metric": "boundary counts", "args": vars(a), "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as root:
        ids = eval_bench.make_tree(root, a.images)
        items = load_split(root, ids, a.ratio, dev)
        res["pixels"] = int(sum(it["gt"].numel() for it in items))
        res["masks"] = int(sum(it["masks"].shape[0] for it in items))
        res["d_min"], res["d_max"] = min(it["d"] for it in items), max(it["d"] for it in items)
        scratch = torch.empty(max(it["inst"].numel() for it in items), dtype=torch.uint8, device=dev)
        counts = torch.zeros(21, 3, dtype=torch.int64, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)

        def band_pass():
            for it in items:
                ops.label_band(it["inst"], it["d"])

        def sem_pass():
            for it in items:
                ops.label_boundary_counts(it["pred"], it["gt"], it["d"], counts, bad)

        def ins_pass():
            for it in items:
                ops.mask_boundary_overlap(it["masks"], it["inst"], it["g"], it["d"], bad, scratch)

        def conf_pass():                                  # the region counts the steps already make, for scale
            for it in items:
                ops.label_confusion(it["pred"], it["gt"])

        def overlap_pass():
            for it in items:
                ops.mask_overlap(it["masks"], it["inst"], it["g"], bad)

        for name, fn in (("label_band", band_pass), ("label_boundary_counts", sem_pass), ("mask_boundary_overlap", ins_pass),
                         ("label_confusion", conf_pass), ("mask_overlap", overlap_pass)):
            res[name + "_split"] = event_ms(fn, a.reps)       # one pass over all images, host launches included

        for name, run in (("eval_sem_seg", eval_sem_seg.run), ("eval_ins_seg", eval_ins_seg.run)):
            for tag, ratio in (("off", 0.0), ("on", a.ratio)):
                args = eval_bench._args(root, [])
                args.boundary_iou_ratio = ratio

                def go(run=run, args=args):
                    with contextlib.redirect_stdout(io.StringIO()):
                        return run(args)
                dt = eval_bench.timed(go, reps=2)
                res["%s_%s_images_per_s" % (name, tag)] = round(a.images / dt, 1)

        n = min(a.cpu_images, len(items))
        try:
            import scipy.ndimage  # noqa: F401
        except ImportError:
            n = 0
            res["scipy"] = "not installed"
        if n > 0:
            host = [{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in it.items()} for it in items[:n]]
            t0 = time.perf_counter()
            want = [scipy_counts(it["pred"], it["gt"], it["masks"], it["inst"], it["g"], it["d"]) for it in host]
            res["scipy_images_per_s"] = round(n / (time.perf_counter() - t0), 2)
            res["cpu_images"] = n
            same = True
            for it, w in zip(items[:n], want):
                c, _ = ops.label_boundary_counts(it["pred"], it["gt"], it["d"])
                got = ops.mask_boundary_overlap(it["masks"], it["inst"], it["g"], it["d"])
                same &= np.array_equal(c.cpu().numpy(), w[0]) and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got, w[1:]))
            res["device_counts_equal_scipy"] = bool(same)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
