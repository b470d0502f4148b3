#!/usr/bin/env python3
"""Rate of the evaluation steps: images/s of eval_cam (T = 1 and T = 100 thresholds in one pass), eval_sem_seg and
eval_ins_seg over a synthetic VOC-size tree (irn_amd/synth.py sizes and CAMs, random label maps and detections), next to
the numpy restatement of chainercv (tests/_eval_ref.py) on the same files, and the share of the GPU kernels' time in the
step (the rest is reading and decoding files).  Prints one JSON line.

    python tools/eval_bench.py [--images 64] [--cpu-images 16]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from irn_amd import synth  # noqa: E402


def make_tree(root, n):
    import _eval_ref as R
    from PIL import Image
    for d in ("SegmentationClass", "SegmentationObject", "ImageSets/Segmentation", "cam", "sem", "ins"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    ids = []
    for i in range(n):
        id = "2008_%06d" % (i + 1)
        rng = np.random.RandomState(i)
        h, w = synth.voc_image_size(i)
        k = max(synth.voc_num_classes(i), 1)
        keys = synth.voc_keys(k, i)
        cls = np.zeros((h, w), np.uint8)
        obj = np.zeros((h, w), np.uint8)
        dets = []
        for j in range(rng.randint(1, 5)):
            y0, x0 = rng.randint(0, h - 40), rng.randint(0, w - 40)
            y1, x1 = y0 + rng.randint(30, h // 2), x0 + rng.randint(30, w // 2)
            c = keys[j % k]
            cls[y0:y1, x0:x1], obj[y0:y1, x0:x1] = 255, 255
            cls[y0 + 2:y1 - 2, x0 + 2:x1 - 2], obj[y0 + 2:y1 - 2, x0 + 2:x1 - 2] = c + 1, j + 1
            m = np.zeros((h, w), bool)
            m[y0 + rng.randint(0, 8):y1, x0:x1 - rng.randint(0, 8)] = True
            dets.append((m, c, rng.rand()))
        R.save_p_png(os.path.join(root, "SegmentationClass", id + ".png"), cls)
        R.save_p_png(os.path.join(root, "SegmentationObject", id + ".png"), obj)
        np.save(os.path.join(root, "cam", id + ".npy"), {"keys": keys, "high_res": synth.cam_blobs(k, h, w, seed=i)})
        sem = np.where(rng.rand(h, w) < 0.05, 255, cls).astype(np.uint8)
        Image.fromarray(sem).save(os.path.join(root, "sem", id + ".png"))
        np.save(os.path.join(root, "ins", id + ".npy"), {"score": np.float32([d[2] for d in dets]),
                                                         "mask": np.stack([d[0] for d in dets]),
                                                         "class": np.int64([d[1] for d in dets])})
        ids.append(id)
    with open(os.path.join(root, "ImageSets", "Segmentation", "train.txt"), "w") as f:
        f.write("\n".join(ids) + "\n")
    return ids


def _args(root, sweep):
    return argparse.Namespace(voc12_root=root, chainer_eval_set="train", cam_out_dir=os.path.join(root, "cam"),
                              sem_seg_out_dir=os.path.join(root, "sem"), ins_seg_out_dir=os.path.join(root, "ins"),
                              cam_eval_thres=0.15, cam_eval_thres_sweep=sweep, num_workers=8)


def timed(fn, reps=1):
    fn()                                                   # warm: kernels loaded, page cache filled
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def kernel_ms(fn):
    """GPU time of the step's kernels (torch.profiler device events) for one run, in ms."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    total = 0.0
    for e in prof.key_averages():
        if any(s in e.key for s in ("k_cam_hist", "k_cam_reduce", "k_label_hist", "k_mask_overlap")):
            total += getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0))
    return total / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--cpu-images", type=int, default=16)
    a = ap.parse_args()
    import io
    import contextlib
    import _eval_ref as R
    from irn_amd.step import eval_cam, eval_ins_seg, eval_sem_seg
    torch.cuda.set_device(0)
    res = {"metric": "eval steps images/s", "images": a.images, "device": torch.cuda.get_device_name(0)}
    sweep100 = [float(t) for t in np.linspace(0.01, 0.99, 99)]
    with tempfile.TemporaryDirectory() as root:
        make_tree(root, a.images)
        steps = {"eval_cam_t1": (eval_cam.run, _args(root, [])), "eval_cam_t100": (eval_cam.run, _args(root, sweep100)),
                 "eval_sem_seg": (eval_sem_seg.run, _args(root, [])), "eval_ins_seg": (eval_ins_seg.run, _args(root, []))}
        for name, (run, args) in steps.items():
            def go(run=run, args=args):
                with contextlib.redirect_stdout(io.StringIO()):
                    run(args)
            dt = timed(go, reps=2)
            kms = kernel_ms(go)
            res[name + "_images_per_s"] = round(a.images / dt, 1)
            res[name + "_kernel_share"] = round(kms / (1e3 * dt), 4)
        if a.cpu_images > 0:
            sub = tempfile.mkdtemp(dir=root)
            for d in ("SegmentationClass", "SegmentationObject", "ImageSets/Segmentation"):
                os.makedirs(os.path.join(sub, d))
            ids = [l.strip() for l in open(os.path.join(root, "ImageSets", "Segmentation", "train.txt"))][:a.cpu_images]
            for d in ("SegmentationClass", "SegmentationObject"):
                for id in ids:
                    os.link(os.path.join(root, d, id + ".png"), os.path.join(sub, d, id + ".png"))
            with open(os.path.join(sub, "ImageSets", "Segmentation", "train.txt"), "w") as f:
                f.write("\n".join(ids) + "\n")
            n = len(ids)
            t0 = time.perf_counter()
            R.eval_cam(sub, "train", os.path.join(root, "cam"), 0.15)
            t1 = time.perf_counter()
            res["numpy_eval_cam_t1_images_per_s"] = round(n / (t1 - t0), 2)
            # a 100-threshold sweep in numpy is 100 argmax passes per image: estimated from 4 thresholds
            t0 = time.perf_counter()
            for t in (0.1, 0.2, 0.3, 0.4):
                R.eval_cam(sub, "train", os.path.join(root, "cam"), t)
            res["numpy_eval_cam_t100_images_per_s_est"] = round(n / ((time.perf_counter() - t0) / 4 * 100), 3)
            t0 = time.perf_counter()
            R.eval_sem_seg(sub, "train", os.path.join(root, "sem"))
            res["numpy_eval_sem_seg_images_per_s"] = round(n / (time.perf_counter() - t0), 2)
            t0 = time.perf_counter()
            R.eval_ins_seg(sub, "train", os.path.join(root, "ins"))
            res["numpy_eval_ins_seg_images_per_s"] = round(n / (time.perf_counter() - t0), 2)
            res["cpu_images"] = n
    print(json.dumps(res))


if __name__ == "__main__":
    main()
