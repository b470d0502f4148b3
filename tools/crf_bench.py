#!/usr/bin/env python3
"""Rate of the cam_to_ir_label step's compute: images/s of `ops.crf_ir_label` (fg + bg dense CRF, t = 10, on the GPU)
over synthetic VOC-size photos and CAMs (irn_amd/synth.py), and of the numpy restatement (tests/_densecrf_ref.py,
float64 and float32) on a few of the same images.  Prints one JSON line.

    python tools/crf_bench.py [--images 64] [--warmup 4] [--cpu-images 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from irn_amd import ops, synth  # noqa: E402


def _items(n, seed0=0):
    out = []
    for i in range(n):
        s = seed0 + i
        h, w = synth.voc_image_size(s)
        k = synth.voc_num_classes(s)
        out.append((synth.photo(h, w, seed=s), synth.cam_blobs(k, h, w, seed=s), synth.voc_keys(k, s)))
    return out


def gpu_rate(items, warmup):
    dev = torch.device("cuda", 0)
    dev_items = [(torch.from_numpy(img).to(dev), torch.from_numpy(cam).to(dev), torch.from_numpy(keys).to(dev))
                 for img, cam, keys in items]
    for img, cam, keys in dev_items[:warmup]:
        ops.crf_ir_label(img, cam, keys, 0.30, 0.05)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for img, cam, keys in dev_items:
        ops.crf_ir_label(img, cam, keys, 0.30, 0.05)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return len(dev_items) / dt, 1e3 * dt / len(dev_items)


def cpu_rate(items, dtype):
    import _densecrf_ref as R
    t0 = time.perf_counter()
    for img, cam, keys in items:
        R.ir_label(img, cam, keys, 0.30, 0.05, dtype=dtype)
    return len(items) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--cpu-images", type=int, default=2)
    a = ap.parse_args()
    items = _items(a.images)
    ips, ms = gpu_rate(items, a.warmup)
    res = {"metric": "cam_to_ir_label images/s", "gpu_images_per_s": round(ips, 2), "gpu_ms_per_image": round(ms, 2),
           "images": a.images, "classes_mean": round(float(np.mean([len(k) for _, _, k in items])), 2),
           "device": torch.cuda.get_device_name(0)}
    if a.cpu_images > 0:
        few = items[:a.cpu_images]
        res["cpu_restatement_f64_images_per_s"] = round(cpu_rate(few, np.float64), 4)
        res["cpu_restatement_f32_images_per_s"] = round(cpu_rate(few, np.float32), 4)
        res["cpu_images"] = a.cpu_images
    print(json.dumps(res))


if __name__ == "__main__":
    main()
