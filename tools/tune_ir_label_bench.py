#!/usr/bin/env python3
"""tune_ir_label's two calls against the calls they replace, on resident inputs.  Prints one JSON line and writes it to
--json-out.

Input: `--images` synthetic VOC-size photos and CAMs, made as tools/crf_bench.py makes them (irn_amd/synth.py), with a ground
truth cut from the CAM blobs.  One measurement is a pass over all images between two device events; after one warm-up pass of
each path the paths alternate, and the median of `--reps` passes is reported as ms per image.

  (a) 4 x 4 grid, 8 distinct thresholds: one `crf_label_sweep` + one `ir_label_confusion` per image, against 16 `crf_ir_label`
      calls per image, each map read back and counted with numpy (what a search by hand over cam_to_ir_label does, minus the
      files).  The two paths must give the same histogram.
  (b) the same for a 2 x 2 grid (4 thresholds against 4 calls)
  (c) `crf_label_sweep` at T = 2 against one `crf_ir_label`: what the chunked entry costs where it shares nothing more
  (d) `ir_label_confusion` alone, 4 x 4 and 16 x 16, on the planes of (a) / random planes of 16 thresholds
  (e) with --classes80, INSTEAD of (a)-(d): the two counts at 81 classes (`n_classes=81`), figures only — `ir_label_confusion`
      at 16 x 16 on random planes of the labels 1..80 (eight launches per image: the fg axis in groups of two), and
      `label_sweep_confusion` of one 94 x 125 score map of 80 channels (375 x 500 output) at 16 thresholds

    python tools/tune_ir_label_bench.py [--images 64] [--reps 20] [--json-out profiles/tune_ir_label_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from irn_amd import ops, synth  # noqa: E402

FG4, BG4 = [0.30, 0.40, 0.50, 0.60], [0.05, 0.10, 0.15, 0.20]
FG2, BG2 = [0.30, 0.45], [0.05, 0.15]


def _items(n, dev):
    out = []
    for s in range(n):
        h, w = synth.voc_image_size(s)
        k = synth.voc_num_classes(s)
        cam, keys = synth.cam_blobs(k, h, w, seed=s), synth.voc_keys(k, s)
        gt, _ = synth.blob_ground_truth(cam, keys, 0.4, 0.32)
        out.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (synth.photo(h, w, seed=s), cam, keys, gt)))
    return out


def _hist22(gt, label):
    r = np.where(gt == 255, 21, gt).astype(np.int64).reshape(-1)
    c = np.where(label == 255, 21, label).astype(np.int64).reshape(-1)
    return np.bincount(r * 22 + c, minlength=484).reshape(22, 22)


def sweep_path(items, fgs, bgs):
    th = np.unique(np.float32(fgs + bgs))
    fi, bi = np.searchsorted(th, np.float32(fgs)), np.searchsorted(th, np.float32(bgs))
    hist = bad = None
    for img, cam, keys, gt in items:
        hist, bad = ops.ir_label_confusion(ops.crf_label_sweep(img, cam, keys, th), fi, bi, gt, hist, bad)
    return hist


def single_path(items, fgs, bgs):
    hist = np.zeros((len(fgs), len(bgs), 22, 22), np.int64)
    for img, cam, keys, gt in items:
        g = gt.cpu().numpy()
        for i, fg in enumerate(fgs):
            for j, bg in enumerate(bgs):
                hist[i, j] += _hist22(g, ops.crf_ir_label(img, cam, keys, fg, bg).cpu().numpy())
    return hist


def alternate(paths, reps):
    """{name: fn} -> {name: median ms of a call}, device events, one warm-up each, then alternating."""
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: float(np.median(v)) for name, v in ms.items()}


def classes80(n, reps, dev):
    rng = np.random.RandomState(0)
    gts = [torch.from_numpy(rng.randint(0, 81, synth.voc_image_size(s)).astype(np.uint8)).to(dev) for s in range(n)]
    planes = [torch.from_numpy(np.where(rng.rand(16, *g.shape) < 0.5, 0, rng.randint(1, 81, size=(16,) + tuple(g.shape))).astype(np.uint8))
              .to(dev) for g in gts]
    rw = torch.from_numpy(np.abs(rng.randn(80, 94, 125)).astype(np.float32)).to(dev)
    gt = torch.from_numpy(rng.randint(0, 81, (375, 500)).astype(np.uint8)).to(dev)
    keys, th = torch.arange(80, device=dev), ops.eval_thresholds(np.linspace(0.05, 0.8, 16), dev)
    all16 = list(range(16))

    def count():
        hist = bad = None
        for p, g in zip(planes, gts):
            hist, bad = ops.ir_label_confusion(p, all16, all16, g, hist, bad, n_classes=81)
    m = alternate({"ir": count, "sweep": lambda: ops.label_sweep_confusion([rw], [(375, 500)], [keys], [gt], th, n_classes=81)}, reps)
    return {"metric": "81-class counts", "images": n, "reps": reps, "device": torch.cuda.get_device_name(0),
            "ir_label_confusion_16x16_us_per_image": round(1e3 * m["ir"] / n, 2),
            "label_sweep_confusion_80ch_375x500_t16_ms": round(m["sweep"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json-out", default=os.path.join(ROOT, "profiles", "tune_ir_label_bench.json"))
    ap.add_argument("--classes80", action="store_true", help="only (e): the 81-class counts")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.classes80:
        print(json.dumps(classes80(a.images, a.reps, dev)))
        return
    items = _items(a.images, dev)
    n = len(items)
    res = {"metric": "tune_ir_label calls, ms per image (median of %d passes over %d images)" % (a.reps, n), "images": n,
           "reps": a.reps, "classes_mean": round(float(np.mean([int(it[2].numel()) for it in items])), 2),
           "device": torch.cuda.get_device_name(0)}
    for tag, fgs, bgs in (("grid4x4", FG4, BG4), ("grid2x2", FG2, BG2)):
        same = bool(np.array_equal(sweep_path(items, fgs, bgs).cpu().numpy(), single_path(items, fgs, bgs)))
        m = alternate({"sweep": lambda: sweep_path(items, fgs, bgs), "single": lambda: single_path(items, fgs, bgs)}, a.reps)
        res[tag] = {"sweep_ms_per_image": round(m["sweep"] / n, 3), "single_calls_ms_per_image": round(m["single"] / n, 3),
                    "speedup": round(m["single"] / m["sweep"], 2), "thresholds": len(set(np.float32(fgs + bgs).tolist())),
                    "single_calls": len(fgs) * len(bgs), "same_histogram": same}
        print(tag, res[tag], file=sys.stderr, flush=True)
    m = alternate({"sweep": lambda: [ops.crf_label_sweep(i, c, k, [0.05, 0.30]) for i, c, k, _ in items],
                   "single": lambda: [ops.crf_ir_label(i, c, k, 0.30, 0.05) for i, c, k, _ in items]}, a.reps)
    res["t2"] = {"sweep_ms_per_image": round(m["sweep"] / n, 3), "crf_ir_label_ms_per_image": round(m["single"] / n, 3),
                 "ratio": round(m["sweep"] / m["single"], 3)}
    print("t2", res["t2"], file=sys.stderr, flush=True)
    th = np.unique(np.float32(FG4 + BG4))
    planes8 = [ops.crf_label_sweep(i, c, k, th) for i, c, k, _ in items]
    rng = np.random.RandomState(0)
    planes16 = [torch.from_numpy(np.where(rng.rand(16, *it[3].shape) < 0.5, 0, rng.randint(1, 21, size=(16,) + tuple(it[3].shape)))
                                 .astype(np.uint8)).to(dev) for it in items]
    fi, bi = np.searchsorted(th, np.float32(FG4)), np.searchsorted(th, np.float32(BG4))
    all16 = list(range(16))

    def count(planes, f, b):
        hist = bad = None
        for p, it in zip(planes, items):
            hist, bad = ops.ir_label_confusion(p, f, b, it[3], hist, bad)
    m = alternate({"4x4": lambda: count(planes8, fi, bi), "16x16": lambda: count(planes16, all16, all16)}, a.reps)
    res["count"] = {"grid4x4_us_per_image": round(1e3 * m["4x4"] / n, 2), "grid16x16_random_planes_us_per_image": round(1e3 * m["16x16"] / n, 2)}
    line = json.dumps(res)
    print(line)
    if a.json_out:
        with open(a.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
