#!/usr/bin/env python3
"""Fused against composed segmentation loss on the GPU: milliseconds per forward + backward and peak allocated bytes.
Prints one JSON line and appends it to profiles/seg_loss_bench.json (a JSON list of runs).

    python tools/seg_loss_bench.py [--batch 16] [--classes 21] [--grid 32] [--factor 16] [--iters 20] [--out FILE]

fused    = ops.seg_cross_entropy(logits, label, factor) + backward to the logits (irn_amd/csrc/seg_loss.hip)
composed = F.interpolate(scale_factor=factor, bilinear) -> F.cross_entropy(ignore_index=255) + backward
           (step/train_sem_seg.py composed_loss: what `--seg_loss composed` runs)
Times are device events around one forward + backward, the median of `iters` runs after a warm-up, the two paths
alternating; the peak is that of one warm iteration above what was allocated before it.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default=16, type=int)
    ap.add_argument("--classes", default=21, type=int)
    ap.add_argument("--grid", default=32, type=int)
    ap.add_argument("--factor", default=16, type=int)
    ap.add_argument("--iters", default=20, type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_loss_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "seg_loss_bench needs a GPU"
    import _seg_loss_ref as R
    from irn_amd import ops
    from irn_amd.step.train_sem_seg import composed_loss
    dev = torch.device("cuda", 0)
    b, c, g, f = args.batch, args.classes, args.grid, args.factor
    x, label, _ = R.make_case((b, c, g, g, f, g * f, g * f), seed=1)
    x = x.to(dev).requires_grad_(True)
    label = label.to(dev)

    def fused():
        ops.seg_cross_entropy(x, label, f).backward()

    def composed():
        composed_loss(x, label, f).backward()

    out = {"batch": b, "classes": c, "grid": g, "factor": f, "iters": args.iters, "device": torch.cuda.get_device_name(0)}
    paths = (("fused", fused), ("composed", composed))
    for name, fn in paths:                                   # warm-up, and the peak of one iteration of each
        fn()
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        out[name + "_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    ms = {name: [] for name, _ in paths}
    for _ in range(args.iters):
        for name, fn in paths:
            x.grad = None
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1))
    for name in ms:
        out[name + "_ms"] = round(float(np.median(ms[name])), 3)
        out[name + "_ms_min_max"] = [round(min(ms[name]), 3), round(max(ms[name]), 3)]
    print(json.dumps(out))
    runs = json.load(open(args.out)) if os.path.exists(args.out) else []
    runs.append(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(runs, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
