#!/usr/bin/env python3
"""Multi-scale segmentation inference: `ops.seg_fuse` against the same thing composed from torch ops, and what
--seg_infer_scales and --seg_crf_iters cost in infer_sem_seg.  Prints one JSON line and appends it to --json-out (every run is
kept).

1. The call, device events on resident inputs: a 375x500 image, 21 classes, stride 16, the scales 0.5 / 0.75 / 1 / 1.25 / 1.5
   (random logit maps of ceil(Hs / 16) cells).  `seg_fuse` (label only, and label + probabilities) against the composed path:
   per scale F.interpolate(size = the image's, bilinear, align_corners = False), softmax, add; then arg-max.  One warm-up of
   each, then the paths alternate; median, minimum and maximum of `--reps` calls, and the peak allocated memory of one call of
   each above what is resident.  The composed path is no bit-level reference: F.interpolate maps output to input by h / H of
   the padded map, `seg_fuse` by Hs / (stride * H); the labels' disagreement is reported, not bounded.
2. The step (`--step-images` > 0), wall time of infer_sem_seg in this process on synthetic VOC-size photos under seeded random
   weights: one scale (the default path), the five scales, and the five scales with --seg_crf_iters 10; a warm-up run of each,
   then `--step-reps` runs alternating, as images/s.
3. The default path against another checkout (`--parent-root DIR`, a built tree of the parent commit): the default-mode step
   in a fresh process of each tree, alternating, `--step-reps` runs each after a warm-up run inside the process.  The yardstick
   is the spread of the parent's own runs.

    python tools/seg_infer_bench.py [--reps 20] [--step-images 64] [--step-reps 3] [--parent-root DIR]
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from irn_amd import ops, synth  # noqa: E402

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5)
H, W, C, STRIDE = 375, 500, 21, 16

CHILD = """
import contextlib, io, sys, time
import torch
import run_train_seg
out = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        run_train_seg.main(sys.argv[1:])
    torch.cuda.synchronize()
    out.append(time.perf_counter() - t0)
print("SECONDS %.6f" % out[1])
"""


def _stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def alternate(paths, reps):
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
    return ms


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def call(reps, dev):
    rng = np.random.RandomState(0)
    sizes = [ops.rescale_size(H, W, s) for s in SCALES]
    maps = [torch.from_numpy((3 * rng.standard_normal((C, -(-hs // STRIDE), -(-ws // STRIDE)))).astype(np.float32)).to(dev)
            for hs, ws in sizes]

    def composed():
        total = None
        for m in maps:
            p = torch.softmax(F.interpolate(m[None], size=(H, W), mode="bilinear", align_corners=False)[0], 0)
            total = p if total is None else total + p
        return torch.argmax(total, 0).to(torch.uint8)

    paths = {"seg_fuse_label": lambda: ops.seg_fuse(maps, sizes, STRIDE, (H, W)),
             "seg_fuse_label_prob": lambda: ops.seg_fuse(maps, sizes, STRIDE, (H, W), want_label=True, want_prob=True),
             "composed_torch": composed}
    ms = alternate(paths, reps)
    res = {"image": [H, W], "classes": C, "scales": list(SCALES), "stride": STRIDE, "reps": reps,
           "ms": {k: _stats(v) for k, v in ms.items()}, "peak_bytes": {k: peak_bytes(fn) for k, fn in paths.items()}}
    res["speedup_label_vs_composed"] = round(res["ms"]["composed_torch"]["median"] / res["ms"]["seg_fuse_label"]["median"], 2)
    res["labels_differing_from_composed"] = int((paths["seg_fuse_label"]()[0] != composed()).sum().item())
    return res


def make_tree(root, n):
    from irn_amd.net import weights
    specs = []
    for i in range(n):
        h, w = synth.voc_image_size(i)
        specs.append({"name": "2008_%06d" % (i + 1), "photo": synth.photo(h, w, seed=i), "quality": 90, "keys": [0],
                      "cls": np.zeros((h, w), np.uint8)})
    synth.write_voc_tree(root, specs, os.path.join(root, "train.txt"))
    os.makedirs(os.path.join(root, "sess"), exist_ok=True)
    torch.save(weights.random_seg_state(), os.path.join(root, "sess", "res50_seg.pth"))


def step_argv(root, tag, extra=()):
    return ["--voc12_root", root, "--infer_list", os.path.join(root, "train.txt"), "--train_list", os.path.join(root, "train.txt"),
            "--num_workers", "8", "--seg_weights_name", os.path.join(root, "sess", "res50_seg"), "--train_sem_seg_pass", "False",
            "--infer_sem_seg_pass", "True", "--seg_pred_dir", os.path.join(root, "pred_" + tag),
            "--log_name", os.path.join(root, "log_" + tag)] + list(extra)


def steps(root, n, reps):
    import run_train_seg
    modes = {"one_scale": [], "five_scales": ["--seg_infer_scales"] + [str(s) for s in SCALES],
             "five_scales_crf10": ["--seg_infer_scales"] + [str(s) for s in SCALES] + ["--seg_crf_iters", "10"]}

    def wall(tag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            run_train_seg.main(step_argv(root, tag, modes[tag]))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    first = {tag: round(wall(tag), 3) for tag in modes}                      # solvers found, code objects loaded
    runs = {tag: [] for tag in modes}
    for _ in range(reps):
        for tag in modes:
            runs[tag].append(wall(tag))
    return {"images": n, "reps": reps, "first_run_s": first, "runs_s": {t: [round(v, 3) for v in r] for t, r in runs.items()},
            "images_per_s": {t: round(n / float(np.median(r)), 1) for t, r in runs.items()}}


def parent_ab(root, n, reps, parent_root):
    def run(tree):
        env = dict(os.environ, PYTHONPATH=tree)
        done = subprocess.run([sys.executable, "-c", CHILD] + step_argv(root, "ab"), cwd=tree, env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, timeout=600)
        if done.returncode != 0:
            raise RuntimeError("the default-mode step failed in %s:\n%s" % (tree, done.stdout[-2000:]))
        return float([ln for ln in done.stdout.splitlines() if ln.startswith("SECONDS ")][-1].split()[1])

    parent, this = [], []
    for _ in range(reps):
        parent.append(run(parent_root))
        this.append(run(ROOT))
    lo, hi = min(parent), max(parent)
    med = float(np.median(this))
    return {"images": n, "parent_runs_s": [round(v, 3) for v in parent], "this_runs_s": [round(v, 3) for v in this],
            "parent_images_per_s": round(n / float(np.median(parent)), 1), "this_images_per_s": round(n / med, 1),
            "this_median_within_parent_spread": bool(lo <= med <= hi),
            "deviation_from_parent_spread_s": round(0.0 if lo <= med <= hi else (med - hi if med > hi else med - lo), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-images", type=int, default=64)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: the default path is timed in both")
    ap.add_argument("--json-out", default=os.path.join(ROOT, "profiles", "seg_infer_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_infer_bench: needs a GPU (nothing is measured without one)")
    torch.cuda.set_device(0)
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    res = {"metric": "seg_fuse vs the composed torch path, ms per call; infer_sem_seg images/s at one scale, five, five + CRF 10",
           "device": torch.cuda.get_device_name(0), "call": call(a.reps, dev)}
    print("call", res["call"], file=sys.stderr, flush=True)
    if a.step_images > 0:
        with tempfile.TemporaryDirectory() as root:
            make_tree(root, a.step_images)
            res["steps"] = steps(root, a.step_images, a.step_reps)
            print("steps", res["steps"], file=sys.stderr, flush=True)
            if a.parent_root:
                res["default_path_vs_parent"] = parent_ab(root, a.step_images, a.step_reps, os.path.abspath(a.parent_root))
    line = json.dumps(res)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
