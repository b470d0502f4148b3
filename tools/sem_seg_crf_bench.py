#!/usr/bin/env python3
"""The score-seeded dense CRF behind `--sem_seg_crf_iters`: its call against the label-seeded one, and what the
flag costs and buys in the steps.  Prints one JSON line and appends it to --json-out (every run is kept).

1. Calls, device events on resident inputs: `--images` synthetic VOC-size photos with CAMs as scores, as tools/crf_bench.py
   makes them.  One measurement is a pass over all images; after a warm-up pass of each the paths alternate; median, minimum
   and maximum of `--reps` passes, as ms per image.
     (a) `crf_score_sweep` at ONE threshold against `crf_ir_label`: the same two lattices, k+1 channels against 2(k+1)
     (b) `crf_score_sweep` at 16 thresholds against 16 single-threshold calls (the lattices built once against 16 times)
2. Steps (`--step-images` > 0), wall time in one process on the tree of tools/tune_sem_seg_bench.py (photos, CAM blobs, ground
   truth cut from the blobs, an IRNet of seeded random weights): make_sem_seg_labels with the flag off and with T = 10,
   alternating, as images/s, and the CRF's share of the step; eval_sem_seg (mIoU, and Boundary IoU at ratio 0.02) on both
   label sets at the configured threshold and at tune_sem_seg's best one of 16.  Synthetic blobs under random IRNet weights
   predict nothing about VOC: the scores are for orientation only.

    python tools/sem_seg_crf_bench.py [--images 64] [--reps 20] [--step-images 32] [--step-reps 3]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from irn_amd import ops, synth  # noqa: E402

THRES16 = [round(0.05 + 0.04 * i, 2) for i in range(16)]         # 0.05 .. 0.65, holds the configured 0.25


def _items(n, dev):
    out = []
    for s in range(n):
        h, w = synth.voc_image_size(s)
        k = max(synth.voc_num_classes(s), 1)
        out.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                         for a in (synth.photo(h, w, seed=s), synth.cam_blobs(k, h, w, seed=s), synth.voc_keys(k, s))))
    return out


def alternate(paths, reps):
    """{name: fn} -> {name: [ms of each pass]}, device events, one warm-up each, then alternating."""
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


def _stats(ms, n):
    return {"median": round(float(np.median(ms)) / n, 4), "min": round(min(ms) / n, 4), "max": round(max(ms) / n, 4)}


def calls(n, reps, dev):
    items = _items(n, dev)
    m = alternate({"score": lambda: [ops.crf_score_sweep(i, c, k, [0.25]) for i, c, k in items],
                   "ir": lambda: [ops.crf_ir_label(i, c, k, 0.30, 0.05) for i, c, k in items]}, reps)
    score, ir = _stats(m["score"], n), _stats(m["ir"], n)
    res = {"images": n, "reps": reps, "classes_mean": round(float(np.mean([int(k.numel()) for _, _, k in items])), 2),
           "crf_score_sweep_t1_ms_per_image": score, "crf_ir_label_ms_per_image": ir,
           "ratio_of_medians": round(score["median"] / ir["median"], 3),
           "score_median_within_ir_spread": bool(score["median"] <= ir["median"] + (ir["max"] - ir["min"]))}
    few = max(1, min(reps, 5))
    m = alternate({"sweep": lambda: [ops.crf_score_sweep(i, c, k, THRES16) for i, c, k in items],
                   "single": lambda: [ops.crf_score_sweep(i, c, k, [t]) for i, c, k in items for t in THRES16]}, few)
    res["sweep16"] = {"reps": few, "sweep_ms_per_image": _stats(m["sweep"], n), "single_calls_ms_per_image": _stats(m["single"], n),
                      "speedup": round(float(np.median(m["single"]) / np.median(m["sweep"])), 2)}
    return res


def steps(root, n, reps):
    import run_sample
    import tune_sem_seg_bench as B
    from irn_amd.step import eval_sem_seg, make_sem_seg_labels, tune_sem_seg
    B.make_tree(root, n)

    def args(t, sem, thres=0.25, extra=()):
        return run_sample.build_parser().parse_args([
            "--voc12_root", root, "--infer_list", os.path.join(root, "train.txt"), "--num_workers", "8", "--worker_devices", "0",
            "--irn_weights_name", os.path.join(root, "res50_irn.pth"), "--cam_out_dir", os.path.join(root, "cam"),
            "--sem_seg_out_dir", os.path.join(root, sem), "--keep_edges_on_device", "0", "--keep_cams_on_device", "0",
            "--sem_seg_crf_iters", str(t), "--sem_seg_bg_thres", str(thres), "--boundary_iou_ratio", "0.02"] + list(extra))

    def quiet(fn, a):
        os.makedirs(a.sem_seg_out_dir, exist_ok=True)
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(a)

    def wall(a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        quiet(make_sem_seg_labels.run, a)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    off, on = args(0, "sem_off"), args(10, "sem_on")
    first = {"off_s": round(wall(off), 3), "on_s": round(wall(on), 3)}          # solvers found, code objects loaded
    t_off, t_on = [], []
    for _ in range(reps):
        t_off.append(wall(off))
        t_on.append(wall(on))
    m_off, m_on = float(np.median(t_off)), float(np.median(t_on))
    res = {"images": n, "reps": reps, "first_run": first, "flag_off_runs_s": [round(t, 3) for t in t_off],
           "flag_on_runs_s": [round(t, 3) for t in t_on], "flag_off_images_per_s": round(n / m_off, 1),
           "flag_on_images_per_s": round(n / m_on, 1), "crf_share_of_step": round(max(m_on - m_off, 0.0) / m_on, 3)}

    def scores(a):
        s = quiet(eval_sem_seg.run, a)
        return {"miou": round(float(s["miou"]), 6), "mbiou": round(float(s["mbiou"]), 6)}

    res["configured_thres_0.25"] = {"t0": scores(off), "t10": scores(on)}
    sweep = ["--tune_bg_thres"] + [str(t) for t in THRES16]
    res["tuned"] = {}
    for tag, t in (("t0", 0), ("t10", 10)):
        best = quiet(tune_sem_seg.run, args(t, "sem_tune", extra=sweep))["best"]
        a = args(t, "sem_best_" + tag, thres=best[2])
        quiet(make_sem_seg_labels.run, a)
        res["tuned"][tag] = dict(scores(a), thres=best[2])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-images", type=int, default=32)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--json-out", default=os.path.join(ROOT, "profiles", "sem_seg_crf_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sem_seg_crf_bench: needs a GPU (nothing is measured without one)")
    torch.cuda.set_device(0)
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    res = {"metric": "crf_score_sweep vs crf_ir_label, ms per image; make_sem_seg_labels with --sem_seg_crf_iters 0 / 10",
           "device": torch.cuda.get_device_name(0), "calls": calls(a.images, a.reps, dev)}
    print("calls", res["calls"], file=sys.stderr, flush=True)
    if a.step_images > 0:
        with tempfile.TemporaryDirectory() as root:
            res["steps"] = steps(root, a.step_images, a.step_reps)
    line = json.dumps(res)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
