#!/usr/bin/env python3
"""tune_sem_seg against the steps it replaces, and its counting kernel against the kernels it fuses.  Prints one JSON line
(and writes it to --json-out).

1. Steps, wall time in one process: a synthetic VOC tree of `--images` VOC-size images (irn_amd/synth.py sizes, photos and
   CAMs; ground truth cut from the CAM blobs; an IRNet of seeded random weights).  `tune_sem_seg` over a 3 x 2 x 16 grid
   (96 points) against make_sem_seg_labels + eval_sem_seg for ONE grid point.  Both run the IRNet themselves
   (keep_edges_on_device off: the label step would otherwise leave its boundary maps to the tuning step).  One warm-up of
   each, then `--reps` alternating repeats; medians.
2. Kernels, device events on resident inputs: the walk outputs of one batch of 64 images, `label_sweep_confusion` at 16
   thresholds against `label_epilogue` + `label_confusion` per threshold (16 epilogues, 16 x 64 counts).  Median of 20,
   alternating; the two must give the same matrices.

    python tools/tune_sem_seg_bench.py [--images 64] [--reps 3] [--json-out profiles/tune_sem_seg_bench.json]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from irn_amd import synth  # noqa: E402

BETAS, EXPS = [6.0, 14.0], [6]                      # + the configured 10 / 8: 3 x 2 walks
THRES = [round(0.05 + 0.04 * i, 2) for i in range(16)]       # 0.05 .. 0.65, holds the configured 0.25


def make_tree(root, n):
    """-> [(name, size, keys, cam, gt)]; writes JPEGImages, SegmentationClass, the split, the image list with its
    cls_labels.npy, the CAM files and the IRNet checkpoint under `root`."""
    from irn_amd.net import weights
    items, specs = [], []
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        h, w = synth.voc_image_size(i)
        k = synth.voc_num_classes(i)
        keys, cam = synth.voc_keys(k, i), synth.cam_blobs(k, *synth.grid_of((h, w)), i)
        gt, _ = synth.blob_ground_truth(synth.upsample4(cam, (h, w)), keys, 0.45, 0.35)
        specs.append({"name": name, "photo": synth.photo(h, w, seed=i), "quality": 90, "keys": keys, "cls": gt,
                      "cam": {"keys": torch.from_numpy(keys), "cam": torch.from_numpy(cam)}})
        items.append((name, (h, w), keys, cam, gt))
    synth.write_voc_tree(root, specs, os.path.join(root, "train.txt"), cam_dir=os.path.join(root, "cam"), cls_labels=20)
    torch.save(weights.random_irn_state(2), os.path.join(root, "res50_irn.pth"))
    return items


def step_args(root):
    sys.path.insert(0, ROOT)
    import run_sample
    return run_sample.build_parser().parse_args([
        "--voc12_root", root, "--infer_list", os.path.join(root, "train.txt"), "--num_workers", "8", "--worker_devices", "0",
        "--irn_weights_name", os.path.join(root, "res50_irn.pth"), "--cam_out_dir", os.path.join(root, "cam"),
        "--sem_seg_out_dir", os.path.join(root, "sem"), "--keep_edges_on_device", "0", "--keep_cams_on_device", "0",
        "--tune_beta"] + [str(b) for b in BETAS] + ["--tune_exp_times"] + [str(e) for e in EXPS] + ["--tune_bg_thres"] + [str(t) for t in THRES])


def steps(root, n, reps):
    from irn_amd.step import eval_sem_seg, make_sem_seg_labels, tune_sem_seg
    args = step_args(root)
    os.makedirs(args.sem_seg_out_dir, exist_ok=True)
    out = {}

    def tune():
        with contextlib.redirect_stdout(io.StringIO()):
            out["tune"] = tune_sem_seg.run(args)

    def one_point():
        with contextlib.redirect_stdout(io.StringIO()):
            make_sem_seg_labels.run(args)
            out["eval"] = eval_sem_seg.run(args)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    warm = {"tune_s": round(wall(tune), 3), "one_point_s": round(wall(one_point), 3)}      # solvers found, code objects loaded
    t_tune, t_one = [], []
    for _ in range(reps):
        t_tune.append(wall(tune))
        t_one.append(wall(one_point))
    same = bool(np.array_equal(out["tune"]["iou"], out["eval"]["iou"], equal_nan=True))
    points = len(out["tune"]["grid"])
    tune_s, one_s = float(np.median(t_tune)), float(np.median(t_one))
    return {"images": n, "grid": "%d x %d x %d" % (len(BETAS) + 1, len(EXPS) + 1, len(THRES)), "grid_points": points,
            "first_run": warm, "reps": reps, "tune_sem_seg_s": round(tune_s, 3), "tune_sem_seg_runs_s": [round(t, 3) for t in t_tune],
            "make_plus_eval_one_point_s": round(one_s, 3), "make_plus_eval_runs_s": [round(t, 3) for t in t_one],
            "tune_images_per_s": round(n / tune_s, 1), "one_point_images_per_s": round(n / one_s, 1),
            "grid_by_repeating_the_steps_s": round(points * one_s, 1),
            "configured_point_iou_equal": same, "best": list(out["tune"]["best"]), "best_miou": round(out["tune"]["grid"][out["tune"]["best"]], 6)}


def kernels(items, reps=20):
    from irn_amd import ops
    from irn_amd.misc import indexing
    dev = torch.device("cuda", 0)
    walker = indexing.RandomWalk(5, dev)
    edges = [torch.from_numpy(synth.edge_field(*synth.grid_of(it[1]), i))[None].to(dev) for i, it in enumerate(items)]
    cams = [torch.from_numpy(it[3]).to(dev) for it in items]
    keys = [torch.from_numpy(it[2]).to(dev) for it in items]
    sizes = [it[1] for it in items]
    gts = [torch.from_numpy(it[4]).to(dev) for it in items]
    flat = torch.cat([g.reshape(-1) for g in gts])
    rws = walker(edges, cams, beta=10.0, exp_times=8)
    walker.sync()
    th = ops.eval_thresholds(sorted(THRES), dev)
    res = {}

    def fused():
        hist, bad = ops.label_sweep_confusion(rws, sizes, keys, flat, th)
        res["fused"] = ops.cam_confusion_matrices(hist)[0]

    def composed():
        confs = []
        for t in sorted(THRES):
            labels = ops.label_epilogue(rws, sizes, t, keys=keys)["labels"]
            conf = void = bad = None
            for lab, g in zip(labels, gts):
                conf, void, bad = ops.label_confusion(lab, g, conf, bad, void=void)
            confs.append(conf)
        res["composed"] = torch.stack(confs)

    times = {"fused": [], "composed": []}
    for name, fn in (("fused", fused), ("composed", composed)):
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in (("fused", fused), ("composed", composed)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    walker.close()
    px = sum(h * w for h, w in sizes)
    f, c = float(np.median(times["fused"])), float(np.median(times["composed"]))
    return {"batch": len(items), "thresholds": len(THRES), "pixels": px, "channels": int(sum(it[3].shape[0] for it in items)),
            "reps": reps, "label_sweep_confusion_ms": round(f, 4), "epilogue_plus_confusion_per_threshold_ms": round(c, 4),
            "fused_min_max_ms": [round(min(times["fused"]), 4), round(max(times["fused"]), 4)],
            "composed_min_max_ms": [round(min(times["composed"]), 4), round(max(times["composed"]), 4)],
            "composed_launches": len(THRES) * (3 + len(items)), "fused_launches": 4,
            "note": "events around the host calls: the composed path's time includes enqueueing its launches",
            "matrices_equal": bool(torch.equal(res["fused"], res["composed"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json-out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tune_sem_seg_bench: needs a GPU (nothing is measured without one)")
    torch.cuda.set_device(0)
    warnings.simplefilter("ignore")
    res = {"metric": "tune_sem_seg vs make_sem_seg_labels + eval_sem_seg; label_sweep_confusion vs label_epilogue + label_confusion",
           "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as root:
        items = make_tree(root, a.images)
        res["steps"] = steps(root, a.images, a.reps)
        res["kernels"] = kernels(items[:64])
    line = json.dumps(res)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
