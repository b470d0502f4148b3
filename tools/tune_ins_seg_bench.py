#!/usr/bin/env python3
"""tune_ins_seg against the steps it replaces, and its counting call against the calls it replaces.  Prints one JSON line
(and writes it to --json-out).

1. Steps, wall time in one process: a synthetic VOC tree of `--images` VOC-size images (irn_amd/synth.py sizes, photos and
   CAMs; class and instance ground truth cut from the CAM blobs, one instance per class; an IRNet of seeded random weights).
   `tune_ins_seg` over a 3 x 2 x 8 grid (48 points) against make_ins_seg_labels + eval_ins_seg for ONE grid point.  Both run
   the IRNet themselves (keep_edges_on_device off).  One warm-up of each, then `--reps` alternating repeats; medians.
2. Calls, device events on resident inputs: the label-epilogue outputs of one batch of 32 images, `detection_overlap_batch`
   against `detect_instance_batch` + `mask_overlap` per image (dense masks to the host and back, as the two steps move
   them).  Median of 20, alternating; the two must give the same counts.

    python tools/tune_ins_seg_bench.py [--images 64] [--reps 9] [--json-out profiles/tune_ins_seg_bench.json]
"""
import argparse
import contextlib
import io
import json
import os
import shutil
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
THRES = [round(0.05 + 0.1 * i, 2) for i in range(8)]         # 0.05 .. 0.75, holds the configured 0.25


def make_tree(root, n):
    """-> [(name, size, keys, cam, inst_map, n_inst)]; writes JPEGImages, SegmentationClass, SegmentationObject, the split,
    the image list with its cls_labels.npy, the CAM files and the IRNet checkpoint under `root`."""
    from irn_amd.net import weights
    items, specs = [], []
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        h, w = synth.voc_image_size(i)
        k = synth.voc_num_classes(i)
        keys, cam = synth.voc_keys(k, i), synth.cam_blobs(k, *synth.grid_of((h, w)), i)
        cls, obj = synth.blob_ground_truth(synth.upsample4(cam, (h, w)), keys, 0.45, 0.35, obj_ids=np.arange(k) + 1)
        specs.append({"name": name, "photo": synth.photo(h, w, seed=i), "quality": 90, "keys": keys, "cls": cls, "obj": obj,
                      "cam": {"keys": torch.from_numpy(keys), "cam": torch.from_numpy(cam)}})
        ids = [v for v in np.unique(obj) if v not in (0, 255)]
        inst = np.zeros((h, w), np.uint8)
        for g, v in enumerate(ids):
            inst[obj == v] = g + 1
        items.append((name, (h, w), keys, cam, inst, len(ids)))
    synth.write_voc_tree(root, specs, os.path.join(root, "train.txt"), cam_dir=os.path.join(root, "cam"), cls_labels=20)
    torch.save(weights.random_irn_state(2), os.path.join(root, "res50_irn.pth"))
    return items


def step_args(root):
    import run_sample
    return run_sample.build_parser().parse_args([
        "--voc12_root", root, "--infer_list", os.path.join(root, "train.txt"), "--num_workers", "8", "--worker_devices", "0",
        "--irn_weights_name", os.path.join(root, "res50_irn.pth"), "--cam_out_dir", os.path.join(root, "cam"),
        "--ins_seg_out_dir", os.path.join(root, "ins"), "--keep_edges_on_device", "0", "--keep_cams_on_device", "0",
        "--tune_beta"] + [str(b) for b in BETAS] + ["--tune_exp_times"] + [str(e) for e in EXPS] + ["--tune_ins_bg_thres"] + [str(t) for t in THRES])


def steps(root, n, reps):
    from irn_amd.step import eval_ins_seg, make_ins_seg_labels, tune_ins_seg
    args = step_args(root)
    out = {}

    def tune():
        with contextlib.redirect_stdout(io.StringIO()):
            out["tune"] = tune_ins_seg.run(args)

    def one_point():
        shutil.rmtree(args.ins_seg_out_dir, ignore_errors=True)
        os.makedirs(args.ins_seg_out_dir)
        with contextlib.redirect_stdout(io.StringIO()):
            make_ins_seg_labels.run(args)
            out["files"] = len(os.listdir(args.ins_seg_out_dir))
            # eval_ins_seg needs a file per image; an image the label step found nothing in has none
            out["eval"] = eval_ins_seg.run(args) if out["files"] == n else None

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
    from irn_amd.step import _common
    _common.shutdown_workers()                      # the label step's worker served every repeat
    same = None if out["eval"] is None else bool(np.array_equal(out["tune"]["ap"], out["eval"]["ap"], equal_nan=True))
    points = len(out["tune"]["grid"])
    tune_s, one_s = float(np.median(t_tune)), float(np.median(t_one))
    return {"images": n, "grid": "%d x %d x %d" % (len(BETAS) + 1, len(EXPS) + 1, len(THRES)), "grid_points": points,
            "first_run": warm, "reps": reps, "tune_ins_seg_s": round(tune_s, 3), "tune_ins_seg_runs_s": [round(t, 3) for t in t_tune],
            "make_plus_eval_one_point_s": round(one_s, 3), "make_plus_eval_runs_s": [round(t, 3) for t in t_one],
            "detection_files_of_one_point": out["files"], "eval_ins_seg_ran": out["eval"] is not None,
            "grid_by_repeating_the_steps_s": round(points * one_s, 1),
            "configured_point_ap_equal": same, "best": list(out["tune"]["best"]), "best_map": round(float(out["tune"]["grid"][out["tune"]["best"]]), 6)}


def calls(items, reps=20):
    from irn_amd import ops
    from irn_amd.misc import indexing
    dev = torch.device("cuda", 0)
    walker = indexing.RandomWalk(5, dev)
    edges = [torch.from_numpy(synth.edge_field(*synth.grid_of(it[1]), i))[None].to(dev) for i, it in enumerate(items)]
    cams = [torch.from_numpy(it[3]).to(dev) for it in items]
    sizes = [it[1] for it in items]
    insts = [torch.from_numpy(it[4]).to(dev) for it in items]
    gs = [it[5] for it in items]
    rws = walker(edges, cams, beta=10.0, exp_times=8)
    walker.sync()
    ep = ops.label_epilogue(rws, sizes, 0.25, want_labels=False, want_argmax=True, want_rw_up=True)
    n_ch = [it[3].shape[0] for it in items]
    class_ids = [it[2] for it in items]
    min_area = [h * w * 0.01 for h, w in sizes]
    res = {}

    def from_map():
        res["map"] = ops.detection_overlap_batch(ep["rw_up"], ep["argmax"], class_ids, n_ch, min_area, insts, gs)

    def dense():
        out = []
        dets = ops.detect_instance_batch(ep["rw_up"], ep["argmax"], class_ids, n_ch, min_area)
        for det, inst, g, (h, w) in zip(dets, insts, gs, sizes):
            mask = np.zeros((0, h, w), bool) if isinstance(det, Exception) else det["mask"]
            inter, ap, ag = ops.mask_overlap(torch.from_numpy(np.ascontiguousarray(mask)).to(dev), inst, g)
            out.append((inter, ap, ag))
        res["dense"] = [tuple(t.cpu().numpy() for t in o) for o in out]

    times = {"from_map": [], "dense": []}
    for name, fn in (("from_map", from_map), ("dense", dense)):
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in (("from_map", from_map), ("dense", dense)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    walker.close()
    equal = all(np.array_equal(r["inter"], d[0]) and np.array_equal(r["area_pred"], d[1]) and np.array_equal(r["area_gt"], d[2])
                for r, d in zip(res["map"], res["dense"]))
    f, c = float(np.median(times["from_map"])), float(np.median(times["dense"]))
    return {"batch": len(items), "pixels": sum(h * w for h, w in sizes), "detections": int(sum(len(r["pred_score"]) for r in res["map"])),
            "gt_instances": int(sum(gs)), "reps": reps, "detection_overlap_batch_ms": round(f, 4),
            "detect_instance_batch_plus_mask_overlap_ms": round(c, 4),
            "from_map_min_max_ms": [round(min(times["from_map"]), 4), round(max(times["from_map"]), 4)],
            "dense_min_max_ms": [round(min(times["dense"]), 4), round(max(times["dense"]), 4)],
            "note": "events around the host calls: both include their read-backs; the dense path also moves its masks to the host "
                    "and back, as make_ins_seg_labels and eval_ins_seg do through their files",
            "counts_equal": bool(equal)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json-out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tune_ins_seg_bench: needs a GPU (nothing is measured without one)")
    torch.cuda.set_device(0)
    warnings.simplefilter("ignore")
    res = {"metric": "tune_ins_seg vs make_ins_seg_labels + eval_ins_seg; detection_overlap_batch vs detect_instance_batch + mask_overlap",
           "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as root:
        items = make_tree(root, a.images)
        res["steps"] = steps(root, a.images, a.reps)
        res["calls"] = calls(items[:32])
    line = json.dumps(res)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
