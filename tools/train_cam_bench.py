#!/usr/bin/env python3
"""The CAM training step's input pipeline and its step rate on synthetic VOC-size images.  Prints one JSON line per section.

    python tools/train_cam_bench.py [--images 128] [--batch 16] [--reps 30] [--warmup 5] [--steps 20] [--workers 8]

`augment`: `ops.augment_batch` on batches of `--batch` decoded images held on the host (what the step does: staging, one
upload, two launches) — the device time between two events around the call and the host time of the call, median over
`--reps` calls after one warm call per batch; and the same with the images already on the device (the kernels and the
device-side packing alone).  `host_pipeline`: the reference's PIL / numpy augmentation of one decoded image on one CPU
thread, median per image.  `step`: images/s of `train_cam`'s own loop (loader with `--workers` processes, batch on the
device, forward, backward, update) over `--steps` steps after `--warmup`, once with `--cam_augment device` and once with
`host`; the clock stops behind a device synchronise.  `--fused_tail_rounds N` adds N pairs of the same `step` section with the
trained stages' fused training tail off and on (`resnet50.TRAIN_FUSED_TAIL`, run_train_cam.py --cam_fused_tail), alternating,
`--cam_augment device`; each line carries the peak of allocated device memory.  `--skip_pipeline` / `--skip_augment_steps`
leave the input-pipeline sections / the device-host pairs out.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from irn_amd import synth  # noqa: E402


def write_tree(root, n):
    from PIL import Image
    os.makedirs(os.path.join(root, "JPEGImages"), exist_ok=True)
    names, labels = [], {}
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        h, w = synth.voc_image_size(i)
        Image.fromarray(synth.photo(h, w, seed=i)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=90)
        lab = np.zeros(20, np.float32)
        lab[synth.voc_keys(synth.voc_num_classes(i), i)] = 1
        labels[int(name.replace("_", ""))] = lab
        names.append(name)
    lst = os.path.join(root, "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(names) + "\n")
    np.save(os.path.join(root, "cls_labels.npy"), labels, allow_pickle=True)
    return lst


def step_args(root, lst, a, augment):
    import run_train_cam
    return run_train_cam.build_parser().parse_args([
        "--voc12_root", root, "--train_list", lst, "--val_list", lst, "--cam_batch_size", str(a.batch), "--num_workers", str(a.workers),
        "--cam_augment", augment, "--cam_num_epoches", "1000000"])


def bench_augment(dataset, a, dev):
    from irn_amd import ops
    crop = dataset.crop_size
    batches = []
    for s in range(0, len(dataset) - a.batch + 1, a.batch):
        items = [dataset[i] for i in range(s, s + a.batch)]
        batches.append(([it["img"] for it in items], [it["aug"] for it in items]))
    out = {"batch": a.batch, "crop": crop, "upload_bytes_per_image": int(np.mean([im.numel() for b in batches for im in b[0]])),
           "float_bytes_per_image": 3 * crop * crop * 4}
    for where in ("host", "device"):
        dev_ms, host_ms = [], []
        for imgs, params in batches:
            src = imgs if where == "host" else [im.to(dev) for im in imgs]
            ops.augment_batch(src, params, crop, device=dev)                         # warm: code loaded, buffers grown
        torch.cuda.synchronize()
        for r in range(a.reps):
            imgs, params = batches[r % len(batches)]
            src = imgs if where == "host" else [im.to(dev) for im in imgs]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            ops.augment_batch(src, params, crop, device=dev)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
            host_ms.append((t1 - t0) * 1e3)
        out["%s_images" % where] = {"device_ms_median": statistics.median(dev_ms), "device_ms_min": min(dev_ms),
                                    "device_ms_max": max(dev_ms), "host_call_ms_median": statistics.median(host_ms)}
    return out


def bench_host_pipeline(raw, host, n):
    """The worker's share of a host item beyond the JPEG decode both forms pay: item(raw=False) - item(raw=True)."""
    t_raw, t_host = [], []
    for i in range(n):
        t0 = time.perf_counter()
        raw[i]
        t1 = time.perf_counter()
        host[i]
        t2 = time.perf_counter()
        t_raw.append((t1 - t0) * 1e3)
        t_host.append((t2 - t1) * 1e3)
    return {"images": n, "decode_only_ms_median": statistics.median(t_raw), "decode_and_augment_ms_median": statistics.median(t_host)}


def bench_step(args, a, dev, fused_tail=False):
    from irn_amd.misc import torchutils
    from irn_amd.net import resnet50 as _r50
    from irn_amd.step import train_cam
    _r50.TRAIN_FUSED_TAIL = bool(fused_tail)
    try:
        return _bench_step(args, a, dev, torchutils, train_cam, bool(fused_tail))
    finally:
        _r50.TRAIN_FUSED_TAIL = False


def _bench_step(args, a, dev, torchutils, train_cam, fused_tail):
    torch.manual_seed(0)
    torch.cuda.reset_peak_memory_stats()
    model = train_cam.build_model(args).to(dev).train()
    train, _ = train_cam.make_datasets(args, 0)
    backbone, new = model.trainable_parameters()
    opt = torchutils.PolyOptimizer([{"params": backbone, "lr": 0.01, "weight_decay": 1e-4}, {"params": new, "lr": 0.1, "weight_decay": 1e-4}],
                                   lr=0.01, weight_decay=1e-4, max_step=10 ** 9)
    done, t0 = 0, None
    ep = 0
    while done < a.warmup + a.steps:
        train.set_epoch(ep)
        for pack in train_cam._loader(train, args, True, ep):
            if done == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            img = train_cam.device_batch(pack, args.cam_crop_size, dev)
            train_cam.train_step(model, opt, img, pack["label"].to(dev, non_blocking=True))
            done += 1
            if done == a.warmup + a.steps:
                break
        ep += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"augment": args.cam_augment, "fused_tail": int(fused_tail), "steps": a.steps, "seconds": dt,
            "images_per_s": a.steps * a.batch / dt, "ms_per_step": dt / a.steps * 1e3,
            "max_memory_allocated_mb": torch.cuda.max_memory_allocated() / 2 ** 20}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--images", default=128, type=int)
    p.add_argument("--batch", default=16, type=int)
    p.add_argument("--reps", default=30, type=int)
    p.add_argument("--warmup", default=5, type=int)
    p.add_argument("--steps", default=20, type=int)
    p.add_argument("--workers", default=8, type=int)
    p.add_argument("--skip_step", action="store_true", help="the input pipeline only")
    p.add_argument("--skip_pipeline", action="store_true", help="no `augment` / `host_pipeline` sections")
    p.add_argument("--skip_augment_steps", action="store_true", help="no device / host pairs of the `step` section")
    p.add_argument("--fused_tail_rounds", default=0, type=int, help="pairs of the `step` section with the fused training tail off / on")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_cam_bench needs a GPU")
    from irn_amd import _tuned
    from irn_amd.step import train_cam
    dev = torch.device("cuda", torch.cuda.current_device())
    with tempfile.TemporaryDirectory() as root:
        lst = write_tree(root, a.images)
        args = step_args(root, lst, a, "device")
        raw, _ = train_cam.make_datasets(args, 0)
        if not a.skip_pipeline:
            print(json.dumps({"augment": bench_augment(raw, a, dev)}), flush=True)
            host, _ = train_cam.make_datasets(step_args(root, lst, a, "host"), 0)
            print(json.dumps({"host_pipeline": bench_host_pipeline(raw, host, min(a.images, 64))}), flush=True)
        if not a.skip_step:
            with _tuned.process_mode():
                for augment in () if a.skip_augment_steps else ("device", "host", "device", "host"):   # alternating: the spread shows next to the difference
                    print(json.dumps({"step": bench_step(step_args(root, lst, a, augment), a, dev)}), flush=True)
                for fused in (0, 1) * a.fused_tail_rounds:
                    print(json.dumps({"step": bench_step(step_args(root, lst, a, "device"), a, dev, fused)}), flush=True)


if __name__ == "__main__":
    main()
