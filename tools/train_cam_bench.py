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

import _train_bench as TB  # noqa: E402


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


def bench_step(args, a, dev, fused_tail=False):
    from irn_amd.net import resnet50 as _r50
    from irn_amd.step import _train, train_cam
    from irn_amd.voc12 import dataloader
    _r50.TRAIN_FUSED_TAIL = bool(fused_tail)
    try:
        torch.manual_seed(0)
        model = train_cam.build_model(args).to(dev).train()
        train, _ = train_cam.make_datasets(args, 0)
        opt = _train.two_rate_optimizer(*model.trainable_parameters(), 0.01, 1e-4, 10 ** 9)

        def step(pack):
            img = _train.device_images(pack, args.cam_crop_size, dev)
            train_cam.train_step(model, opt, img, pack["label"].to(dev, non_blocking=True))

        figures, _ = TB.timed_steps(train, lambda ep: _train.loader(train, a.batch, a.workers, True, ep, dataloader.classification_collate),
                                    step, a.warmup, a.steps, a.batch)
        return {"augment": args.cam_augment, "fused_tail": int(bool(fused_tail)), **figures}
    finally:
        _r50.TRAIN_FUSED_TAIL = False


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
        lst, _ = TB.write_tree(root, a.images, labels="cls")
        args = step_args(root, lst, a, "device")
        raw, _ = train_cam.make_datasets(args, 0)
        if not a.skip_pipeline:
            print(json.dumps({"augment": bench_augment(raw, a, dev)}), flush=True)
            host, _ = train_cam.make_datasets(step_args(root, lst, a, "host"), 0)
            print(json.dumps({"host_pipeline": TB.bench_host_pipeline(raw, host, min(a.images, 64))}), flush=True)
        if not a.skip_step:
            with _tuned.process_mode():
                for augment in () if a.skip_augment_steps else ("device", "host", "device", "host"):   # alternating: the spread shows next to the difference
                    print(json.dumps({"step": bench_step(step_args(root, lst, a, augment), a, dev)}), flush=True)
                for fused in (0, 1) * a.fused_tail_rounds:
                    print(json.dumps({"step": bench_step(step_args(root, lst, a, "device"), a, dev, fused)}), flush=True)


if __name__ == "__main__":
    main()
