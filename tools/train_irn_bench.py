#!/usr/bin/env python3
"""The IRNet training step's input pipeline and its step rate on synthetic VOC-size images.  Prints one JSON line per section.

    python tools/train_irn_bench.py [--images 128] [--batch 32] [--crop 512] [--reps 20] [--warmup 3] [--steps 20] [--workers 8]

`augment_pair`: `ops.augment_pair_batch` on batches of `--batch` decoded images and IR label maps held on the host (what the
step does: staging, one upload, three launches) — the device time between two events around the call and the host time of
the call, median over `--reps` calls after one warm call per batch; and the same with the inputs already on the device (the
kernels and the device-side packing alone).  `host_pipeline`: the PIL / numpy augmentation of one decoded pair on one CPU
thread, median per image.  `step`: images/s of `train_irn`'s own loop (loader with `--workers` processes, batch on the device,
forward, fused loss, backward, update) over `--steps` steps after `--warmup` of ONE pass over the list (each image is named
several times) — the model is built, MIOpen's first-use searches have run and the loader's workers have started before the
clock starts — with `--irn_augment device` and `host` alternating `--rounds` times; the clock stops behind a device
synchronise.  `--irn_trunk autograd` (default) / `inference` / `both` chooses the trunk of the step (run_train.py --irn_trunk):
with `both` every round runs the augment modes given by `--augments` once per trunk mode, alternating.  `inference` and `both`
set MIOpen up as `train_irn.run` does for `--irn_trunk inference` (`_tuned.miopen_setup`, before the model is built) — for the
whole process, so the default path's own figure is that of a run with `--irn_trunk autograd`.  Every `step` line carries the
trunk passes it counted by layout (`resnet50.PASS_STATS`) and the peak of allocated device memory.  `--skip_pipeline` leaves
the input-pipeline sections out.  Needs a GPU: there is no fallback.
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


def step_args(root, lst, label_dir, a, augment):
    import run_train
    return run_train.build_parser().parse_args([
        "--voc12_root", root, "--train_list", lst, "--infer_list", lst, "--ir_label_out_dir", label_dir, "--irn_batch_size", str(a.batch),
        "--irn_crop_size", str(a.crop), "--num_workers", str(a.workers), "--irn_augment", augment, "--irn_num_epoches", "1000000"])


def bench_augment(dataset, a, dev):
    from irn_amd import ops
    crop = dataset.crop_size
    batches = []
    for s in range(0, a.images - a.batch + 1, a.batch):
        items = [dataset[i] for i in range(s, s + a.batch)]
        batches.append(([it["img"] for it in items], [it["label_map"] for it in items], [it["aug"] for it in items]))
    out = {"batch": a.batch, "crop": crop, "reduce": 4,
           "upload_bytes_per_image": int(np.mean([im.numel() + lb.numel() for b in batches for im, lb in zip(b[0], b[1])])),
           "host_path_bytes_per_image": 3 * crop * crop * 4 + (crop // 4) ** 2}
    for where in ("host", "device"):
        place = (lambda ts: ts) if where == "host" else (lambda ts: [t.to(dev) for t in ts])
        dev_ms, host_ms = [], []
        for imgs, labs, params in batches:
            ops.augment_pair_batch(place(imgs), place(labs), params, crop, device=dev)      # warm: code loaded, buffers grown
        torch.cuda.synchronize()
        for r in range(a.reps):
            imgs, labs, params = batches[r % len(batches)]
            imgs, labs = place(imgs), place(labs)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            ops.augment_pair_batch(imgs, labs, params, crop, device=dev)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
            host_ms.append((t1 - t0) * 1e3)
        out["%s_inputs" % where] = {"device_ms_median": statistics.median(dev_ms), "device_ms_min": min(dev_ms),
                                    "device_ms_max": max(dev_ms), "host_call_ms_median": statistics.median(host_ms)}
    return out


def bench_step(args, a, dev, model, optimizer, trunk="autograd"):
    from irn_amd.net import resnet50 as _r50
    from irn_amd.step import _train, train_irn
    train, _ = train_irn.make_datasets(args, 0)
    before = {k: _r50.PASS_STATS[k] for k in ("channels_last", "nchw", "pad_rows")}
    assert len(train) >= (a.warmup + a.steps) * a.batch          # one pass: the loader's start lies in the warm-up

    def step(pack):
        img, label = _train.device_pair(pack, args.irn_crop_size, dev, reduce=4)
        train_irn.train_step(model, optimizer, img, label, trunk)

    figures, _ = TB.timed_steps(train, lambda ep: _train.loader(train, a.batch, a.workers, True, ep, train_irn.collate(train)),
                                step, a.warmup, a.steps, a.batch)
    train_irn.check_split_overflow(trunk)
    return {"augment": args.irn_augment, "irn_trunk": trunk, "workers": a.workers, **figures,
            "trunk_passes": {k: _r50.PASS_STATS[k] - before[k] for k in before}}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--images", default=128, type=int)
    p.add_argument("--batch", default=32, type=int)
    p.add_argument("--crop", default=512, type=int)
    p.add_argument("--reps", default=20, type=int)
    p.add_argument("--warmup", default=3, type=int)
    p.add_argument("--steps", default=20, type=int)
    p.add_argument("--workers", default=8, type=int)
    p.add_argument("--rounds", default=2, type=int, help="device / host pairs of the step section: the spread shows next to the difference")
    p.add_argument("--skip_step", action="store_true", help="the input pipeline only")
    p.add_argument("--skip_pipeline", action="store_true", help="no `augment_pair` / `host_pipeline` sections")
    p.add_argument("--irn_trunk", default="autograd", choices=("autograd", "inference", "both"))
    p.add_argument("--augments", default=["device", "host"], nargs="+", choices=("device", "host"))
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_irn_bench needs a GPU")
    from irn_amd import _tuned
    from irn_amd.misc import indexing
    from irn_amd.step import _train, train_irn
    dev = torch.device("cuda", torch.cuda.current_device())
    with tempfile.TemporaryDirectory() as root:
        lst, label_dir = TB.write_tree(root, a.images, labels="ir", repeat=-(-(a.warmup + a.steps) * a.batch // a.images))
        args = step_args(root, lst, label_dir, a, "device")
        raw, _ = train_irn.make_datasets(args, 0)
        if not a.skip_pipeline:
            print(json.dumps({"augment_pair": bench_augment(raw, a, dev)}), flush=True)
            host, _ = train_irn.make_datasets(step_args(root, lst, label_dir, a, "host"), 0)
            print(json.dumps({"host_pipeline": TB.bench_host_pipeline(raw, host, min(a.images, 64))}), flush=True)
        if not a.skip_step:
            trunks = ("autograd", "inference") if a.irn_trunk == "both" else (a.irn_trunk,)
            with _tuned.process_mode():
                if "inference" in trunks:
                    _tuned.miopen_setup(torch.cuda.current_device())          # before the first convolution, as train_irn.run does
                torch.manual_seed(0)
                grid = a.crop // 4
                model = train_irn.build_model(args, indexing.PathIndex(radius=10, default_size=(grid, grid))).to(dev).train()
                opt = _train.two_rate_optimizer(*model.trainable_parameters(), 0.01, 1e-4, 10 ** 9)
                for augment in tuple(a.augments) * a.rounds:
                    for trunk in trunks:
                        print(json.dumps({"step": bench_step(step_args(root, lst, label_dir, a, augment), a, dev, model, opt, trunk)}), flush=True)


if __name__ == "__main__":
    main()
