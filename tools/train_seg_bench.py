#!/usr/bin/env python3
"""The segmentation training step's rate on synthetic VOC-size images, fused against composed loss.  Prints one JSON line per
measurement.

    python tools/train_seg_bench.py [--images 64] [--batch 16] [--crop 512] [--warmup 3] [--steps 20] [--workers 8] [--rounds 2]

`step`: images/s of `train_sem_seg`'s own loop (loader with `--workers` processes, the batch built on the device, forward,
loss, backward, update) over `--steps` steps after `--warmup`, `--seg_loss fused` and `composed` alternating `--rounds` times so
that the spread shows next to the difference; the clock stops behind a device synchronise; each line carries the peak of
allocated device memory.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import _train_bench as TB  # noqa: E402


def step_args(root, lst, a, loss):
    import run_train_seg
    return run_train_seg.build_parser().parse_args([
        "--voc12_root", root, "--train_list", lst, "--seg_label_dir", os.path.join(root, "sem_seg"), "--seg_batch_size", str(a.batch),
        "--seg_crop_size", str(a.crop), "--num_workers", str(a.workers), "--seg_loss", loss, "--seg_num_epoches", "1000000"])


def bench_step(args, a, dev):
    from irn_amd.step import _train, train_sem_seg
    from irn_amd.voc12 import dataloader
    torch.manual_seed(0)
    model = train_sem_seg.build_model(args).to(dev).train()
    train = train_sem_seg.make_dataset(args, 0)
    # the seeded random weights give large logits: a rate that keeps every step finite (the step's cost does not depend on it)
    opt = _train.two_rate_optimizer(*model.trainable_parameters(), 1e-6, 5e-4, 10 ** 9)

    def step(pack):
        img, label = _train.device_pair(pack, args.seg_crop_size, dev, reduce=1)
        return train_sem_seg.train_step(model, opt, img, label, args.seg_loss)

    figures, last = TB.timed_steps(train, lambda ep: _train.loader(train, a.batch, a.workers, True, ep, dataloader.affinity_collate),
                                   step, a.warmup, a.steps, a.batch)
    return {"seg_loss": args.seg_loss, "batch": a.batch, "crop": a.crop, **figures, "last_loss": float(last)}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--images", default=64, type=int)
    p.add_argument("--batch", default=16, type=int)
    p.add_argument("--crop", default=512, type=int)
    p.add_argument("--warmup", default=3, type=int)
    p.add_argument("--steps", default=20, type=int)
    p.add_argument("--workers", default=8, type=int)
    p.add_argument("--rounds", default=2, type=int)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_seg_bench needs a GPU")
    from irn_amd import _tuned
    dev = torch.device("cuda", torch.cuda.current_device())
    with tempfile.TemporaryDirectory() as root:
        lst, _ = TB.write_tree(root, a.images, labels="sem_seg")
        with _tuned.process_mode():
            for loss in ("fused", "composed") * a.rounds:
                print(json.dumps({"step": bench_step(step_args(root, lst, a, loss), a, dev)}), flush=True)


if __name__ == "__main__":
    main()
