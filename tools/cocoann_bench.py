#!/usr/bin/env python3
"""Rate of the make_cocoann step: images/s over a synthetic VOC-size tree, the share of the GPU kernels in it, the bytes
that come back per image against the dense masks' bytes, the kernels alone on masks that are already on the device, and
the numpy restatement of pycocotools (tests/_cocomask_ref.py) on the same files and host.  Prints one JSON line.

The detections are blob masks, not the output of make_ins_seg_labels: irn_amd/synth.py sizes, 1-4 masks per image
(thresholded `synth.cam_blobs`, upsampled from the stride-4 grid as the label step upsamples its walk), scores in (0, 1).

    python tools/cocoann_bench.py [--images 64] [--cpu-images 16]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from irn_amd import synth  # noqa: E402


def blob_masks(k, h, w, seed):
    gh, gw = synth.grid_of((h, w))
    cams = torch.from_numpy(synth.cam_blobs(k, gh, gw, seed=seed))[None]
    up = torch.nn.functional.interpolate(cams, size=(h, w), mode="bilinear", align_corners=False)[0].numpy()
    return up > np.random.RandomState(seed).uniform(0.3, 0.6, (k, 1, 1))


def make_tree(root, n):
    from PIL import Image
    for d in ("JPEGImages", "ins"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    names, dense, n_masks = [], 0, 0
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        rng = np.random.RandomState(i)
        h, w = synth.voc_image_size(i)
        Image.fromarray(synth.photo(h, w, seed=i)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=90)
        k = rng.randint(1, 5)
        masks = blob_masks(k, h, w, i)
        np.save(os.path.join(root, "ins", name + ".npy"), {"score": rng.uniform(0.05, 1.0, k).astype(np.float32), "mask": masks,
                                                           "class": rng.randint(0, 20, k).astype(np.int64)})
        names.append(name)
        dense += masks.size
        n_masks += k
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return names, dense, n_masks


def _args(root, out):
    return argparse.Namespace(voc12_root=root, infer_list=os.path.join(root, "list.txt"), ins_seg_out_dir=os.path.join(root, "ins"),
                              cocoann_out=out, num_workers=8)


def kernel_ms(fn):
    """GPU time of the encoder's kernels (torch.profiler device events) for one run, in ms."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    total = 0.0
    for e in prof.key_averages():
        if "k_rle_" in e.key:
            total += getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0))
    return total / 1e3


def kernels_alone(names, root, reps=20):
    """The two entries on every image's masks, resident on the device: HIP-event time per image, and the bytes the
    floor counts (two reads of the masks, one write of the counts) over that time."""
    from irn_amd import _lib, ops
    dev = torch.device("cuda", 0)
    work = []
    for name in names:
        det = np.load(os.path.join(root, "ins", name + ".npy"), allow_pickle=True).item()
        m = torch.from_numpy(det["mask"]).to(dev).view(torch.uint8).contiguous()
        _, offsets, _, _ = ops.mask_rle(m)
        n, h, w = m.shape
        work.append((m, n, h, w, torch.from_numpy(offsets).to(dev), int(offsets[-1]),
                     torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                     torch.empty((n, 4), dtype=torch.int32, device=dev), torch.empty(max(int(offsets[-1]), 1), dtype=torch.int32, device=dev),
                     torch.empty(_lib.lib.irn_mask_rle_scratch_bytes(n, h, w), dtype=torch.uint8, device=dev)))
    moved = sum(2 * m.numel() + 4 * total for m, _, _, _, _, total, *_ in work)

    def once():
        for m, n, h, w, off, _, runs, area, bbox, counts, scratch in work:
            _lib.check(_lib.lib.irn_mask_rle_count(m.data_ptr(), n, h, w, runs.data_ptr(), area.data_ptr(), bbox.data_ptr(),
                                                   scratch.data_ptr(), _lib._stream()))
            _lib.check(_lib.lib.irn_mask_rle_emit(m.data_ptr(), n, h, w, off.data_ptr(), counts.data_ptr(), scratch.data_ptr(),
                                                  _lib._stream()))
    once()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        once()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    return ms / len(work) * 1e3, moved / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--cpu-images", type=int, default=16)
    a = ap.parse_args()
    import _cocomask_ref as R
    from irn_amd.step import make_cocoann
    torch.cuda.set_device(0)
    res = {"metric": "make_cocoann images/s", "images": a.images, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as root:
        names, dense, n_masks = make_tree(root, a.images)
        out = os.path.join(root, "coco.json")

        def go():
            with contextlib.redirect_stdout(io.StringIO()):
                make_cocoann.run(_args(root, out))
        go()                                                   # warm: kernels loaded, page cache filled
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            go()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 3
        kms = kernel_ms(go)
        coco = json.load(open(out))
        n_counts = sum(len(R.from_string(x["segmentation"]["counts"])) for x in coco["annotations"])
        res["masks_per_image"] = round(n_masks / a.images, 2)
        res["counts_per_image"] = round(n_counts / a.images, 1)
        res["step_images_per_s"] = round(a.images / dt, 1)
        res["kernel_share"] = round(kms / (1e3 * dt), 4)
        res["kernel_ms_per_image_in_step"] = round(kms / a.images, 4)
        # what comes back per image: the run lengths (4 bytes each) and, per mask, area + bbox + run count (28 bytes)
        res["bytes_back_per_image"] = round((4 * n_counts + 28 * len(coco["annotations"])) / a.images, 1)
        res["dense_mask_bytes_per_image"] = round(dense / a.images, 1)
        res["json_bytes_per_image"] = round(os.path.getsize(out) / a.images, 1)
        us, gbs = kernels_alone(names, root)
        res["kernels_alone_us_per_image"] = round(us, 2)
        res["kernels_alone_floor_gb_per_s"] = round(gbs, 1)
        if a.cpu_images > 0:
            sub = names[:a.cpu_images]
            t0 = time.perf_counter()
            R.cocoann(sub, root, os.path.join(root, "ins"))
            res["numpy_images_per_s"] = round(len(sub) / (time.perf_counter() - t0), 2)
            res["cpu_images"] = len(sub)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
