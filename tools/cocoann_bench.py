#!/usr/bin/env python3
"""Rate of the make_cocoann step: images/s over a synthetic VOC-size tree, the share of the GPU kernels in it, the bytes
that come back per image against the dense masks' bytes, the kernels alone on masks that are already on the device, and
the numpy restatement of pycocotools (tests/_cocomask_ref.py) on the same files and host.  Prints one JSON line.

The detections are blob masks, not the output of make_ins_seg_labels: irn_amd/synth.py sizes, 1-4 masks per image
(thresholded `synth.cam_blobs`, upsampled from the stride-4 grid as the label step upsamples its walk), scores in (0, 1).

    python tools/cocoann_bench.py [--images 64] [--cpu-images 16]

With --segmentation polygon it measures the polygon mode instead: the step's images/s in both modes, three
runs of each, alternating; the three polygon entries alone between HIP events on masks that are already on the device, with
the sizes a first call read back (median of 20 passes over the images); the bytes read back and the JSON bytes per image; and
the plain-loop restatement (tests/_polygon_ref.py) on the host over --cpu-images of the images.  The result line is also
appended to profiles/cocoann_polygon_bench.json.

    python tools/cocoann_bench.py --segmentation polygon
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


def _args(root, out, segmentation="rle"):
    return argparse.Namespace(voc12_root=root, infer_list=os.path.join(root, "list.txt"), ins_seg_out_dir=os.path.join(root, "ins"),
                              cocoann_out=out, num_workers=8, cocoann_segmentation=segmentation)


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


def polygon_kernels_alone(names, root, reps=20):
    """The three polygon entries on every image's masks, resident on the device, with the edge, loop and corner counts of
    a first `ops.mask_polygons` call: HIP-event time per image (no read-back inside), launches per image, bytes the step
    reads back per image."""
    from irn_amd import _lib, ops
    L, dev = _lib.lib, torch.device("cuda", 0)
    work, launches, back = [], 0, 0
    for name in names:
        det = np.load(os.path.join(root, "ins", name + ".npy"), allow_pickle=True).item()
        m = torch.from_numpy(det["mask"]).to(dev).view(torch.uint8).contiguous()
        n, h, w = m.shape
        xy, loop_offsets, _, _ = ops.mask_polygons(m)
        scratch = torch.empty(L.irn_mask_polygon_scratch_bytes(n, h, w), dtype=torch.uint8, device=dev)
        head = torch.empty(4 * n + 1, dtype=torch.int32, device=dev)
        _lib.check(L.irn_mask_polygon_edges(m.data_ptr(), n, h, w, head.data_ptr(), scratch.data_ptr(), _lib._stream()))
        off = head[:n + 1].cpu().numpy().astype(np.int64)
        n_edges, longest = int(off[n]), int(np.diff(off).max())
        trace = torch.empty(max(L.irn_mask_polygon_trace_scratch_bytes(n_edges), 1), dtype=torch.uint8, device=dev)
        n_loops, n_verts = len(loop_offsets) - 1, len(xy)
        out = torch.empty(max(n_loops + 2 * n_verts, 1), dtype=torch.int32, device=dev)
        work.append((m, n, h, w, head, scratch, trace, n_edges, longest, out, n_loops, n_verts))
        rounds = int(np.ceil(np.log2(max(longest, 1))))
        launches += 8 + 2 * (rounds + rounds % 2)
        back += 4 * (n + 1) + 12 * n + 4 * (n_loops + 2 * n_verts)

    def once():
        for m, n, h, w, head, scratch, trace, n_edges, longest, out, n_loops, n_verts in work:
            p = head.data_ptr()
            _lib.check(L.irn_mask_polygon_edges(m.data_ptr(), n, h, w, p, scratch.data_ptr(), _lib._stream()))
            _lib.check(L.irn_mask_polygon_count(m.data_ptr(), n, h, w, p, n_edges, longest, p + 4 * (n + 1), p + 4 * (2 * n + 1),
                                                p + 4 * (3 * n + 1), scratch.data_ptr(), trace.data_ptr(), _lib._stream()))
            _lib.check(L.irn_mask_polygon_emit(n_edges, out.data_ptr(), n_loops, out.data_ptr() + 4 * n_loops, n_verts,
                                               trace.data_ptr(), _lib._stream()))
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
    return float(np.median(times)) / len(work) * 1e3, launches / len(work), back / len(work)


def polygon_main(a):
    import _polygon_ref as P
    from irn_amd.step import make_cocoann
    torch.cuda.set_device(0)
    res = {"metric": "make_cocoann polygon mode", "images": a.images, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as root:
        names, dense, n_masks = make_tree(root, a.images)
        outs = {mode: os.path.join(root, mode + ".json") for mode in ("rle", "polygon")}

        def go(mode):
            with contextlib.redirect_stdout(io.StringIO()):
                return make_cocoann.run(_args(root, outs[mode], mode))
        stats = {mode: go(mode) for mode in outs}                  # warm: kernels loaded, page cache filled
        rates = {mode: [] for mode in outs}
        for _ in range(3):
            for mode in outs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                go(mode)
                torch.cuda.synchronize()
                rates[mode].append(round(a.images / (time.perf_counter() - t0), 1))
        res["masks_per_image"] = round(n_masks / a.images, 2)
        res["step_images_per_s"] = rates
        res["masks_with_holes"], res["holes"] = stats["polygon"]["masks_with_holes"], stats["polygon"]["holes"]
        coco = json.load(open(outs["polygon"]))
        res["corners_per_image"] = round(sum(len(loop) // 2 for x in coco["annotations"] for loop in x["segmentation"]) / a.images, 1)
        res["json_bytes_per_image"] = {mode: round(os.path.getsize(outs[mode]) / a.images, 1) for mode in outs}
        res["dense_mask_bytes_per_image"] = round(dense / a.images, 1)
        us, launches, back = polygon_kernels_alone(names, root)
        res["kernels_alone_us_per_image"] = round(us, 2)
        res["launches_per_image"] = round(launches, 1)
        res["bytes_back_per_image"] = round(back, 1)
        if a.cpu_images > 0:
            sub = names[:a.cpu_images]
            masks = [np.load(os.path.join(root, "ins", name + ".npy"), allow_pickle=True).item()["mask"] for name in sub]
            t0 = time.perf_counter()
            for m in masks:
                P.mask_polygons(m)
            res["restatement_images_per_s"] = round(len(sub) / (time.perf_counter() - t0), 3)
            res["cpu_images"] = len(sub)
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "cocoann_polygon_bench.json"), "a") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--cpu-images", type=int, default=16)
    ap.add_argument("--segmentation", choices=("rle", "polygon"), default="rle")
    a = ap.parse_args()
    if a.segmentation == "polygon":
        return polygon_main(a)
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
