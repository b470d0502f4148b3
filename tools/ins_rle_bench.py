#!/usr/bin/env python3
"""The instance step's back half in both output formats, and make_cocoann on what each wrote.  Prints one JSON line.

64 synthetic VOC-size images (irn_amd/synth.py sizes, fields and CAMs, resident on the device as the step holds them
after the IRNet forward).  Per format, in the same process: front end + walk + epilogue + detections in batches of
`--batch` with the step's own hand-over (the detections of batch i are collected and given to the writer threads after
batch i+1 has been enqueued), files written — images/s and device-to-host bytes per image; then make_cocoann over the
directory — images/s.  The two COCO files must be byte-identical.  Last, the kernels alone on one batch (HIP events):
the dense emit, and the two run-length entries.

    python tools/ins_rle_bench.py [--images 64] [--batch 32] [--reps 3]
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


def make_items(n, dev, root):
    from PIL import Image
    os.makedirs(os.path.join(root, "JPEGImages"), exist_ok=True)
    items = []
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        h, w = synth.voc_image_size(i)
        gh, gw = synth.grid_of((h, w))
        k = synth.voc_num_classes(i)
        Image.fromarray(synth.photo(h, w, seed=i)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=90)
        items.append({"name": name, "edge": torch.from_numpy(synth.edge_field(gh, gw, i))[None].to(dev),
                      "dp": torch.from_numpy(synth.displacement_field(gh, gw, seed=i, strength=0.3)).to(dev),
                      "cam": torch.from_numpy(synth.cam_blobs(k, gh, gw, i)).to(dev),
                      "keys": torch.from_numpy(synth.voc_keys(k, i)), "size": (h, w)})
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("\n".join(it["name"] for it in items) + "\n")
    return items


def step(walker, items, batch, fmt, out_dir, timings):
    """make_ins_seg_labels._flush without the IRNet forward: back half of batch i, then the collection of batch i-1."""
    from irn_amd.step import _common
    from irn_amd.step import make_ins_seg_labels as mis
    args = argparse.Namespace(ins_seg_out_dir=out_dir, ins_seg_format=fmt)
    writer = _common.AsyncWriter(threads=_common.writer_threads(args, 1))
    try:
        emit = None
        for s in range(0, len(items), batch):
            part = items[s:s + batch]
            pending = mis.instance_back(walker, part, mis.instance_front(part), 10.0, 8, 0.25, deferred=True, fmt=fmt,
                                        timings=timings)
            if emit is not None:
                mis._write(*emit, args, writer)
            emit = ([it["name"] for it in part], pending)
        mis._write(*emit, args, writer)
    finally:
        writer.close()


def timed(fn, reps):
    fn()                                                       # warm: kernels loaded, buffers grown, page cache filled
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def kernels_alone(walker, items, reps=20):
    """One batch's detection kernels between HIP events, ms per batch: the dense emit, the run-length count and emit."""
    import ctypes as C

    from irn_amd import ops
    from irn_amd._lib import _stream, check, i32_array, lib, ptr_array
    from irn_amd.step import make_ins_seg_labels as mis
    cmaps, k_dev = mis.instance_front(items)
    ks = [int(k) for k in k_dev.cpu().tolist()]
    rws = walker([it["edge"] for it in items], [it["cam"] for it in items], beta=10.0, exp_times=8, inst_maps=cmaps, k_inst=ks)
    ep = ops.label_epilogue(rws, [it["size"] for it in items], 0.25, want_labels=False, want_argmax=True, want_rw_up=True)
    walker.sync()
    n_ch = [it["cam"].shape[0] * k for it, k in zip(items, ks)]
    dc = ops.detect_batch_count(ep["rw_up"], ep["argmax"], n_ch)
    n, dev, hs, ws, nds, scratch = dc.n, dc.dev, dc.hs, dc.ws, dc.nds, dc.scratch
    cs_a, hs_a, ws_a, sc_p, am_p = dc.cs_a, dc.hs_a, dc.ws_a, dc.sc_p, dc.am_p
    G, nd_a = sum(nds), i32_array(nds)
    area_min = (C.c_double * n)(*[it["size"][0] * it["size"][1] * 0.01 for it in items])
    dense = [torch.empty(max(nd, 1) * h * w, dtype=torch.uint8, device=dev) for nd, h, w in zip(nds, hs, ws)]
    score, chan = torch.empty(max(G, 1), dtype=torch.float32, device=dev), torch.empty(max(G, 1), dtype=torch.int32, device=dev)
    firsts = np.concatenate([[0], np.cumsum(nds)]).tolist()
    live = [nd > 0 for nd in nds]
    sc_o = ptr_array([score.data_ptr() + 4 * g if l else None for g, l in zip(firsts, live)])
    ch_o = ptr_array([chan.data_ptr() + 4 * g if l else None for g, l in zip(firsts, live)])
    mk_o = ptr_array([m.data_ptr() if l else None for m, l in zip(dense, live)])
    head = torch.empty(32 * max(G, 1), dtype=torch.uint8, device=dev)
    rle_scratch = torch.empty(lib.irn_detect_instance_batch_rle_scratch_bytes(n, hs_a, ws_a, nd_a), dtype=torch.uint8, device=dev)
    base = head.data_ptr()

    def count_dense():      # (the labelling is shared by both paths and is not part of either figure)
        check(lib.irn_detect_instance_batch_emit(n, sc_p, am_p, cs_a, hs_a, ws_a, nd_a, area_min, sc_o, ch_o, mk_o, scratch.data_ptr(),
                                                 _stream()))

    def count_rle():
        check(lib.irn_detect_instance_batch_rle_count(n, sc_p, am_p, cs_a, hs_a, ws_a, nd_a, area_min, base, base + 4 * G, base + 8 * G,
                                                      base + 12 * G, base + 16 * G, scratch.data_ptr(), rle_scratch.data_ptr(),
                                                      _stream()))
    count_rle()
    n_runs = head[12 * G:16 * G].view(torch.int32).cpu().numpy()
    runs = [int(n_runs[a:b].sum()) for a, b in zip(firsts[:-1], firsts[1:])]
    total = sum(runs)
    ws_bytes = lib.irn_detect_instance_batch_rle_sort_bytes(total, G)
    sort_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    runs_a = (C.c_int64 * n)(*runs)

    def emit_rle():
        check(lib.irn_detect_instance_batch_rle_emit(n, hs_a, ws_a, nd_a, runs_a, counts.data_ptr(), rle_scratch.data_ptr(),
                                                     sort_ws.data_ptr(), ws_bytes, _stream()))

    def ms(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times))
    return {"batch": n, "detections": G, "runs": total, "dense_emit_ms": round(ms(count_dense), 4),
            "rle_count_ms": round(ms(count_rle), 4), "rle_emit_ms": round(ms(emit_rle), 4),
            "dense_mask_bytes": int(sum(nd * h * w for nd, h, w in zip(nds, hs, ws)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from irn_amd.misc import indexing
    from irn_amd.step import make_cocoann
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"metric": "instance step back half + make_cocoann, npy vs rle", "images": a.images, "batch": a.batch,
           "device": torch.cuda.get_device_name(0)}
    warnings.simplefilter("ignore")
    with tempfile.TemporaryDirectory() as root:
        items = make_items(a.images, dev, root)
        walker = indexing.RandomWalk(5, dev)
        for fmt in ("npy", "rle"):
            out_dir, coco = os.path.join(root, "ins_" + fmt), os.path.join(root, fmt + ".json")
            os.makedirs(out_dir)
            timings = {}
            dt = timed(lambda: step(walker, items, a.batch, fmt, out_dir, timings), a.reps)
            files = os.listdir(out_dir)
            res[fmt] = {"step_images_per_s": round(a.images / dt, 1),
                        "d2h_bytes_per_image": round(timings["bytes"] / (a.reps + 1) / a.images, 1),
                        "file_bytes_per_image": round(sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) / a.images, 1),
                        "files": len(files)}
            args = argparse.Namespace(voc12_root=root, infer_list=os.path.join(root, "list.txt"), ins_seg_out_dir=out_dir,
                                      cocoann_out=coco, num_workers=8)

            def export():
                with contextlib.redirect_stdout(io.StringIO()):
                    make_cocoann.run(args)
            res[fmt]["cocoann_images_per_s"] = round(a.images / timed(export, a.reps), 1)
        res["coco_files_identical"] = open(os.path.join(root, "npy.json"), "rb").read() == open(os.path.join(root, "rle.json"), "rb").read()
        res["annotations"] = len(json.load(open(os.path.join(root, "rle.json")))["annotations"])
        res["kernels_per_batch"] = kernels_alone(walker, items[:a.batch])
        walker.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
