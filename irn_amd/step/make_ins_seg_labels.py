"""Instance pseudo-label step — drop-in for reference step/make_ins_seg_labels.py (`run(args)`).

Reads  args.irn_network, args.irn_weights_name, args.infer_list, args.voc12_root, args.cam_out_dir,
       args.beta, args.exp_times, args.ins_seg_bg_thres, args.num_workers
Writes args.ins_seg_out_dir/<name>.npy = {'score': float[N], 'mask': bool[N,H,W], 'class': int64[N]}
       (schema consumed by step/make_cocoann.py:34-38 and step/eval_ins_seg.py)
       or, with args.ins_seg_format == "rle" (not in the reference), args.ins_seg_out_dir/<name>.rle.npz = {'score' f32[N],
       'class' i64[N], 'size' i64[2] = (H, W), 'counts' u32[total], 'offsets' i64[N+1], 'area' i64[N], 'bbox' i32[N,4]}:
       detection d's mask as its COCO run lengths counts[offsets[d]:offsets[d+1]] (`ops.detect_instance_rle_batch`; plain
       arrays, no pickle).  No dense mask is allocated, filled or copied in that mode.

Per image (step/make_ins_seg_labels.py:119-152): EdgeDisplacement forward -> edge, dp; centroid
refinement, clustering, per-instance CAM split, random walk, label epilogue and the per-mask
connected components all run on the GPU through libirn_hip.so.  An image with no detected instance
is skipped with a warning (the reference crashes in np.stack([])).
"""
import os
import warnings

import numpy as np
import torch

from .. import ops
from ..net import resnet50 as _r50
from . import _labels, _split_auto

find_centroids_with_refinement = ops.find_centroids_with_refinement
cluster_centroids = ops.cluster_centroids
detect_instance = ops.detect_instance


def instance_front(items):
    """First half of step/make_ins_seg_labels.py:131-150 for a batch: centroid refinement and clustering, ENQUEUED only — the
    instance counts K stay on the device.  -> what `instance_back` needs."""
    dps = [it["dp"] for it in items]
    return ops.cluster_centroids_batch(ops.find_centroids_batch(dps), dps, k_on_device=True)


def instance_back(walker, items, front, beta, exp_times, bg_thres, deferred=False, fmt="npy", timings=None):
    """Second half: reads the K of `instance_front` (the first host round trip of the batch), then the per-instance CAM split +
    random walk, the label epilogue and the detections — with dense masks (`fmt` "npy") or as run lengths ("rle")."""
    cmaps, k_dev = front
    ks = [int(k) for k in k_dev.cpu().tolist()]
    rws = walker([it["edge"] for it in items], [it["cam"] for it in items], beta=beta, exp_times=exp_times,
                 inst_maps=cmaps, k_inst=ks)
    def epilogue():
        return ops.label_epilogue(rws, [it["size"] for it in items], bg_thres, want_labels=False, want_argmax=True, want_rw_up=True)
    ep = epilogue()
    if walker.sync():                       # the persistent walk gave up and the batch was re-run on the streaming sweeps
        ep = epilogue()
    n_ch = [it["cam"].shape[0] * k for it, k in zip(items, ks)]
    class_ids = [np.repeat(np.asarray(torch.as_tensor(it["keys"]).cpu()), k) for it, k in zip(items, ks)]
    detect = {"npy": ops.detect_instance_batch, "rle": ops.detect_instance_rle_batch}[fmt]
    return detect(ep["rw_up"], ep["argmax"], class_ids, n_ch, [it["size"][0] * it["size"][1] * 0.01 for it in items],
                  timings=timings, deferred=deferred)


def instance_labels_batch(walker, items, beta, exp_times, bg_thres, deferred=False):
    """step/make_ins_seg_labels.py:131-150 for a batch of images.  items: dicts with GPU tensors
    `edge` [1,h,w], `dp` [2,h,w], `cam` [C,h,w], CPU/GPU `keys` [C] and `size` (H, W).  Every stage runs ONCE for the
    whole batch — centroid refinement, clustering, random walk (a 128x128 grid is 16 tiles at radius 5: one image uses
    1/16 of the GPU), label epilogue, detection — with three host round trips per BATCH: the instance counts K (they
    size the walk's channels), the detection counts, and the packed detections.  Returns a list of detection dicts
    (or the ValueError of an image without detections, in its slot); with `deferred=True` an `ops.PendingDetections`
    whose `result()` is that list — the packed transfer then runs under whatever the caller enqueues next."""
    return instance_back(walker, items, instance_front(items), beta, exp_times, bg_thres, deferred=deferred)


def instance_labels(walker, edge, dp, cams, keys, size, beta, exp_times, bg_thres):
    """One image: returns the detection dict (numpy) — step/make_ins_seg_labels.py:131-150."""
    det = instance_labels_batch(walker, [{"edge": edge, "dp": dp, "cam": cams, "keys": keys, "size": size}],
                                beta, exp_times, bg_thres)[0]
    if isinstance(det, Exception):
        raise det
    return det


def ins_seg_format(args):
    fmt = getattr(args, "ins_seg_format", "npy")
    if fmt not in ("npy", "rle"):
        raise ValueError("ins_seg_format must be npy or rle, got %r" % (fmt,))
    return fmt


def save_rle(path, det):
    """One image's run-length detections as <name>.rle.npz: the arrays of `ops.detect_instance_rle_batch`, size as int64[2]."""
    with open(path, "wb") as f:            # an open file: np.savez would append ".npz" to a name
        np.savez(f, score=det["score"], size=np.asarray(det["size"], np.int64), counts=det["counts"],
                 offsets=det["offsets"], area=det["area"], bbox=det["bbox"], **{"class": det["class"]})


def _write(names, pending, args, writer, flags=None, redo=None, store=None):
    """Hand the batch's detections to the writer threads.  `flags` (`--split_gemm auto`: the batch's fp16-range flag words, sent
    to the host right behind its IRNet forward, long before the detections `pending.result()` waits for): an image that left
    the range gets no file and goes on `redo`."""
    rle = ins_seg_format(args) == "rle"
    dets = pending.result()
    bad = _labels.drop_flagged(flags, redo, store, wait=True)
    for name, det in zip(names, dets):
        if name in bad:
            continue
        if isinstance(det, Exception):
            warnings.warn("%s: %s — no file written" % (name, det))
            continue
        if rle:
            writer.submit(save_rle, os.path.join(args.ins_seg_out_dir, name + ".rle.npz"), det)
        else:
            writer.submit(np.save, os.path.join(args.ins_seg_out_dir, name + ".npy"), det)


def _flush(model, walker, pend, args, writer, state, redo=None):
    """One turn of the step's three-stage pipeline; `state` = {"front": batch whose IRNet forward + clustering are enqueued,
    "emit": batch whose detections are crossing PCIe}.  In this order:
      1. the batch in `front` gets its back half (the K read-back, by now long computed; walk, epilogue, detections) —
         BEFORE anything of the new batch is enqueued, so that its two small read-backs never queue behind 45 ms of IRNet;
      2. the batch in `pend` gets its IRNet forward, centroid refinement and clustering enqueued — the GPU works on them while
         the caller's loop decodes and uploads the next batch (round 5: the K read-back used to stall that loop for the whole
         forward, 40 % of the step);
      3. the batch in `emit` is collected and handed to the writer threads.
    With a `redo` list (`--split_gemm auto`) stage 2 records the IRNet forward's per-image fp16-range flags and stage 3 acts on them."""
    done = None
    if state.get("front") is not None:
        items, front, *auto = state["front"]                # auto: (the batch's flag words on their way to the host, the edge store)
        extra = {"fmt": "rle"} if ins_seg_format(args) == "rle" else {}        # the default call is the one it always was
        if getattr(args, "detect_timings", None) is not None:                   # a caller's dict for the detection calls' `timings`
            extra["timings"] = args.detect_timings
        done = ([it["name"] for it in items],
                instance_back(walker, items, front, float(args.beta), int(args.exp_times), float(args.ins_seg_bg_thres), deferred=True,
                              **extra), *auto)
        state["front"] = None
    if pend:
        kw = _labels.edge_store_kw(model, args)
        _labels.edges_for(model, pend, _labels.irn_batch(args), auto=redo is not None, **kw)
        items = list(pend)
        pend.clear()
        auto = (_labels.flag_read(items), kw.get("store")) if redo is not None else ()
        state["front"] = (items, instance_front(items), *auto)
    if state.get("emit") is not None:
        names, pending, *auto = state["emit"]
        _write(names, pending, args, writer, *((auto[0], redo, auto[1]) if auto else ()))
    state["emit"] = done


def _work(process_id, model, dataset, args):
    batch = _labels.walk_batch(args, 32)
    with _labels.worker(process_id, model, dataset, args) as w:
        pend, state = [], {}
        redo = _split_auto.Redo() if _split_auto.enabled() else None      # --split_gemm auto
        for item in _labels.items(w, args):
            pend.append(item)
            if len(pend) == batch:
                _flush(w.model, w.walker, pend, args, w.writer, state, redo)
        _flush(w.model, w.walker, pend, args, w.writer, state, redo)      # the last batch's front half ...
        _flush(w.model, w.walker, pend, args, w.writer, state, redo)      # ... its back half ...
        _flush(w.model, w.walker, pend, args, w.writer, state, redo)      # ... and its collection
        if redo is not None:
            # the images that left fp16's range once more, IRNet on the fp32 GEMMs: their maps go back into the store
            todo = _labels.redo_items(redo, w, args)
            with _r50.fp32_gemms():
                for i in range(0, len(todo), batch):
                    pend = todo[i:i + batch]
                    for _ in range(3):
                        _flush(w.model, w.walker, pend, args, w.writer, state)
            redo.report(process_id)


def run(args):
    _labels.run_step(_work, args.ins_seg_out_dir, args, opening="[ ")


