"""Multi-scale CAM inference step — drop-in for reference step/make_cam.py (`run(args)`).

Reads  args.cam_network, args.cam_weights_name(+'.pth'), args.train_list, args.voc12_root,
       args.cam_scales, args.num_workers
Writes args.cam_out_dir/<name>.npy = {"keys": LongTensor[K], "cam": FloatTensor[K,h,w] (cpu),
       "high_res": float32 ndarray [K,H,W]}   (same pickle schema as step/make_cam.py:55-56)

The per-scale inputs are built on the GPU from the decoded uint8 image (irn_msf_pack: Pillow-exact bicubic,
normalise, flip pair; args.device_preprocess=False keeps the reference's PIL loop in the loader workers).
The ResNet-50 forward passes run on PyTorch-ROCm (MIOpen), `cam_batch` images of one size per pass (default 8;
the reference: one image + its flip); the merge (step/make_cam.py:38-52) is one HIP kernel pair (irn_cam_merge).
Every image's {keys, cam} also stays on the device (`_stores.CAM_STORE`) for label steps that run later in the same
process.  One process per GPU over strided shards, no communication.
"""
import os
import warnings

import numpy as np
import torch

from ..misc import torchutils
from ..voc12 import dataloader as voc12_dataloader
from . import _classes, _io, _pool, _report, _split_auto, _stores


def merge_scales(outputs, size, label):
    """outputs: per-scale GPU [C,hs,ws] activation maps (C classes) -> (keys, cam [K,ceil(H/4),ceil(W/4)],
    high_res [K,H,W]) — step/make_cam.py:38-52 in two launches of libirn_hip.so (irn_cam_merge).
    GPU tensors only (the torch-op restatement the tests compare with lives in oracle/torch_mirrors.py)."""
    from .. import ops
    return ops.cam_merge(outputs, size, label)


def _save_cam(path, keys_cpu, event, staging, cam_view, hi_view, auto=None):
    """Writer-thread half of a CAM hand-off: wait for the image's device-to-host copies, write the reference's
    dictionary (step/make_cam.py:55-56), recycle the staging buffer.  `auto` = (the flush's flag words — copied on the same stream
    in front of the image, so behind `event` they have landed —, the image's index in the flush, its name, the worker's redo
    list): an image that left fp16's range is not written; its name goes on the list."""
    event.synchronize()
    try:
        if auto is not None and auto[0].flagged(auto[1]):
            auto[3].add(auto[2])
            return
        np.save(path, {"keys": keys_cpu, "cam": cam_view.clone(), "high_res": hi_view.numpy()})
    finally:
        _io.PINNED.give(staging)
        if auto is not None:
            auto[0].release()


def _flush_group(model, group, scales, args, writer, store, redo=None):
    """One trunk pass per scale for all images of a size group ([image, flip, image, flip, ...]), then the per-image
    merge (irn_cam_merge) and the asynchronous write of the reference's dictionary.  Nothing here waits for the device:
    the present classes come from the host-side label, the results leave through page-locked staging on the stream, and
    the writer threads wait for each image's copy event — so the next group's passes are queued while this one runs.  With a
    `redo` list (`--split_gemm auto`) the passes record the fp16-range flag per row and scale; the words leave with the images."""
    if not group:
        return
    from ..net import resnet50 as _r50
    outs = []
    flags = torch.zeros((len(scales), 2 * len(group)), dtype=torch.int32, device=group[0]["imgs"][0].device) if redo is not None else None
    for si in range(len(scales)):
        x = torch.cat([g["imgs"][si] for g in group])
        before = (_r50.PASS_STATS["channels_last"], _r50.PASS_STATS["nchw"])
        with _split_auto.recording(None if flags is None else flags[si]):
            outs.append(model.forward_batch(x))
        _report.CAM_STATS["channels_last"] += _r50.PASS_STATS["channels_last"] - before[0]
        _report.CAM_STATS["nchw"] += _r50.PASS_STATS["nchw"] - before[1]
    _report.CAM_STATS["full_group_flushes" if len(group) >= int(getattr(args, "cam_batch", 0) or 8) else "partial_group_flushes"] += 1
    read = None if flags is None else _split_auto.FlagRead(flags, [g["name"] for g in group], users=len(group))
    for i, g in enumerate(group):
        keys_cpu = torch.nonzero(g["label"])[:, 0]
        keys, cam, high_res = merge_scales([o[i] for o in outs], g["size"], g["label"])
        if store is not None:
            store.put(g["name"], keys_cpu, keys, cam, cam_out_dir=args.cam_out_dir, run_id=getattr(args, "cam_run_id", None))
        n_cam, n_hi = cam.numel() * 4, high_res.numel() * 4
        staging = _io.PINNED.take(n_cam + n_hi)
        cam_view = staging[:n_cam].view(torch.float32).view(cam.shape)
        hi_view = staging[n_cam:n_cam + n_hi].view(torch.float32).view(high_res.shape)
        cam_view.copy_(cam, non_blocking=True)
        hi_view.copy_(high_res, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        job = (os.path.join(args.cam_out_dir, g["name"] + ".npy"), keys_cpu, event, staging, cam_view, hi_view)
        if read is None:
            writer.submit(_save_cam, *job)
        else:
            writer.submit(_save_cam, *job, auto=(read, i, g["name"], redo))
    group.clear()


def _redo_fp32(model, databin, index_of, redo, scales, batch, args, writer, store):
    """`--split_gemm auto`, after the shard's loop: the images on the redo list once more — decoded again, every scale again,
    in the same `pass_rows` passes — with the split-precision GEMMs off; written and stored like any other image, so the files
    are those of a `--split_gemm 0` run.  The entries the split pass left in the store are dropped first."""
    from torch.utils.data import default_collate
    from ..net import resnet50 as _r50
    names = sorted(n for n, _ in redo.items())
    for name in names:
        _stores.CAM_STORE.drop(name, args.cam_out_dir)
    groups = {}
    with _r50.fp32_gemms():
        for name in names:
            pack = default_collate([databin[index_of[name]]])
            size = (int(pack["size"][0]), int(pack["size"][1]))
            group = groups.setdefault(size, [])
            group.append({"name": name, "size": size, "label": pack["label"][0], "imgs": _io.device_images(pack, scales)})
            if len(group) == batch:
                _flush_group(model, group, scales, args, writer, store)
        for group in groups.values():
            _flush_group(model, group, scales, args, writer, store)


def _work(process_id, model, dataset, args):
    model = _pool.materialise(model)      # a network, or the (class, checkpoint) a worker builds it from
    scales = tuple(float(s) for s in args.cam_scales)
    # images per trunk pass (the reference runs batch 2 = one image + flip, step/make_cam.py:32-33); images of one size
    # are stacked per scale — VOC is mostly 500x375 / 375x500 — and every size group is flushed at the end
    batch = int(getattr(args, "cam_batch", 0) or 8)
    store = _stores.CAM_STORE if _stores.keep_cams(args) else None
    _stores.CAM_STORE.drop_dir(args.cam_out_dir)        # this directory's files are about to be rewritten
    redo = _split_auto.Redo() if _split_auto.enabled() else None      # --split_gemm auto: images to compute again on the fp32 GEMMs
    index_of = {}
    groups = {}
    pending_bytes, max_pending = 0, int(getattr(args, "cam_pending_bytes", 0) or (4 << 30))
    with _io.shard_io(process_id, dataset, args) as (databin, n_gpus, loader, writer):
        with torch.no_grad(), torch.cuda.device(_pool.worker_device(process_id, args)):
            model.cuda()
            for it, pack in enumerate(loader):
                img_name = pack["name"][0]
                if not isinstance(img_name, str):
                    img_name = voc12_dataloader.decode_int_filename(img_name)
                label = pack["label"][0]
                size = (int(pack["size"][0]), int(pack["size"][1]))
                if float(label.sum()) == 0:
                    # the reference would write an empty dictionary here and crash later in the label steps
                    warnings.warn("%s: no positive class in the image-level label, skipped" % img_name)
                    staging = pack.pop("_staging", None) if isinstance(pack, dict) else None
                    if staging is not None:                  # the loader thread's page-locked copy of an image nobody uploads
                        _io.PINNED.give(staging)
                    continue
                group = groups.setdefault(size, [])
                imgs = _io.device_images(pack, scales)
                index_of[img_name] = it
                group.append({"name": img_name, "size": size, "label": label, "imgs": imgs})
                pending_bytes += sum(t.numel() * t.element_size() for t in imgs)
                if len(group) == batch:
                    pending_bytes -= sum(t.numel() * t.element_size() for g in group for t in g["imgs"])
                    _flush_group(model, group, scales, args, writer, store, redo)
                elif pending_bytes > max_pending:
                    # VOC has hundreds of distinct image sizes: incomplete size groups may not pile up on the device
                    # without bound (34 MB per waiting 500x375 image) — the fullest one goes early
                    big = max(groups.values(), key=len)
                    pending_bytes -= sum(t.numel() * t.element_size() for g in big for t in g["imgs"])
                    _flush_group(model, big, scales, args, writer, store, redo)
                _io.progress(process_id, n_gpus, it, len(databin))
            for group in groups.values():
                _flush_group(model, group, scales, args, writer, store, redo)
            if redo is not None:
                writer.drain()                 # every image's flags have been looked at
                if len(redo):
                    _redo_fp32(model, databin, index_of, redo, scales, batch, args, writer, store)
                redo.report(process_id)


def run(args):
    c = _classes.num_classes(args)
    model = _pool.ModelSpec(args.cam_network, "CAM", args.cam_weights_name + ".pth", strict=True,
                            n_classes=None if c == _classes.VOC_CLASSES else c)   # built by the worker(s); a --cam_network of the user's own need not know the argument
    n_gpus = _pool.n_gpus_or_raise(args)
    scales = tuple(float(s) for s in args.cam_scales)
    dataset = voc12_dataloader.VOC12ClassificationDatasetMSF(args.train_list, voc12_root=args.voc12_root,
                                                             scales=scales, raw=_io.device_preprocess(args), n_classes=c)
    names = [voc12_dataloader.decode_int_filename(v) for v in dataset.img_name_list]
    dataset = torchutils.split_dataset(dataset, n_gpus)
    os.makedirs(args.cam_out_dir, exist_ok=True)
    args.cam_run_id = _stores.new_cam_run(args.cam_out_dir)      # device-held CAMs of earlier runs of this directory go stale
    print("[ ", end="")
    _pool.spawn_workers(_work, model, dataset, args)
    print("]")
    # which worker made (and, with keep_cams_on_device, still holds) every image's CAM: strided like the shards
    # (misc/torchutils.py:66-68) — the label steps of this run send an image to the worker that has its CAM
    owners = {name: i % n_gpus for i, name in enumerate(names)}
    owners["__n_workers__"] = n_gpus
    _stores.CAM_OWNERS[os.path.abspath(args.cam_out_dir)] = owners
    torch.cuda.empty_cache()
