"""Shared plumbing of the label steps (make_sem_seg_labels, make_ins_seg_labels); tune_sem_seg walks with the same pieces.

A label step is `run_step`: the split sharded over the worker devices, one `_work` of the step's own module per shard.  Every
`_work` is a loop over `items()` (one image at a time, with its CAM) inside `worker()` (network, loader, writer threads and
walker of the shard, taken down again however the loop ends); what it does with a batch of images is the step's own.  The
boundary / displacement maps come from `edges_for`, handed from step to step on the device as `edge_store_kw` says."""
import contextlib
import os
import types
import weakref

import numpy as np
import torch
from PIL import Image

from ..voc12 import dataloader as voc12_dataloader
from .. import _tuned
from . import _io, _pool, _report, _split_auto, _stores

RADIUS = 5   # hard-coded at both reference call sites (step/make_sem_seg_labels.py:41, step/make_ins_seg_labels.py:135)


def walk_radius(args, default):
    """The reference hard-codes radius 5 at its call sites (step/make_sem_seg_labels.py:41,
    step/make_ins_seg_labels.py:135); `args.radius` (run_sample.py --radius) overrides it, e.g. 10 for BASELINE
    configs[2]."""
    return int(getattr(args, "radius", 0) or default)


def make_walker(args, default_radius):
    """The steps' random walk: radius as `walk_radius`, and the schedule switch — `args.walk_accel` (run_sample.py
    --walk_accel {0,1}; None = the environment variable IRN_WALK_ACCEL, else the library default 1) chooses between the
    truncated Chebyshev series of the operator and the reference's own count of 2^exp_times applications
    (misc/indexing.py:136-137); `args.walk_accel_tol_exp` = e moves the series' truncation bound to 10^-e."""
    from ..misc import indexing
    walker = indexing.RandomWalk(walk_radius(args, default_radius))
    accel = getattr(args, "walk_accel", None)
    if accel not in (None, ""):
        walker.set_option("accel", 1 if int(accel) else 0)
    tol = getattr(args, "walk_accel_tol_exp", None)
    if tol not in (None, "", 0):
        walker.set_option("accel_tol_exp", int(tol))
    return walker


def crf_iters(args):
    """--sem_seg_crf_iters: mean-field iterations of the score-seeded CRF behind the semantic labels, 0 = off."""
    return int(getattr(args, "sem_seg_crf_iters", 0) or 0)


def check_crf(args, step, thres, loader=True):
    """What a step with the CRF on refuses before any work: the CRF reads the decoded uint8 pixels on the device, which (for
    a step that reads its images through the `loader`) only the raw loader items hand over, and its unary takes the
    logarithm of the threshold."""
    from .. import ops
    if loader and not _io.device_preprocess(args):
        raise ValueError("%s: --sem_seg_crf_iters %d needs the decoded image on the device, which --device_preprocess False "
                         "does not hand over; turn one of the two off" % (step, crf_iters(args)))
    if not np.float32(thres) >= ops.CRF_SCORE_EPS:
        raise ValueError("%s: --sem_seg_crf_iters needs a background threshold of at least %g, got %r"
                         % (step, ops.CRF_SCORE_EPS, thres))


def rgb_pixels(p, raw, staging=None):
    """Keep an image's decoded pixels for the CRF: `raw` (host uint8 [H,W,3]) goes to the device once, stays as p["rgb"] and
    feeds the IRNet's input p["img"] — the same pixels for both, as in cam_to_ir_label."""
    from .. import ops
    p["rgb"] = _io.upload(raw, staging)
    p["img"] = ops.msf_pack(p["rgb"], (1.0,))[0]


def crf_planes(rws, sizes, keys, rgbs, names, thres, t, outs=None):
    """The CRF's label maps of a batch of walks: the epilogue's normalised scores (`rw_up`) instead of its labels, then per
    image one `crf_score_sweep` over the background thresholds `thres` -> uint8 [T,H,W] each, one at a time (a generator; into
    `outs[i]` where given)."""
    from .. import ops
    ups = ops.label_epilogue(rws, sizes, float(thres[0]), want_labels=False, want_rw_up=True)["rw_up"]
    for i, up in enumerate(ups):
        if up.shape[0] > 31:
            raise ValueError("%s: %d classes present, the CRF takes at most 31 per image" % (names[i], up.shape[0]))
        yield ops.crf_score_sweep(rgbs[i], up, keys[i], thres, t=t, out=None if outs is None else outs[i])


def crf_refine(rws, sizes, keys, rgbs, names, thres, t):
    """The label maps of a batch with the CRF on, at the single threshold `thres`: each image's map in its stretch of ONE flat
    uint8 buffer (what `label_epilogue(packed=True)` returns as 'labels_flat')."""
    offs = np.concatenate([[0], np.cumsum([hh * ww for hh, ww in sizes])])
    flat = torch.empty(int(offs[-1]), dtype=torch.uint8, device=rws[0].device)
    outs = [flat[int(offs[i]):int(offs[i + 1])].view(1, hh, ww) for i, (hh, ww) in enumerate(sizes)]
    for _ in crf_planes(rws, sizes, keys, rgbs, names, [thres], t, outs):
        pass
    return flat


def irn_batch(args):
    return int(getattr(args, "irn_batch", 0) or 8)              # images per IRNet trunk pass


def walk_batch(args, default):
    return int(getattr(args, "walk_batch", 0) or default)       # images per walk launch (results per image unchanged)


def edges_for(model, pend, irn_batch, store=None, model_key=None, dump_dir=None, auto=False):
    """EdgeDisplacement forward for the pending images, `irn_batch` at a time: ragged images are padded to the
    512^2 crop like the reference pads each one (net/resnet50_irn.py:225), so a chunk is ONE trunk pass.  With a `store`
    (`_stores.EDGE_STORE`) the maps the other label step already computed for an image (same network, same file) are taken
    from device memory instead, and what is computed here is left there for it.  `auto` (`--split_gemm auto`): the passes record
    the fp16-range flag per row; every image computed here gets `_split_flags` (device int32 [2]: image, flip) and keeps its
    `_edge_key` — `flag_read` sends the words to the host, `drop_flagged` acts on them.  A store hit is final and gets neither."""
    todo = pend
    if store is not None:
        todo = []
        for p in pend:
            key = (model_key, getattr(model, "crop_size", None), getattr(model, "stride", None), p.get("stamp"))
            dev = p["dev"] if "dev" in p else p["img"].device
            hit = store.get(key, dev) if p.get("stamp") is not None else None
            if hit is not None:
                p["edge"], p["dp"] = hit
                p.pop("img", None)
            else:
                p["_edge_key"] = key if p.get("stamp") is not None else None
                todo.append(p)
    for p in todo:
        if p.get("img") is None:
            # the loader skipped this image's pixels because the store held its maps then, and they are gone now (evicted
            # between the loader's look and this one): decode it here
            img = torch.from_numpy(np.array(Image.open(p["stamp"][0]).convert("RGB")))
            p["img"] = _io.device_images({"img": img[None]}, (1.0,))[0]
    for i in range(0, len(todo), irn_batch):
        chunk = todo[i:i + irn_batch]
        flags = torch.zeros(2 * len(chunk), dtype=torch.int32, device=chunk[0]["img"].device) if auto else None
        with _split_auto.recording(flags):
            maps = model.forward_batch([p.pop("img") for p in chunk])
        if auto:
            # an image that left the range is computed again later and nothing of this pass is written; until the host knows,
            # the walk and the instance kernels get zero maps for it instead of NaN (decided on the device)
            bad, zero = (flags.view(-1, 2) != 0).any(dim=1), flags.new_zeros((), dtype=torch.float32)
        for j, (p, (edge, dp)) in enumerate(zip(chunk, maps)):
            if auto:
                edge, dp = torch.where(bad[j], zero, edge), torch.where(bad[j], zero, dp)
            p["edge"], p["dp"] = edge, dp
            key = p.pop("_edge_key", None)
            if store is not None and key is not None:
                store.put(key, edge, dp.clone())         # dp is a view into the batch's output: keep 1 image, not 8
            if auto:
                p["_split_flags"], p["_edge_key"] = flags[2 * j:2 * j + 2], key
    if dump_dir:
        # verification aid (args.edge_out_dir, off by default): the maps this step walks on, per image, so that a run can be
        # checked against the oracle on ITS OWN inputs (the reference keeps them in memory only, step/make_sem_seg_labels.py:28-34).
        # Synchronous on purpose: not a production path
        os.makedirs(dump_dir, exist_ok=True)
        for p in pend:
            np.save(os.path.join(dump_dir, p["name"] + ".npy"), {"edge": p["edge"].cpu().numpy(), "dp": p["dp"].cpu().numpy()})


def flag_read(items):
    """`--split_gemm auto`: the flag words `edges_for(auto=True)` left with `items`, gathered ([2 n] int32, zeros for store hits)
    and sent to page-locked memory on the current stream -> the `_split_auto.FlagRead` to look at behind the batch's own
    read-back, or None when no image of the batch was computed here."""
    if not any("_split_flags" in p for p in items):
        return None
    zero = None
    words = []
    for p in items:
        f = p.get("_split_flags")
        if f is None:
            zero = f = zero if zero is not None else torch.zeros(2, dtype=torch.int32, device=p["edge"].device)
        words.append(f)
    read = _split_auto.FlagRead(torch.cat(words), [p["name"] for p in items])
    read.edge_keys = {p["name"]: p.get("_edge_key") for p in items}
    read.sizes = {p["name"]: p["size"] for p in items}
    return read


def drop_flagged(read, redo, store=None, wait=False):
    """Behind the batch's read-back: the names of the batch that left fp16's range (none without a `read`).  They go on the
    worker's `redo` list with their size, and the maps the split pass put into `store` for them are dropped; the caller writes
    no file for them."""
    if read is None:
        return set()
    bad = read.names(wait=wait)
    for name in bad:
        redo.add(name, read.sizes[name])
        if store is not None and read.edge_keys.get(name) is not None:
            store.drop(read.edge_keys[name])
    read.release()
    return set(bad)


def redo_items(redo, w, args):
    """The redo list as `item`s (pixels decoded again by `edges_for`), in name order, with their CAMs as they are NOW — the
    fp32 one where make_cam recomputed the image too."""
    cam_run = _stores.current_cam_run(args.cam_out_dir)
    todo = [item(name, size, w.dev, args, cam_run) for name, size in sorted(redo.items())]
    if w.keep_rgb:
        for p in todo:
            rgb_pixels(p, torch.from_numpy(np.array(Image.open(p["stamp"][0]).convert("RGB"))))
    return todo


def skip_image_predicate(model, args, device):
    """`skip_image` for the step's dataset: True for images whose boundary / displacement maps the other label step left on
    this device (the EdgeStore entry `edges_for` will hit) — their JPEG need not be decoded or uploaded."""
    kw = edge_store_kw(model, args)
    store = kw.get("store")
    if store is None:
        return None
    mk, crop, stride = kw["model_key"], getattr(model, "crop_size", None), getattr(model, "stride", None)
    return lambda name: store.peek((mk, crop, stride, _stores.image_stamp(args.voc12_root, name)), device)


_MODEL_KEYS = {}          # id(network) -> (weak reference to it, key of the ModelSpec it was built from); set in build_model


def remember_model(model, spec_key):
    """Note which checkpoint (class + path + mtime + size) a worker built `model` from: the identity the EdgeStore keys
    its entries by.  The weak reference guards against a later object reusing the id of a freed network."""
    for k in [k for k, (ref, _) in _MODEL_KEYS.items() if ref() is None]:
        del _MODEL_KEYS[k]
    _MODEL_KEYS[id(model)] = (weakref.ref(model), spec_key)


def model_key(model):
    hit = _MODEL_KEYS.get(id(model))
    return hit[1] if hit is not None and hit[0]() is model else None


def edge_store_kw(model, args):
    """Keyword arguments of `edges_for` that switch the device hand-off of the edge maps on (see _stores.EdgeStore)."""
    dump = {"dump_dir": args.edge_out_dir} if getattr(args, "edge_out_dir", None) else {}
    if not _stores.keep_edges(args):
        return dump
    key = model_key(model)
    if key is None:
        # a network handed over as a module (not built from a ModelSpec) has no identity that survives an in-place weight
        # update or a recycled id(): no hand-off for it, every step computes its own maps
        return dump
    return {"store": _stores.EDGE_STORE, "model_key": key, **dump}


def build_model(model):
    """A network, or the (class, checkpoint) a worker builds it from -> the network, remembered under its checkpoint's key."""
    spec_key = model.key() if isinstance(model, _pool.ModelSpec) else None
    model = _pool.materialise(model)
    if spec_key is not None:
        remember_model(model, spec_key)
    return model


def item(name, size, dev, args, cam_run):
    """What a step keeps per image; `img` is the caller's to fill in.  The CAM: from the device if make_cam left it there, else its file."""
    keys, keys_dev, cam = _stores.CAM_STORE.get(name, args.cam_out_dir, dev, cam_run, _stores.keep_cams(args))
    return {"name": name, "size": size, "img": None, "dev": dev, "cam": cam, "keys": keys, "keys_dev": keys_dev,
            "stamp": _stores.image_stamp(args.voc12_root, name)}


@contextlib.contextmanager
def worker(process_id, model, dataset, args, keep_rgb=False):
    """One shard of a label step on its worker's device.  Walker (its context and device buffers) and writer are closed however
    the block ends; the walk's fall-back count and the step's summary line come only after a block that ended well.
    `keep_rgb`: every item keeps its decoded pixels on the device (`rgb_pixels`), so no image's pixels are skipped."""
    model = build_model(model)
    dev = torch.device("cuda", _pool.worker_device(process_id, args))
    with _io.shard_io(process_id, dataset, args) as (databin, n_gpus, loader, writer), torch.no_grad(), torch.cuda.device(dev):
        _io.set_skip_image(databin, None if keep_rgb else skip_image_predicate(model, args, dev))
        model.cuda()
        with contextlib.closing(make_walker(args, RADIUS)) as walker:
            yield types.SimpleNamespace(model=model, walker=walker, writer=writer, loader=loader, dev=dev, databin=databin,
                                        n_gpus=n_gpus, process_id=process_id, keep_rgb=keep_rgb)
            _report.WALK_STATS["fallback_runs"] += walker.fallback_runs
            _report.step_summary(process_id, walker)


@contextlib.contextmanager
def tuning(args, dev):
    """The frame of a tuner (tune_sem_seg, tune_ins_seg) in the caller's process on `dev`: the label steps' MIOpen settings and
    reproducible mode (`process_mode`), their network and their walker -> (model, walker).  The walker is closed however the
    block ends.  A tuner whose loop ended well calls `end_walk(walker)` itself, before its read-backs and checks: those come
    after the walker is closed and still belong inside the mode."""
    with _tuned.process_mode(dev.index), torch.no_grad(), torch.cuda.device(dev):
        model = build_model(_pool.ModelSpec(args.irn_network, "EdgeDisplacement", args.irn_weights_name, strict=False))
        model.cuda()
        with contextlib.closing(make_walker(args, RADIUS)) as walker:
            yield model, walker


def end_walk(walker):
    """After a tuner's loop that ended well: the walk's fall-back count goes to WALK_STATS, the walker is closed."""
    _report.WALK_STATS["fallback_runs"] += walker.fallback_runs
    walker.close()


def items(w, args):
    """The shard's images in order, each as `item` with its pixels on the device (`img` None where the skip predicate emptied them)."""
    cam_run = _stores.current_cam_run(args.cam_out_dir)
    for it, pack in enumerate(w.loader):
        name = pack["name"][0]
        name = name if isinstance(name, str) else voc12_dataloader.decode_int_filename(name)
        p = item(name, (int(pack["size"][0]), int(pack["size"][1])), w.dev, args, cam_run)
        if w.keep_rgb:
            rgb_pixels(p, pack["img"][0], pack.pop("_staging", None))
        else:
            imgs = _io.device_images(pack, (1.0,))
            p["img"] = None if imgs is None else imgs[0]
        yield p
        _io.progress(w.process_id, w.n_gpus, it, len(w.databin))


def run_step(work, out_dir, args, opening="["):
    """`run(args)` of a label step: `work` on every shard of `args.infer_list`, inside the reference's bracket (`opening`)."""
    model = _pool.ModelSpec(args.irn_network, "EdgeDisplacement", args.irn_weights_name, strict=False)   # built by the worker(s)
    n_gpus = _pool.n_gpus_or_raise(args)
    dataset = voc12_dataloader.VOC12ClassificationDatasetMSF(args.infer_list, voc12_root=args.voc12_root,
                                                             scales=(1.0,), raw=_io.device_preprocess(args))
    dataset = _stores.label_step_shards(dataset, n_gpus, args)     # strided (misc/torchutils.py:66-68) or CAM-owner aware
    os.makedirs(out_dir, exist_ok=True)
    print(opening, end="")
    _pool.spawn_workers(work, model, dataset, args)
    print("]")
