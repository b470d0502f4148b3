"""Host logic the tuning steps share (tune_sem_seg, tune_ins_seg, tune_ir_label): how a threshold axis is built and refused,
the (beta, exp_times) axes of the two walk tuners, the configured point, the best point, the split and its JPEGs, and the
frame of a walk tuner's `run`.  What a step counts per batch and how it reports stay in the step's own module."""
import numpy as np
import torch
from PIL import Image

from .. import ops
from ..voc12 import dataloader as voc12_dataloader
from ..voc12 import eval_data
from . import _classes, _eval, _io, _labels, _report, _stores

MAX_PAIRS = 64                        # (beta, exp_times) pairs = walks per batch


def threshold_axis(value, extra, what, limit, step):
    """-> (the values as requested, the same as ascending float32) of the axis of `what` ("background" / "foreground")
    thresholds: the configured `value` and the `extra` ones, sorted and without repeats.  Values are told apart as float32 (the
    kernels compare in float32) and the first spelling of a float32 value names it."""
    req = {}
    for t in [float(value)] + [float(t) for t in (extra or ())]:
        req.setdefault(float(np.float32(t)), t)
    th32 = np.unique(np.asarray(list(req), np.float32))
    if np.isnan(th32).any():
        raise ValueError("%s: a %s threshold is NaN" % (step, what))
    if th32.size > limit:
        raise ValueError("%s: %d %s thresholds (at most %d)" % (step, th32.size, what, limit))
    return [req[float(t)] for t in th32], th32


def walk_axes(args, thres, tune_thres, max_thres, step):
    """-> (betas, exp_times, thresholds as requested, the same as ascending float32) of a walk tuner: every axis holds the
    configured value, sorted and without repeats.  `thres` / `tune_thres` name the threshold's two attributes of `args`."""
    betas = sorted({float(args.beta)} | {float(b) for b in (getattr(args, "tune_beta", None) or ())})
    exps = sorted({int(args.exp_times)} | {int(e) for e in (getattr(args, "tune_exp_times", None) or ())})
    req, th32 = threshold_axis(getattr(args, thres), getattr(args, tune_thres, None), "background", max_thres, step)
    if len(betas) * len(exps) > MAX_PAIRS:
        raise ValueError("%s: %d beta x %d exp_times = %d walks per image (at most %d)"
                         % (step, len(betas), len(exps), len(betas) * len(exps), MAX_PAIRS))
    if any(e < 0 for e in exps):
        raise ValueError("%s: exp_times must not be negative" % step)
    return betas, exps, req, th32


def configured(req, th32, value):
    """The spelling on the axis (req, th32) of the configured `value`, which `threshold_axis` has put there."""
    return req[int(np.searchsorted(th32, np.float32(value)))]


def pick_best(grid, tie_order):
    """The grid point of the highest score; ties go to the smaller coordinate, the coordinates taken in `tie_order` (a NaN
    never wins against a number)."""
    def rank(point):
        m = grid[point]
        return (m == m, m if m == m else 0.0) + tuple(-point[i] for i in tie_order)
    return max(grid, key=rank)


def split_ids(args):
    return eval_data.seg_ids(args.voc12_root, args.chainer_eval_set)


def refuse_empty(ids, args, step):
    if not ids:
        raise ValueError("%s: the split %s lists no images" % (step, args.chainer_eval_set))


def jpeg(args, id, gt_shape):
    """The image as RGB uint8 [H,W,3], checked against the shape of its ground truth."""
    img = np.array(Image.open(voc12_dataloader.get_img_path(id, args.voc12_root)).convert("RGB"))
    _eval.check_shape(id, "image", img.shape[:2], gt_shape)
    return img


def batches(iterable, n):
    """Lists of up to n consecutive items, the last one as short as it comes."""
    pend = []
    for item in iterable:
        pend.append(item)
        if len(pend) == n:
            yield pend
            pend = []
    if pend:
        yield pend


def run_walk(args, step, grid_axes, thres, load, gt_key, what, default_batch, counter, keep_rgb=False):
    """`run` of a walk tuner up to its report -> (what `finish` returns, axes, the configured point).

    grid_axes(args) -> `walk_axes`; `thres` names the configured threshold in `args`.  load(id, c) -> the image's ground truth
    and, under "image", its `jpeg`; the map under `gt_key` gives the image's size and an image without class keys has no
    `what` to score.  counter(axes, c, dev, bad) -> (count(model, walker, pend) for one batch of `_labels.item` dicts, which
    also hold what `load` returned; finish() for the read-backs once `bad` has been checked).  c = --num_classes.
    `keep_rgb`: every item keeps its decoded pixels on the device under "rgb" (what the IRNet's input is packed from).
    Refusals come in this order: no split file, the grid, an empty split, no GPU — all before any image is read."""
    ids = split_ids(args)
    axes = grid_axes(args)
    point = (float(args.beta), int(args.exp_times), configured(axes[2], axes[3], getattr(args, thres)))
    refuse_empty(ids, args, step)
    dev = _eval.device()
    c = _classes.num_classes(args)
    with _labels.tuning(args, dev) as (model, walker):
        batch = _labels.walk_batch(args, default_batch)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        count, finish = counter(axes, c, dev, bad)
        cam_run = _stores.current_cam_run(args.cam_out_dir)

        def items():
            for id, it in _eval.items(ids, lambda id: load(id, c), args):
                p = _labels.item(id, tuple(int(v) for v in it[gt_key].shape), dev, args, cam_run)
                if p["keys"].numel() == 0:
                    raise ValueError("%s: %s has no class key in %s: an image without a CAM has no %s to score"
                                     % (step, id, args.cam_out_dir, what))
                rgb = _io.upload(it.pop("image"))
                if keep_rgb:
                    p["rgb"] = rgb
                p["img"] = ops.msf_pack(rgb, (1.0,))[0]
                p.update(it)
                yield p
        for pend in batches(items(), batch):
            count(model, walker, pend)
            pend.clear()                     # the batch's device tensors go before the next batch is read
        _labels.end_walk(walker)             # before the read-backs and checks, which still belong inside the mode
        _eval.raise_if_bad(bad, step, c)
        out = finish()
        _report.check_split_overflow(step)
    return out, axes, point
