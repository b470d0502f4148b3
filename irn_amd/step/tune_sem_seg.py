"""Tuning step (not in the reference): score a grid of --beta x --exp_times x --sem_seg_bg_thres against the ground truth
in ONE pass over the split — what make_sem_seg_labels + eval_sem_seg give per grid point, without a label file.

Reads  args.voc12_root (ImageSets/Segmentation/<args.chainer_eval_set>.txt, JPEGImages/<id>.jpg, SegmentationClass/<id>.png),
       args.cam_out_dir/<id>.npy (`cam` / `keys` of make_cam), args.irn_network, args.irn_weights_name,
       args.beta, args.exp_times, args.sem_seg_bg_thres (the configured point: always on the grid),
       args.tune_beta, args.tune_exp_times, args.tune_bg_thres (more values per axis)
Prints the lines of eval_sem_seg at the configured point, one `beta .. exp_times .. thres .. miou ..` line per grid point and
       the best one; returns {'iou', 'miou', 'grid': {(beta, exp_times, thres): miou}, 'ious': {... : iou}, 'best': (beta,
       exp_times, thres)}.  Writes nothing.

The boundary map of an image does not depend on the three numbers: per batch the IRNet runs once (`edges_for`, as the label
step runs it), every (beta, exp_times) pair costs one walk, and `ops.label_sweep_confusion` counts every threshold of that
walk in one pass (one histogram of (GT, first arg-max class, number of thresholds below its score)).  The
walker, its batches and the IRNet batches are those of make_sem_seg_labels, and the counting kernel computes its scores with
the label epilogue's own device functions, so a grid point's counts are those of the files the two steps would have written.  Runs in the
calling process on its current device like the evaluation steps (step/_eval.py)."""
import numpy as np
import torch
from PIL import Image

from .. import ops
from ..misc import evaluation
from ..voc12 import dataloader as voc12_dataloader
from ..voc12 import eval_data
from . import _classes, _eval, _io, _labels, _report, _stores

MAX_PAIRS = 64                        # (beta, exp_times) pairs = walks per batch


def grid_axes(args, thres="sem_seg_bg_thres", tune_thres="tune_bg_thres", max_thres=ops.EVAL_MAX_THRES, step="tune_sem_seg"):
    """-> (betas, exp_times, thresholds as requested, the same as ascending float32): every axis holds the configured value,
    sorted and without repeats; thresholds are told apart as float32 (the label epilogue compares in float32).  The keywords
    name the threshold's two attributes of `args`, its limit and the step the refusals speak for (tune_ins_seg has its own)."""
    betas = sorted({float(args.beta)} | {float(b) for b in (getattr(args, "tune_beta", None) or ())})
    exps = sorted({int(args.exp_times)} | {int(e) for e in (getattr(args, "tune_exp_times", None) or ())})
    req = {}
    for t in [float(getattr(args, thres))] + [float(t) for t in (getattr(args, tune_thres, None) or ())]:
        req.setdefault(float(np.float32(t)), t)              # the first spelling of a float32 value names it
    th32 = np.unique(np.asarray(list(req), np.float32))
    if np.isnan(th32).any():
        raise ValueError("%s: a background threshold is NaN" % step)
    if th32.size > max_thres:
        raise ValueError("%s: %d background thresholds (at most %d)" % (step, th32.size, max_thres))
    if len(betas) * len(exps) > MAX_PAIRS:
        raise ValueError("%s: %d beta x %d exp_times = %d walks per image (at most %d)"
                         % (step, len(betas), len(exps), len(betas) * len(exps), MAX_PAIRS))
    if any(e < 0 for e in exps):
        raise ValueError("%s: exp_times must not be negative" % step)
    return betas, exps, [req[float(t)] for t in th32], th32


def pick_best(grid):
    """The grid point of the highest mIoU; ties go to the smaller exp_times, then the smaller beta, then the smaller
    threshold (a NaN mIoU never wins against a number)."""
    def rank(point):
        m = grid[point]
        return (m == m, m if m == m else 0.0, -point[1], -point[0], -point[2])
    return max(grid, key=rank)


def report(conf, void, axes, configured):
    """Scores of every grid point from conf int64 [P,T,nc,nc] / void int64 [P,T,nc] (nc = --num_classes + 1; pairs in beta-major order), printed in
    the step's format; returns the step's dict."""
    betas, exps, req, _ = axes
    grid, ious = {}, {}
    for p, (b, e) in enumerate((b, e) for b in betas for e in exps):
        for i, t in enumerate(req):
            s = evaluation.sem_seg_scores(conf[p, i], void[p, i])
            ious[(b, e, t)] = s["iou"]
            grid[(b, e, t)] = evaluation.nanmean(s["iou"])
            if (b, e, t) == configured:
                here = s
    print(here["fp"][0], here["fn"][0])
    print(evaluation.mean(here["fp"][1:]), evaluation.mean(here["fn"][1:]))
    out = {"iou": here["iou"], "miou": evaluation.nanmean(here["iou"])}
    print(out)
    for (b, e, t), m in grid.items():
        print("beta %g exp_times %d thres %g miou %.6f" % (b, e, t, m))
    best = pick_best(grid)
    print("best beta %g exp_times %d thres %g miou %.6f" % (best + (grid[best],)))
    out.update(grid=grid, ious=ious, best=best)
    return out


def _count(model, walker, pend, pairs, th, hist, bad, args, nc):
    """One batch: the boundary maps once, then per (beta, exp_times) a walk and the count of every threshold."""
    _labels.edges_for(model, pend, _labels.irn_batch(args), **_labels.edge_store_kw(model, args))
    edges, cams = [p["edge"] for p in pend], [p["cam"] for p in pend]
    sizes, keys = [p["size"] for p in pend], [p["keys_dev"] for p in pend]
    gts = _io.upload(torch.cat([p["gt"].reshape(-1) for p in pend]))     # the batch's maps back to back: one copy
    for p, (beta, exp_times) in enumerate(pairs):
        rws = walker(edges, cams, beta=beta, exp_times=exp_times)
        # before the count, not after: the count adds into an accumulator and cannot be redone once a fallback re-run has
        # replaced the walk's outputs
        walker.sync()
        _, bad = ops.label_sweep_confusion(rws, sizes, keys, gts, th, hist[p], bad, n_classes=nc)
    pend.clear()
    return bad


def run(args):
    ids = eval_data.seg_ids(args.voc12_root, args.chainer_eval_set)
    axes = grid_axes(args)
    betas, exps, req, th32 = axes
    pairs = [(b, e) for b in betas for e in exps]
    configured = (float(args.beta), int(args.exp_times), req[int(np.searchsorted(th32, np.float32(args.sem_seg_bg_thres)))])
    if not ids:
        raise ValueError("tune_sem_seg: the split %s lists no images" % args.chainer_eval_set)
    dev = _eval.device()
    nc = _classes.num_classes(args) + 1

    def load(id):
        gt = eval_data.class_label(args.voc12_root, id)
        img = np.array(Image.open(voc12_dataloader.get_img_path(id, args.voc12_root)).convert("RGB"))
        _eval.check_shape(id, "image", img.shape[:2], gt.shape)
        return {"gt": gt, "image": img}

    with _labels.tuning(args, dev) as (model, walker):
        batch = _labels.walk_batch(args, 64)
        th = torch.from_numpy(th32).to(dev)
        hist = torch.zeros((len(pairs), nc + 1, nc, len(th32) + 1), dtype=torch.int64, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        cam_run = _stores.current_cam_run(args.cam_out_dir)
        pend = []
        for id, it in _eval.items(ids, load, args):
            p = _labels.item(id, tuple(int(v) for v in it["gt"].shape), dev, args, cam_run)
            if p["keys"].numel() == 0:
                raise ValueError("tune_sem_seg: %s has no class key in %s: an image without a CAM has no label to score"
                                 % (id, args.cam_out_dir))
            p.update(img=ops.msf_pack(_io.upload(it["image"]), (1.0,))[0], gt=it["gt"])
            pend.append(p)
            if len(pend) == batch:
                bad = _count(model, walker, pend, pairs, th, hist, bad, args, nc)
        if pend:
            bad = _count(model, walker, pend, pairs, th, hist, bad, args, nc)
        _labels.end_walk(walker)             # before the read-backs and checks, which still belong inside the mode
        _eval.raise_if_bad(bad, "tune_sem_seg", nc - 1)
        conf, void = zip(*(ops.cam_confusion_matrices(hist[p], n_classes=nc) for p in range(len(pairs))))
        conf, void = torch.stack(conf).cpu().numpy(), torch.stack(void).cpu().numpy()
        _report.check_split_overflow("tune_sem_seg")
    return report(conf, void, axes, configured)
