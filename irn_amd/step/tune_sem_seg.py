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
calling process on its current device like the evaluation steps (step/_eval.py).
With args.sem_seg_crf_iters T > 0 the grid is scored on the CRF-refined maps make_sem_seg_labels writes with the same flag
(DESIGN.md §29): per walk the epilogue hands over its normalised scores, `ops.crf_score_sweep` runs every threshold of an
image in one call (at most IRN_CRF_MAX_SWEEP = 16 thresholds) and `ops.label_confusion` counts each plane.  The image's
lattices are rebuilt for every (beta, exp_times) pair: they depend on the pixels only, but sharing them across walks would
keep every image's lattices of a batch alive at once.  With T = 0 the step is what it was.
The grid rules and the frame of `run` (refusals, batches, checks) are step/_tune.py's, shared with tune_ins_seg."""
import functools

import torch

from .. import ops
from ..misc import evaluation
from ..voc12 import eval_data
from . import _io, _labels, _tune

MAX_PAIRS = _tune.MAX_PAIRS
_walk_axes = functools.partial(_tune.walk_axes, thres="sem_seg_bg_thres", tune_thres="tune_bg_thres", max_thres=ops.EVAL_MAX_THRES,
                               step="tune_sem_seg")


def grid_axes(args):
    """`_tune.walk_axes` of the step.  With --sem_seg_crf_iters on every threshold is one CRF per image and walk: at most
    IRN_CRF_MAX_SWEEP of them, each at least the unary's clip."""
    axes = _walk_axes(args)
    if _labels.crf_iters(args):
        th32 = axes[3]
        if th32.size > ops.CRF_MAX_SWEEP:
            raise ValueError("tune_sem_seg: %d background thresholds with --sem_seg_crf_iters on (at most IRN_CRF_MAX_SWEEP = %d: "
                             "each one is a CRF per image and walk)" % (th32.size, ops.CRF_MAX_SWEEP))
        _labels.check_crf(args, "tune_sem_seg", th32.min(), loader=False)
    return axes
# ties go to the smaller exp_times, then the smaller beta, then the smaller threshold
pick_best = functools.partial(_tune.pick_best, tie_order=(1, 0, 2))


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


def run(args):
    def load(id, c):
        gt = eval_data.class_label(args.voc12_root, id)
        return {"gt": gt, "image": _tune.jpeg(args, id, gt.shape)}

    def counter(axes, c, dev, bad):
        pairs = [(b, e) for b in axes[0] for e in axes[1]]
        th = torch.from_numpy(axes[3]).to(dev)
        hist = torch.zeros((len(pairs), c + 2, c + 1, len(th) + 1), dtype=torch.int64, device=dev)

        def count(model, walker, pend):
            """One batch: the boundary maps once, then per (beta, exp_times) a walk and the count of every threshold."""
            _labels.edges_for(model, pend, _labels.irn_batch(args), **_labels.edge_store_kw(model, args))
            edges, cams = [p["edge"] for p in pend], [p["cam"] for p in pend]
            sizes, keys = [p["size"] for p in pend], [p["keys_dev"] for p in pend]
            gts = _io.upload(torch.cat([p["gt"].reshape(-1) for p in pend]))     # the batch's maps back to back: one copy
            for p, (beta, exp_times) in enumerate(pairs):
                rws = walker(edges, cams, beta=beta, exp_times=exp_times)
                # before the count, not after: the count adds into an accumulator and cannot be redone once a fallback re-run
                # has replaced the walk's outputs
                walker.sync()
                ops.label_sweep_confusion(rws, sizes, keys, gts, th, hist[p], bad, n_classes=c + 1)

        def finish():
            conf, void = zip(*(ops.cam_confusion_matrices(hist[p], n_classes=c + 1) for p in range(len(pairs))))
            return torch.stack(conf).cpu().numpy(), torch.stack(void).cpu().numpy()
        return count, finish

    def crf_counter(axes, c, dev, bad):
        """The counter with --sem_seg_crf_iters on.  A CRF map is not monotone in the threshold, so the threshold histogram
        does not apply: every plane of the image's sweep is counted as eval_sem_seg counts a file."""
        pairs = [(b, e) for b in axes[0] for e in axes[1]]
        th32 = axes[3]
        conf = torch.zeros((len(pairs), len(th32), c + 1, c + 1), dtype=torch.int64, device=dev)
        void = torch.zeros((len(pairs), len(th32), c + 1), dtype=torch.int64, device=dev)

        def count(model, walker, pend):
            _labels.edges_for(model, pend, _labels.irn_batch(args), **_labels.edge_store_kw(model, args))
            edges, cams = [p["edge"] for p in pend], [p["cam"] for p in pend]
            sizes, keys = [p["size"] for p in pend], [p["keys_dev"] for p in pend]
            rgbs, names = [p["rgb"] for p in pend], [p["name"] for p in pend]
            gts = _io.upload(torch.cat([p["gt"].reshape(-1) for p in pend]))
            for p, (beta, exp_times) in enumerate(pairs):
                rws = walker(edges, cams, beta=beta, exp_times=exp_times)
                walker.sync()                # as above: the counts cannot be redone after a fallback re-run
                off = 0
                for i, planes in enumerate(_labels.crf_planes(rws, sizes, keys, rgbs, names, th32, crf_t)):
                    gt = gts[off:off + planes[0].numel()].view(planes.shape[1:])
                    off += planes[0].numel()
                    for j in range(len(th32)):
                        ops.label_confusion(planes[j], gt, conf[p, j], bad, pred_255_as=0, void=void[p, j], n_classes=c + 1)

        def finish():
            return conf.cpu().numpy(), void.cpu().numpy()
        return count, finish

    crf_t = _labels.crf_iters(args)
    (conf, void), axes, configured = _tune.run_walk(args, "tune_sem_seg", grid_axes, "sem_seg_bg_thres", load, "gt", "label", 64,
                                                    crf_counter if crf_t else counter, keep_rgb=crf_t > 0)
    return report(conf, void, axes, configured)

