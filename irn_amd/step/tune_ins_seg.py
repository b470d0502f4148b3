"""Tuning step (not in the reference): score a grid of --beta x --exp_times x --ins_seg_bg_thres against the ground truth in
ONE pass over the split — what make_ins_seg_labels + eval_ins_seg give per grid point, without a detection file and without
a dense mask.

Reads  args.voc12_root (ImageSets/Segmentation/<args.chainer_eval_set>.txt, JPEGImages/<id>.jpg, SegmentationObject/<id>.png,
       SegmentationClass/<id>.png), args.cam_out_dir/<id>.npy (`cam` / `keys` of make_cam), args.irn_network,
       args.irn_weights_name, args.beta, args.exp_times, args.ins_seg_bg_thres (the configured point: always on the grid),
       args.tune_beta, args.tune_exp_times (shared with tune_sem_seg), args.tune_ins_bg_thres (more values per axis)
Prints `0.5iou: {...}` of eval_ins_seg at the configured point, one `beta .. exp_times .. thres .. map ..` line per grid point
       and the best one; returns {'ap', 'map', 'grid': {(beta, exp_times, thres): map}, 'aps': {... : ap}, 'best': (beta,
       exp_times, thres)}.  Writes nothing.

The IRNet forward, the centroid refinement and the clustering of an image do not depend on the three numbers: per batch they
run once (`edges_for`, `make_ins_seg_labels.instance_front`, as the label step runs them).  Every (beta, exp_times) pair costs
one walk and one label epilogue at the LOWEST threshold of the grid; a higher threshold only turns pixels of that argmax map
into background (`ops.argmax_rethreshold_batch`), and `ops.detection_overlap_batch` counts the detections of the map against
the GT instances straight from the labelled map.  The counts are the integers eval_ins_seg's `ops.mask_overlap`
counts on the label step's files and go through the same host AP code, so a grid point's scores are those of the two steps.

An image without any detection at a grid point: the label step writes no file for it and eval_ins_seg would then fail on the
missing file.  Here such an image counts as ZERO detections at that point — its GT instances still count as positives.

Runs in the calling process on its current device like the evaluation steps (step/_eval.py).
The grid rules and the frame of `run` (refusals, batches, checks) are step/_tune.py's, shared with tune_sem_seg."""
import functools

import numpy as np
import torch

from .. import ops
from ..misc import evaluation
from ..voc12 import eval_data
from . import _io, _labels, _tune, make_ins_seg_labels

MAX_THRES = 64                        # thresholds: each one is a labelling pass per walk
grid_axes = functools.partial(_tune.walk_axes, thres="ins_seg_bg_thres", tune_thres="tune_ins_bg_thres", max_thres=MAX_THRES,
                              step="tune_ins_seg")
# ties go to the smaller exp_times, then the smaller beta, then the smaller threshold
pick_best = functools.partial(_tune.pick_best, tie_order=(1, 0, 2))


def report(records, axes, configured):
    """Scores of every grid point from records {(beta, exp_times, thres): per-image records in split order} (what
    `evaluation.instance_ap_voc` takes), printed in the step's format; returns the step's dict."""
    betas, exps, req, _ = axes
    grid, aps = {}, {}
    for point in ((b, e, t) for b in betas for e in exps for t in req):
        s = evaluation.instance_ap_voc(records[point], iou_thresh=0.5)
        aps[point], grid[point] = s["ap"], s["map"]
        if point == configured:
            here = s
    print("0.5iou:", here)
    for (b, e, t), m in grid.items():
        print("beta %g exp_times %d thres %g map %.6f" % (b, e, t, m))
    best = pick_best(grid)
    print("best beta %g exp_times %d thres %g map %.6f" % (best + (grid[best],)))
    return {"ap": here["ap"], "map": here["map"], "grid": grid, "aps": aps, "best": best}


def run(args):
    def load(id, c):
        inst_map, inst_class = eval_data.instance_label(args.voc12_root, id, n_fg=c)
        return {"inst_map": inst_map, "inst_class": inst_class, "image": _tune.jpeg(args, id, inst_map.shape)}

    def counter(axes, c, dev, bad):
        betas, exps, req, th32 = axes
        records = {(b, e, t): [] for b in betas for e in exps for t in req}

        def count(model, walker, pend):
            """One batch: boundary maps, centroids and clusters once; per (beta, exp_times) one walk and one epilogue at the
            lowest threshold; per threshold the map at that threshold and the overlap counts of its detections."""
            _labels.edges_for(model, pend, _labels.irn_batch(args), **_labels.edge_store_kw(model, args))
            cmaps, k_dev = make_ins_seg_labels.instance_front(pend)
            ks = [int(k) for k in k_dev.cpu().tolist()]
            edges, cams, sizes = [p["edge"] for p in pend], [p["cam"] for p in pend], [p["size"] for p in pend]
            insts = [_io.upload(p["inst_map"]) for p in pend]
            gt_class = [p["inst_class"].numpy() for p in pend]
            gs = [len(g) for g in gt_class]
            n_ch = [p["cam"].shape[0] * k for p, k in zip(pend, ks)]
            class_ids = [np.repeat(np.asarray(torch.as_tensor(p["keys"]).cpu()), k) for p, k in zip(pend, ks)]
            min_area = [s[0] * s[1] * 0.01 for s in sizes]
            for b in betas:
                for e in exps:
                    rws = walker(edges, cams, beta=b, exp_times=e, inst_maps=cmaps, k_inst=ks)

                    def epilogue():
                        return ops.label_epilogue(rws, sizes, float(th32[0]), want_labels=False, want_argmax=True, want_rw_up=True)
                    ep = epilogue()
                    if walker.sync():           # the persistent walk gave up and the batch was re-run on the streaming sweeps
                        ep = epilogue()
                    for i, t in enumerate(req):
                        am = ep["argmax"] if i == 0 else ops.argmax_rethreshold_batch(ep["rw_up"], ep["argmax"], float(th32[i]))
                        recs = ops.detection_overlap_batch(ep["rw_up"], am, class_ids, n_ch, min_area, insts, gs, bad)
                        for rec, g in zip(recs, gt_class):
                            rec["gt_class"] = g
                        records[(b, e, t)] += recs
        return count, lambda: records

    records, axes, configured = _tune.run_walk(args, "tune_ins_seg", grid_axes, "ins_seg_bg_thres", load, "inst_map", "instance",
                                               32, counter)
    return report(records, axes, configured)
