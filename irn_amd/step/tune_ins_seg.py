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

Runs in the calling process on its current device like the evaluation steps (step/_eval.py)."""
import numpy as np
import torch
from PIL import Image

from .. import ops
from ..misc import evaluation
from ..voc12 import dataloader as voc12_dataloader
from ..voc12 import eval_data
from . import _classes, _eval, _io, _labels, _report, _stores, make_ins_seg_labels
from .tune_sem_seg import grid_axes as _grid_axes
from .tune_sem_seg import pick_best

MAX_THRES = 64                        # thresholds: each one is a labelling pass per walk


def grid_axes(args):
    """`tune_sem_seg.grid_axes` on this step's threshold (--ins_seg_bg_thres / --tune_ins_bg_thres, at most MAX_THRES)."""
    return _grid_axes(args, thres="ins_seg_bg_thres", tune_thres="tune_ins_bg_thres", max_thres=MAX_THRES, step="tune_ins_seg")


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


def _count(model, walker, pend, axes, records, bad, args):
    """One batch: boundary maps, centroids and clusters once; per (beta, exp_times) one walk and one epilogue at the lowest
    threshold; per threshold the map at that threshold and the overlap counts of its detections."""
    betas, exps, req, th32 = axes
    _labels.edges_for(model, pend, _labels.irn_batch(args), **_labels.edge_store_kw(model, args))
    cmaps, k_dev = make_ins_seg_labels.instance_front(pend)
    ks = [int(k) for k in k_dev.cpu().tolist()]
    edges, cams, sizes = [p["edge"] for p in pend], [p["cam"] for p in pend], [p["size"] for p in pend]
    insts = [_io.upload(p["inst_map"]) for p in pend]
    gs = [len(p["gt_class"]) for p in pend]
    n_ch = [p["cam"].shape[0] * k for p, k in zip(pend, ks)]
    class_ids = [np.repeat(np.asarray(torch.as_tensor(p["keys"]).cpu()), k) for p, k in zip(pend, ks)]
    min_area = [s[0] * s[1] * 0.01 for s in sizes]
    for b in betas:
        for e in exps:
            rws = walker(edges, cams, beta=b, exp_times=e, inst_maps=cmaps, k_inst=ks)

            def epilogue():
                return ops.label_epilogue(rws, sizes, float(th32[0]), want_labels=False, want_argmax=True, want_rw_up=True)
            ep = epilogue()
            if walker.sync():                   # the persistent walk gave up and the batch was re-run on the streaming sweeps
                ep = epilogue()
            for i, t in enumerate(req):
                am = ep["argmax"] if i == 0 else ops.argmax_rethreshold_batch(ep["rw_up"], ep["argmax"], float(th32[i]))
                recs = ops.detection_overlap_batch(ep["rw_up"], am, class_ids, n_ch, min_area, insts, gs, bad)
                for p, rec in zip(pend, recs):
                    rec["gt_class"] = p["gt_class"]
                records[(b, e, t)] += recs
    pend.clear()


def run(args):
    ids = eval_data.seg_ids(args.voc12_root, args.chainer_eval_set)
    axes = grid_axes(args)
    betas, exps, req, th32 = axes
    configured = (float(args.beta), int(args.exp_times), req[int(np.searchsorted(th32, np.float32(args.ins_seg_bg_thres)))])
    if not ids:
        raise ValueError("tune_ins_seg: the split %s lists no images" % args.chainer_eval_set)
    dev = _eval.device()
    c = _classes.num_classes(args)

    def load(id):
        inst_map, inst_class = eval_data.instance_label(args.voc12_root, id, n_fg=c)
        img = np.array(Image.open(voc12_dataloader.get_img_path(id, args.voc12_root)).convert("RGB"))
        _eval.check_shape(id, "image", img.shape[:2], inst_map.shape)
        return {"inst_map": inst_map, "inst_class": inst_class, "image": img}

    records = {(b, e, t): [] for b in betas for e in exps for t in req}
    with _labels.tuning(args, dev) as (model, walker):
        batch = _labels.walk_batch(args, 32)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        cam_run = _stores.current_cam_run(args.cam_out_dir)
        pend = []
        for id, it in _eval.items(ids, load, args):
            p = _labels.item(id, tuple(int(v) for v in it["inst_map"].shape), dev, args, cam_run)
            if p["keys"].numel() == 0:
                raise ValueError("tune_ins_seg: %s has no class key in %s: an image without a CAM has no instance to score"
                                 % (id, args.cam_out_dir))
            p.update(img=ops.msf_pack(_io.upload(it["image"]), (1.0,))[0], inst_map=it["inst_map"],
                     gt_class=it["inst_class"].numpy())
            pend.append(p)
            if len(pend) == batch:
                _count(model, walker, pend, axes, records, bad, args)
        if pend:
            _count(model, walker, pend, axes, records, bad, args)
        _labels.end_walk(walker)             # before the read-backs and checks, which still belong inside the mode
        _eval.raise_if_bad(bad, "tune_ins_seg", c)
        _report.check_split_overflow("tune_ins_seg")
    return report(records, axes, configured)
