#!/usr/bin/env python3
"""CLI boundary — same flags and step order as reference run_sample.py:8-137, for the steps this repository
implements: the label-generation steps (make_cam, cam_to_ir_label, make_ins_seg, make_sem_seg), the evaluation
steps that score them (eval_cam, eval_ins_seg, eval_sem_seg), the grid search over the semantic labels' three numbers
(tune_sem_seg, step/tune_sem_seg.py; not in the reference), the same search over the instance labels' three numbers
(tune_ins_seg, step/tune_ins_seg.py; not in the reference), the search over the IR labels' two thresholds (tune_ir_label,
step/tune_ir_label.py; not in the reference) and the COCO export of the instance labels (make_cocoann,
step/make_cocoann.py; not in the reference's run_sample.py, which leaves it to be run by hand).

The training steps of the reference have commands of their own (train_cam: run_train_cam.py, train_irn: run_train.py);
their `--*_pass` flags are accepted here so existing command lines keep working, and asking for one of them
is an error rather than a silent skip.  Weights are inputs: --cam_weights_name / --irn_weights_name
must point at checkpoints written by those commands or by the reference's training steps (any state dict with the
same keys).
"""
import argparse
import os

from irn_amd.misc import pyutils
from irn_amd.step import _classes


def _flag(v):
    """The reference declares pass flags without type= (a CLI value arrives as str and fails its
    `is True` test); parse the usual spellings instead."""
    if isinstance(v, bool):
        return v
    return str(v).strip().lower() in ("1", "true", "yes", "y")


def _split_gemm(v):
    """--split_gemm: 0 / 1 as the integers they always were, or "auto"."""
    v = str(v).strip().lower()
    if v not in ("0", "1", "auto"):
        raise argparse.ArgumentTypeError("0, 1 or auto, got %r" % v)
    return v if v == "auto" else int(v)


def _ratio(v):
    """--boundary_iou_ratio: a float that is 0 or above (nan is refused)."""
    r = float(v)
    if not r >= 0:
        raise argparse.ArgumentTypeError("--boundary_iou_ratio: 0 (off) or a positive ratio of the image diagonal, got %r" % v)
    return r


def _crf_iters(v):
    """--sem_seg_crf_iters: an integer that is 0 or above."""
    t = int(v)
    if t < 0:
        raise argparse.ArgumentTypeError("--sem_seg_crf_iters: 0 (off) or a number of mean-field iterations, got %r" % v)
    return t


def apply_split_gemm(args, auto=True):
    """--split_gemm into IRN_SPLIT_GEMM (workers read it when they import the trunk) and the trunk's module switches of this
    process; unset: both stay as the environment made them.  `auto` False: a command whose steps have no per-image fallback
    runs "auto" as 1."""
    if args.split_gemm is not None:
        from irn_amd.net import resnet50 as _r50
        _r50.set_split_mode(args.split_gemm if auto or args.split_gemm != "auto" else 1)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--num_workers", default=(os.cpu_count() or 2) // 2, type=int)
    p.add_argument("--voc12_root", required=True, type=str)
    p.add_argument("--train_list", default="voc12/train_aug.txt", type=str)
    p.add_argument("--val_list", default="voc12/val.txt", type=str)
    p.add_argument("--infer_list", default="voc12/train.txt", type=str)
    p.add_argument("--chainer_eval_set", default="train", type=str)
    _classes.add_arguments(p)              # --num_classes, --class_names
    p.add_argument("--cam_network", default="net.resnet50_cam", type=str)
    p.add_argument("--cam_scales", default=(1.0, 0.5, 1.5, 2.0), type=float, nargs="+")
    p.add_argument("--irn_network", default="net.resnet50_irn", type=str)
    p.add_argument("--beta", default=10, type=float)
    p.add_argument("--exp_times", default=8, type=int)
    p.add_argument("--ins_seg_bg_thres", default=0.25, type=float)
    p.add_argument("--sem_seg_bg_thres", default=0.25, type=float)
    p.add_argument("--sem_seg_crf_iters", default=0, type=_crf_iters,
                   help="make_sem_seg_labels, tune_sem_seg: refine the labels by a dense CRF whose unary is the log of the walk's "
                        "scores and of --sem_seg_bg_thres (not in the reference; DESIGN.md §29); mean-field iterations, 0 = off, "
                        "10 is the usual count.  Needs device preprocessing, a threshold of at least 1e-5 and at most 31 classes "
                        "per image; tune_sem_seg then takes at most 16 thresholds")
    p.add_argument("--radius", default=5, type=int,
                   help="random-walk radius of the label steps (not a flag of the reference, which hard-codes 5 at "
                        "step/make_sem_seg_labels.py:41 and step/make_ins_seg_labels.py:135; 10 = BASELINE configs[2])")
    p.add_argument("--conf_fg_thres", default=0.30, type=float, help="cam_to_ir_label: CAM score of a confident foreground seed")
    p.add_argument("--conf_bg_thres", default=0.05, type=float, help="cam_to_ir_label: CAM score below which a seed is background")
    # training / evaluation hyper-parameters of the reference (run_sample.py:25-40): accepted so that an existing
    # command line keeps parsing; the steps that read them are run by run_train_cam.py (cam_*) and run_train.py (irn_*)
    for name, default, typ in (("cam_crop_size", 512, int), ("cam_batch_size", 16, int), ("cam_num_epoches", 5, int),
                               ("cam_learning_rate", 0.1, float), ("cam_weight_decay", 1e-4, float),
                               ("irn_crop_size", 512, int), ("irn_batch_size", 32, int), ("irn_num_epoches", 3, int),
                               ("irn_learning_rate", 0.1, float), ("irn_weight_decay", 1e-4, float)):
        p.add_argument("--" + name, default=default, type=typ, help="read by run_train_cam.py / run_train.py; accepted and ignored here")
    p.add_argument("--cam_eval_thres", default=0.15, type=float,
                   help="eval_cam: background score of the CAM argmax (step/eval_cam.py:15)")
    p.add_argument("--cam_eval_thres_sweep", default=[], type=float, nargs="*",
                   help="eval_cam: more thresholds counted in the same pass (not in the reference; at most 255); prints the "
                        "miou of each and the best one")
    p.add_argument("--boundary_iou_ratio", default=0.0, type=_ratio,
                   help="eval_sem_seg, eval_ins_seg: also score Boundary IoU / Boundary AP (Cheng et al., CVPR 2021; not in the "
                        "reference) on bands of round(R * image diagonal) pixels; 0 = off, the published value is 0.02")
    p.add_argument("--tune_beta", default=[], type=float, nargs="*",
                   help="tune_sem_seg: more values of --beta on the grid (not in the reference)")
    p.add_argument("--tune_exp_times", default=[], type=int, nargs="*",
                   help="tune_sem_seg: more values of --exp_times on the grid; beta x exp_times gives at most 64 walks per image")
    p.add_argument("--tune_bg_thres", default=[], type=float, nargs="*",
                   help="tune_sem_seg: more values of --sem_seg_bg_thres, all counted in one pass per walk (at most 256)")
    p.add_argument("--tune_ins_bg_thres", default=[], type=float, nargs="*",
                   help="tune_ins_seg: more values of --ins_seg_bg_thres on its grid (with --tune_beta / --tune_exp_times; at most "
                        "64: each one is a labelling pass per walk)")
    p.add_argument("--tune_conf_fg_thres", default=[], type=float, nargs="*",
                   help="tune_ir_label: more values of --conf_fg_thres on its grid (not in the reference; at most 16 per axis and "
                        "16 distinct thresholds over both axes: each is one CRF per image)")
    p.add_argument("--tune_conf_bg_thres", default=[], type=float, nargs="*",
                   help="tune_ir_label: more values of --conf_bg_thres on its grid")
    p.add_argument("--worker_devices", default="", type=str,
                   help="device ordinal of every worker process, e.g. 0,1,2,3 (default: one per visible GPU like the reference; "
                        "0,0 = two workers sharing GPU 0)")
    p.add_argument("--cam_batch", default=0, type=int, help="images of one size per CAM trunk pass (0 = 8)")
    p.add_argument("--irn_batch", default=0, type=int, help="images per IRNet trunk pass (0 = 8)")
    p.add_argument("--keep_cams_on_device", default=True, type=_flag,
                   help="hand the CAMs of make_cam to the label steps in device memory when they run in the same process "
                        "(the .npy files are written all the same)")
    p.add_argument("--keep_edges_on_device", default=True, type=_flag,
                   help="the label step that runs first leaves every image's boundary / displacement maps on the device and the "
                        "other one skips its IRNet forward (the reference runs EdgeDisplacement in both steps)")
    p.add_argument("--walk_batch", default=0, type=int,
                   help="images per random-walk launch (not in the reference); 0 = the step's default (64 sem-seg, 32 ins-seg)")
    p.add_argument("--walk_accel", default=None, type=int, choices=(0, 1),
                   help="random-walk schedule (not in the reference): 1 = x.T^(2^exp_times) as a truncated Chebyshev series of the "
                        "operator (84 applications at exp_times 8; the default), 0 = the reference's own 2^exp_times applications "
                        "(misc/indexing.py:136-137).  Unset: the environment variable IRN_WALK_ACCEL, else 1")
    p.add_argument("--walk_accel_tol_exp", default=0, type=int,
                   help="truncation bound 10^-e of the series (0 = the library default, e = 7; 6 = 78 applications: +7 %%, may flip an argmax at an exact tie)")
    p.add_argument("--deterministic", default=None, type=int, choices=(0, 1),
                   help="1 (the default) = bit-reproducible backbones: any worker layout writes identical files (tuned shapes on a "
                        "find database without split-K solvers, MIOpen's deterministic attribute elsewhere); 0 = the last 2-4 %% of "
                        "speed, outputs then move by ~1e-5 from run to run (not in the reference).  Unset: the environment "
                        "variable IRN_DETERMINISTIC, else 1")
    p.add_argument("--split_gemm", default=None, type=_split_gemm, choices=(0, 1, "auto"),
                   help="1 (default): the trunk's 1x1 convolutions as fp16 hi/lo split products with fp32 accumulation (fp32-level "
                        "accuracy, ~15 %% faster end to end); a step raises at its end if an activation left fp16's range.  0: plain "
                        "fp32 GEMMs.  auto: as 1, but make_cam, make_sem_seg and make_ins_seg notice such an activation per image, "
                        "write nothing computed from it and compute that image again on the fp32 GEMMs (its files are those of 0, "
                        "all others those of 1; one line per worker names the images).  The tune_* steps, run_train.py and "
                        "run_train_cam.py keep the end-of-step check: auto behaves as 1 there.  (also IRN_SPLIT_GEMM)")
    p.add_argument("--step_timeout", default=0.0, type=float,
                   help="seconds a step may take in its worker processes before the pool is stopped and the step raises "
                        "(0 = no limit; also IRN_STEP_TIMEOUT_S)")
    p.add_argument("--log_name", default="sample_train_eval", type=str)
    p.add_argument("--cam_weights_name", default="sess/res50_cam.pth", type=str)
    p.add_argument("--irn_weights_name", default="sess/res50_irn.pth", type=str)
    p.add_argument("--cam_out_dir", default="result/cam", type=str)
    p.add_argument("--ir_label_out_dir", default="result/ir_label", type=str)
    p.add_argument("--sem_seg_out_dir", default="result/sem_seg", type=str)
    p.add_argument("--ins_seg_out_dir", default="result/ins_seg", type=str)
    p.add_argument("--ins_seg_format", default="npy", choices=("npy", "rle"),
                   help="make_ins_seg_labels: npy = the reference's <name>.npy with dense masks; rle (not in the reference) = "
                        "<name>.rle.npz with every mask as its COCO run lengths, encoded on the GPU — make_cocoann and "
                        "eval_ins_seg read either")
    p.add_argument("--cocoann_out", default="voc2012_train_custom.json", type=str,
                   help="make_cocoann: the COCO annotation file it writes (the reference hard-codes this name, step/make_cocoann.py:48)")
    p.add_argument("--cocoann_segmentation", default="rle", choices=("rle", "polygon"),
                   help="make_cocoann: rle = every mask as COCO's compressed run lengths; polygon = as the polygons of its "
                        "outer boundary along pixel edges, integer corners, traced on the GPU (the reference writes skimage "
                        "contours; irn_amd/step/make_cocoann.py says how these differ)")
    p.add_argument("--edge_out_dir", default=None, type=str,
                   help="verification aid (not in the reference): also write every image's boundary / displacement maps "
                        "(<name>.npy = {'edge' [1,h,w], 'dp' [2,h,w]}) as the label steps used them")
    for name, default in (("train_cam_pass", False), ("make_cam_pass", True), ("eval_cam_pass", False),
                          ("cam_to_ir_label_pass", False), ("train_irn_pass", False), ("make_ins_seg_pass", True),
                          ("eval_ins_seg_pass", False), ("make_cocoann_pass", False), ("make_sem_seg_pass", True),
                          ("eval_sem_seg_pass", False), ("tune_sem_seg_pass", False), ("tune_ins_seg_pass", False),
                          ("tune_ir_label_pass", False)):
        p.add_argument("--" + name, default=default, type=_flag)
    return p


OUT_OF_SCOPE = ("train_cam_pass", "train_irn_pass")


def main(argv=None):
    """Runs the requested passes in the reference's order; returns {step name: printed dict} of the evaluation passes."""
    args = build_parser().parse_args(argv)
    for name in OUT_OF_SCOPE:
        if getattr(args, name):
            raise SystemExit("--train_irn_pass: IRNet training is run by `python run_train.py --train_irn_pass True`, not from here"
                             if name == "train_irn_pass" else
                             "--%s: CAM training is run by `python run_train_cam.py`, not from here" % name)
    if args.class_names:
        _classes.class_names(args)           # a missing file or a wrong line count, before any step has run
    for d in (args.cam_out_dir, args.sem_seg_out_dir, args.ins_seg_out_dir) + ((args.ir_label_out_dir,) if args.cam_to_ir_label_pass else ()):
        os.makedirs(d, exist_ok=True)
    apply_split_gemm(args)
    if args.deterministic is not None:
        os.environ["IRN_DETERMINISTIC"] = str(int(args.deterministic))      # read by every process that sets MIOpen up (workers inherit it)
    pyutils.Logger(args.log_name + ".log")
    print(vars(args))
    results = {}
    if args.make_cam_pass is True:
        from irn_amd.step import make_cam
        timer = pyutils.Timer("step.make_cam:")
        make_cam.run(args)
    if args.eval_cam_pass is True:
        from irn_amd.step import eval_cam
        timer = pyutils.Timer("step.eval_cam:")
        results["eval_cam"] = eval_cam.run(args)
    if args.cam_to_ir_label_pass is True:
        from irn_amd.step import cam_to_ir_label
        timer = pyutils.Timer("step.cam_to_ir_label:")
        cam_to_ir_label.run(args)
    if args.make_ins_seg_pass is True:
        from irn_amd.step import make_ins_seg_labels
        timer = pyutils.Timer("step.make_ins_seg_labels:")
        make_ins_seg_labels.run(args)
    if args.eval_ins_seg_pass is True:
        from irn_amd.step import eval_ins_seg
        timer = pyutils.Timer("step.eval_ins_seg:")
        results["eval_ins_seg"] = eval_ins_seg.run(args)
    if args.make_cocoann_pass is True:
        from irn_amd.step import make_cocoann
        timer = pyutils.Timer("step.make_cocoann:")
        results["make_cocoann"] = make_cocoann.run(args)
    if args.make_sem_seg_pass is True:
        from irn_amd.step import make_sem_seg_labels
        timer = pyutils.Timer("step.make_sem_seg_labels:")
        make_sem_seg_labels.run(args)
    if args.eval_sem_seg_pass is True:
        from irn_amd.step import eval_sem_seg
        timer = pyutils.Timer("step.eval_sem_seg:")  # noqa: F841
        results["eval_sem_seg"] = eval_sem_seg.run(args)
    if args.tune_sem_seg_pass is True:
        from irn_amd.step import tune_sem_seg
        timer = pyutils.Timer("step.tune_sem_seg:")  # noqa: F841
        results["tune_sem_seg"] = tune_sem_seg.run(args)
    if args.tune_ins_seg_pass is True:
        from irn_amd.step import tune_ins_seg
        timer = pyutils.Timer("step.tune_ins_seg:")  # noqa: F841
        results["tune_ins_seg"] = tune_ins_seg.run(args)
    if args.tune_ir_label_pass is True:
        from irn_amd.step import tune_ir_label
        timer = pyutils.Timer("step.tune_ir_label:")  # noqa: F841
        results["tune_ir_label"] = tune_ir_label.run(args)
    from irn_amd.step import _common
    _common.shutdown_workers()           # the per-GPU workers served every pass above
    return results                       # what the evaluation passes printed, by step name


if __name__ == "__main__":
    main()
