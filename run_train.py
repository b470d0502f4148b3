#!/usr/bin/env python3
"""Entry point of the training side: `train_irn` (irn_amd/step/train_irn.py), with `cam_to_ir_label` in front of it when
asked for, so that labels and weights come out of one command:

    python run_train.py --voc12_root VOC2012 --cam_to_ir_label_pass True --train_irn_pass True

The flags are run_sample.py's (the `irn_*` hyper-parameters that run_sample.py accepts and ignores are read here) plus
--seed, --irn_init_weights, --irn_augment and --irn_trunk.  run_sample.py itself keeps refusing the training passes; `--train_cam_pass` is refused
here as well: CAM training has a command of its own, `python run_train_cam.py` (irn_amd/step/train_cam.py).
"""
import os

import run_sample
from irn_amd.misc import pyutils


def build_parser():
    p = run_sample.build_parser()
    p.add_argument("--seed", default=0, type=int, help="fixes the shuffle, the augmentations and the random initial weights")
    p.add_argument("--irn_init_weights", default=None, type=str,
                   help="state dict the IRNet starts from, loaded non-strictly (an ImageNet ResNet-50 trunk, an earlier "
                        "checkpoint); unset: seeded random weights.  Nothing is downloaded")
    p.add_argument("--irn_augment", default="device", choices=("device", "host"),
                   help="device: the loader hands over bytes, the IR label map and the draws, the (image, label) batch is "
                        "rescaled / mirrored / cropped on the GPU (bit-identical); host: the PIL / numpy pipeline in the "
                        "loader workers")
    p.add_argument("--irn_trunk", default="autograd", choices=("autograd", "inference"),
                   help="autograd: the frozen trunk of a training step runs inside the autograd graph (NCHW, composed ops, fp32 "
                        "MIOpen convolutions); inference: under no_grad on the label steps' path — fused tails, and for a crop the "
                        "shipped MIOpen database is tuned for (512) the channels-last split-GEMM pass in rows of 16.  In the "
                        "reproducible mode any OTHER crop runs the trunk in NCHW passes of 2 rows, which can be slower than "
                        "autograd.  Same gradients up to rounding, other bits")
    return p


def start(args):
    """The preamble of the three training commands: the process's mode from --deterministic, the log file, the flags."""
    if args.deterministic is not None:
        os.environ["IRN_DETERMINISTIC"] = str(int(args.deterministic))
    pyutils.Logger(args.log_name + ".log")
    print(vars(args))


def main(argv=None):
    """Runs cam_to_ir_label and train_irn where their pass flags ask for them; returns {step name: what the step returned}."""
    args = build_parser().parse_args(argv)
    if args.train_cam_pass:
        raise SystemExit("--train_cam_pass: CAM training is run by `python run_train_cam.py`, not from here")
    run_sample.apply_split_gemm(args, auto=False)       # training keeps the end-of-step fp16-range check: "auto" runs as 1
    start(args)
    results = {}
    if args.cam_to_ir_label_pass is True:
        from irn_amd.step import _common, cam_to_ir_label
        timer = pyutils.Timer("step.cam_to_ir_label:")
        cam_to_ir_label.run(args)
        _common.shutdown_workers()
    if args.train_irn_pass is True:
        from irn_amd.step import train_irn
        timer = pyutils.Timer("step.train_irn:")  # noqa: F841
        results["train_irn"] = train_irn.run(args)
    return results


if __name__ == "__main__":
    main()
