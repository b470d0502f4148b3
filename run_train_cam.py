#!/usr/bin/env python3
"""Entry point of CAM classifier training: `train_cam` (irn_amd/step/train_cam.py), the step that writes the checkpoint
every other step starts from:

    python run_train_cam.py --voc12_root VOC2012 --cam_init_weights resnet50_imagenet.pth
    python run_sample.py --voc12_root VOC2012            # make_cam reads the file written above

The flags are run_train.py's (the `cam_*` hyper-parameters, --train_list, --val_list, --cam_weights_name, --seed,
--deterministic) plus --cam_init_weights, --cam_resize_long, --cam_augment and --cam_fused_tail.  The step has a command of its own because
run_sample.py and run_train.py keep refusing `--train_cam_pass True`; the pass flags are parsed and ignored here.
"""
import run_train
from irn_amd.misc import pyutils


def build_parser():
    p = run_train.build_parser()
    p.add_argument("--cam_init_weights", default=None, type=str,
                   help="state dict the classifier starts from, loaded non-strictly: a bare ResNet-50 trunk (conv1.weight, "
                        "layer1.0...; the ImageNet one) or a full net.resnet50_cam.Net state; unset: seeded random weights.  "
                        "Nothing is downloaded")
    p.add_argument("--cam_resize_long", default=(320, 640), type=int, nargs=2, metavar=("MIN", "MAX"),
                   help="range the long side of a training image is resized to, both ends included (step/train_cam.py:45)")
    p.add_argument("--cam_augment", default="device", choices=("device", "host"),
                   help="device: the loader hands over bytes and draws, the batch is resized / mirrored / cropped on the GPU "
                        "(bit-identical); host: the reference's PIL / numpy pipeline in the loader workers")
    p.add_argument("--cam_fused_tail", default=0, type=int, choices=(0, 1),
                   help="1: batch norm + residual + ReLU of the trained stages as one differentiable HIP pass forward and one "
                        "backward (ops.bn_act) instead of the composed autograd ops; reproducible either way, the bits differ")
    return p


def main(argv=None):
    """Runs train_cam; returns {"train_cam": what the step returned}."""
    args = build_parser().parse_args(argv)
    args.cam_resize_long = tuple(args.cam_resize_long)
    run_train.start(args)
    from irn_amd.step import train_cam
    timer = pyutils.Timer("step.train_cam:")  # noqa: F841
    return {"train_cam": train_cam.run(args)}


if __name__ == "__main__":
    main()
