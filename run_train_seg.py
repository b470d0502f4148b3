#!/usr/bin/env python3
"""Entry point of the step the pseudo-labels are made for: training a segmentation network on `result/sem_seg/*.png`
(`train_sem_seg`, irn_amd/step/train_sem_seg.py), predicting with it (`infer_sem_seg`) and scoring the predictions
(`eval_sem_seg` on --seg_pred_dir):

    python run_train_seg.py --voc12_root VOC2012 --seg_init_weights resnet50_imagenet.pth
    python run_train_seg.py --voc12_root VOC2012 --train_sem_seg_pass False --infer_sem_seg_pass True --eval_seg_pass True \\
        --infer_list voc12/val.txt --chainer_eval_set val

The flags are run_train.py's (--train_list, --infer_list, --chainer_eval_set, --sem_seg_out_dir, --num_classes, --seed,
--deterministic, ...) plus the `seg_*` ones below.  The pass flags of the other commands are parsed and ignored here;
run_sample.py, run_train.py and run_train_cam.py are unchanged.
"""
import copy

import run_sample
import run_train
from irn_amd.misc import pyutils


def build_parser():
    p = run_train.build_parser()
    p.add_argument("--train_sem_seg_pass", default=True, type=run_sample._flag)
    p.add_argument("--infer_sem_seg_pass", default=False, type=run_sample._flag)
    p.add_argument("--eval_seg_pass", default=False, type=run_sample._flag,
                   help="eval_sem_seg on the predictions in --seg_pred_dir (against --chainer_eval_set)")
    p.add_argument("--seg_label_dir", default=None, type=str,
                   help="directory of the training label PNGs (0 = background, class + 1 otherwise, anything above "
                        "--num_classes ignored); unset: --sem_seg_out_dir, where make_sem_seg_labels writes")
    p.add_argument("--seg_crop_size", default=512, type=int, help="side of the training crop, a multiple of 16")
    p.add_argument("--seg_batch_size", default=16, type=int)
    p.add_argument("--seg_num_epoches", default=30, type=int,
                   help="passes over --train_list (default 30: about 20 000 steps of 16 on train_aug, DeepLab-v2's schedule)")
    p.add_argument("--seg_learning_rate", default=2.5e-4, type=float,
                   help="rate of the backbone, the head trains at ten times it; poly schedule (default 2.5e-4, DeepLab-v2's)")
    p.add_argument("--seg_weight_decay", default=5e-4, type=float, help="default 5e-4, DeepLab-v2's")
    p.add_argument("--seg_rescale", default=(0.5, 1.5), type=float, nargs=2, metavar=("MIN", "MAX"),
                   help="range of the random factor image and label are rescaled by before the crop")
    p.add_argument("--seg_weights_name", default="sess/res50_seg", type=str, help="the step writes this name + '.pth'")
    p.add_argument("--seg_init_weights", default=None, type=str,
                   help="state dict the network starts from, loaded non-strictly: a bare ResNet-50 trunk (conv1.weight, "
                        "layer1.0...; the ImageNet one), a net.resnet50_cam.Net checkpoint (its classifier is dropped) or an "
                        "earlier file of this step; unset: seeded random weights.  Nothing is downloaded")
    p.add_argument("--seg_augment", default="device", choices=("device", "host"),
                   help="device: the loader hands over bytes, the label map and the draws, the (image, label) batch is rescaled / "
                        "mirrored / cropped on the GPU (bit-identical); host: the PIL / numpy pipeline in the loader workers")
    p.add_argument("--seg_loss", default="fused", choices=("fused", "composed"),
                   help="fused: upsampling + softmax cross-entropy and its backward in one HIP pass each (ops.seg_cross_entropy), "
                        "bit-reproducible, no [B,C,crop,crop] tensor; composed: F.interpolate -> F.cross_entropy, for "
                        "comparison (three such tensors, float atomics in the backward: not reproducible)")
    p.add_argument("--seg_pred_dir", default="result/seg_pred", type=str,
                   help="where infer_sem_seg writes its PNGs and --eval_seg_pass reads them")
    p.add_argument("--seg_infer_scales", default=[1.0], type=float, nargs="+", metavar="S",
                   help="infer_sem_seg: 1..16 factors in (0, 4] the image is rescaled by (bicubic); the softmax of every scale's "
                        "logits, upsampled to the image's size, is averaged in one HIP launch (ops.seg_fuse).  Default 1.0 alone: "
                        "the single-scale arg-max (ops.seg_argmax)")
    p.add_argument("--seg_crf_iters", default=0, type=int,
                   help="infer_sem_seg: mean-field iterations of a dense CRF seeded with the averaged probabilities "
                        "(ops.crf_prob); 0 = off (default); needs --num_classes <= 31")
    return p


def main(argv=None):
    """Runs train_sem_seg, infer_sem_seg and eval_sem_seg where their pass flags ask for them; returns {step name: what the
    step returned}."""
    args = build_parser().parse_args(argv)
    args.seg_rescale = tuple(args.seg_rescale)
    run_train.start(args)
    results = {}
    if args.train_sem_seg_pass is True:
        from irn_amd.step import train_sem_seg
        timer = pyutils.Timer("step.train_sem_seg:")
        results["train_sem_seg"] = train_sem_seg.run(args)
    if args.infer_sem_seg_pass is True:
        from irn_amd.step import infer_sem_seg
        timer = pyutils.Timer("step.infer_sem_seg:")
        results["infer_sem_seg"] = infer_sem_seg.run(args)
    if args.eval_seg_pass is True:
        from irn_amd.step import eval_sem_seg
        timer = pyutils.Timer("step.eval_sem_seg:")  # noqa: F841
        scored = copy.copy(args)
        scored.sem_seg_out_dir = args.seg_pred_dir
        results["eval_sem_seg"] = eval_sem_seg.run(scored)
    return results


if __name__ == "__main__":
    main()
