"""Segmentation training on the pseudo-labels (not in the reference, which hands `result/sem_seg` to an external DeepLab),
single GPU, single process.

Reads  args.train_list, args.voc12_root, args.seg_label_dir (default args.sem_seg_out_dir: the PNGs of make_sem_seg_labels,
       0 = background, class + 1 otherwise), args.seg_crop_size, args.seg_batch_size, args.seg_num_epoches,
       args.seg_learning_rate, args.seg_weight_decay, args.seg_rescale, args.num_workers, args.seed, args.seg_init_weights,
       args.seg_augment, args.seg_loss, args.num_classes
Writes args.seg_weights_name + '.pth': the state dict of net.resnet50_seg.Net, which infer_sem_seg loads

The shared loop (irn_amd/step/_train.py) on its own network and loss.  The (image, label) batch is built on the GPU
(`--seg_augment device`, the default): the loader workers hand over the decoded image, the label map and the augmentation's
draws, and `ops.augment_pair_batch(..., reduce=1)` rescales, normalises, mirrors and crops both (irn_amd/csrc/augment.hip),
bit for bit what the PIL / numpy pipeline gives for the same draws — `--seg_augment host` runs that pipeline in the workers
instead.  The loss is `ops.seg_cross_entropy(model.forward_train(img), label, 16)`: bilinear upsampling of the stride-16
logits, softmax cross-entropy over the pixels whose label is a class of the dataset (255, the crop's fill, and any byte above
--num_classes are ignored) and its backward in one HIP pass each (irn_amd/csrc/seg_loss.hip): no [B, C, crop, crop] tensor
exists and no float atomic takes part in a gradient.  `--seg_loss composed` is F.interpolate ->
F.cross_entropy(ignore_index=255), for comparison: three such tensors, and ATen's scattering upsample backward, so not
reproducible.  In the reproducible mode (IRN_DETERMINISTIC, default 1) two runs write the same file whatever the number of
loader workers.  Initial weights: `--seg_init_weights` (a state dict loaded non-strictly: a bare ResNet-50 trunk such as the
ImageNet one, a CAM checkpoint, or an earlier file of this step), else the seeded random state of net.weights; nothing is
downloaded.
"""
import torch
import torch.nn.functional as F

from .. import _tuned
from ..net import weights
from ..net.resnet50_seg import OUTPUT_STRIDE, Net
from ..voc12 import dataloader
from . import _classes, _train

PRINT_EVERY = 50


def build_model(args):
    c = _classes.num_classes(args)
    model = Net(n_classes=c)
    init = getattr(args, "seg_init_weights", None)
    # (`classifier.`: a CAM checkpoint's read-out)
    state = _train.init_state(init, drop=("classifier.",)) if init else weights.random_seg_state(n_classes=c)
    model.load_state_dict(state, strict=False)
    return model


def device_augment(args):
    return getattr(args, "seg_augment", "device") != "host"


def label_dir(args):
    return getattr(args, "seg_label_dir", None) or args.sem_seg_out_dir


def make_dataset(args, seed):
    return dataloader.VOC12AffinityDataset(args.train_list, label_dir=label_dir(args), voc12_root=args.voc12_root,
                                           hor_flip=True, crop_size=args.seg_crop_size, crop_method="random",
                                           rescale=tuple(getattr(args, "seg_rescale", (0.5, 1.5))), seed=seed,
                                           raw=device_augment(args), reduce=1)


def composed_loss(logits, label, factor):
    """F.interpolate -> F.cross_entropy(ignore_index=255) on labels with every byte >= C mapped to 255: the function
    `ops.seg_cross_entropy` computes, from ATen's kernels."""
    c = logits.shape[1]
    lab = label.long()
    lab = torch.where(lab >= c, torch.full_like(lab, 255), lab)
    z = F.interpolate(logits, scale_factor=factor, mode="bilinear", align_corners=False)[..., :lab.shape[1], :lab.shape[2]]
    return F.cross_entropy(z, lab, ignore_index=255, reduction="sum") / (lab != 255).sum().clamp(min=1)


def seg_loss(args):
    kind = getattr(args, "seg_loss", "fused") or "fused"
    if kind not in ("fused", "composed"):
        raise ValueError("train_sem_seg: seg_loss is 'fused' or 'composed', got %r" % (kind,))
    return kind


def train_step(model, optimizer, img, label, kind="fused"):
    """One optimisation step on a batch already on the device; returns the loss as a device scalar."""
    logits = model.forward_train(img)
    if kind == "fused":
        from .. import ops
        loss = ops.seg_cross_entropy(logits, label, OUTPUT_STRIDE)
    else:
        loss = composed_loss(logits, label, OUTPUT_STRIDE)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach().double()


def run(args):
    """Returns {'first_loss': float, 'steps': int}."""
    # the mode only (MIOpen stays as the caller has it), before the model is built or a convolution runs
    with _tuned.process_mode():
        return _run(args)


def _run(args):
    device = torch.device("cuda", torch.cuda.current_device())
    seed = int(getattr(args, "seed", 0))
    torch.manual_seed(seed)
    crop, batch = int(args.seg_crop_size), args.seg_batch_size
    if crop % OUTPUT_STRIDE:
        raise ValueError("train_sem_seg: --seg_crop_size %d is no multiple of %d" % (crop, OUTPUT_STRIDE))
    kind = seg_loss(args)
    model = build_model(args)

    train_dataset = make_dataset(args, seed)
    max_step = _train.max_steps("train_sem_seg", "train_list", train_dataset, batch, args.seg_num_epoches)
    optimizer = _train.two_rate_optimizer(*model.trainable_parameters(), args.seg_learning_rate, args.seg_weight_decay, max_step)

    def make_loader(seed):
        return _train.loader(train_dataset, batch, args.num_workers, True, seed, dataloader.affinity_collate)

    def step(pack):
        img, label = _train.device_pair(pack, crop, device, reduce=1)
        return train_step(model, optimizer, img, label, kind)

    first = _train.fit(model, optimizer, train_dataset, make_loader, device, args.seg_num_epoches, batch, seed, PRINT_EVERY, step,
                       "loss:%.4f")
    _train.save_state(model, args.seg_weights_name + ".pth")
    return {"first_loss": float(first), "steps": optimizer.global_step}
