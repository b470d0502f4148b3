"""CAM classifier training (reference step/train_cam.py), single GPU, single process.

Reads  args.train_list, args.val_list, args.voc12_root (cls_labels.npy beside the lists), args.cam_crop_size,
       args.cam_batch_size, args.cam_num_epoches, args.cam_learning_rate, args.cam_weight_decay, args.num_workers,
       args.seed, args.cam_init_weights, args.cam_resize_long, args.cam_augment, args.cam_fused_tail
Writes args.cam_weights_name + '.pth' (the reference appends the suffix, step/train_cam.py:100, and make_cam reads the file
       under that name): the state dict of net.resnet50_cam.Net, which loads into CAM with strict=True

The reference's loop (the shared one, irn_amd/step/_train.py) with three differences.  The input batch is built on the GPU
(`--cam_augment device`, the default): the loader workers hand over the decoded bytes and the augmentation's draws, and
`ops.augment_batch` resizes, normalises, mirrors, crops and pads the whole batch in two launches (irn_amd/csrc/augment.hip),
bit for bit what the reference's PIL / numpy pipeline gives for the same draws — `--cam_augment host` runs that pipeline in
the workers instead.  Stages 1-2 of the trunk, which the reference detaches, run under `no_grad` (`Net.forward_train`).  And
there is no nn.DataParallel: one device.  In the reproducible mode (IRN_DETERMINISTIC, default 1) the step sets the process's
mode before its first convolution like train_irn, and two runs write the same file.
With `--cam_fused_tail 1` (default 0) the elementwise tail of every unit of the trained half — batch norm, residual add, ReLU
and their backward — is one differentiable HIP pass each way (`ops.bn_act`, irn_amd/csrc/bn_act.hip) instead of ATen's
composed kernels; reproducible like the default, other bits (one rounding per layer differs).
Initial weights: `--cam_init_weights` (a state dict loaded non-strictly: a bare ResNet-50 trunk such as the ImageNet one, or
a full `Net` state), else the seeded random state of net.weights; nothing is downloaded.
"""
import torch
import torch.nn.functional as F

from .. import _tuned
from ..net import weights
from ..net.resnet50_cam import Net
from ..voc12 import dataloader
from . import _classes, _train
from ._train import MAX_LOADER_WORKERS  # noqa: F401

PRINT_EVERY = 100


def build_model(args):
    c = _classes.num_classes(args)
    model = Net(n_classes=c)
    init = getattr(args, "cam_init_weights", None)
    model.load_state_dict(_train.init_state(init) if init else weights.random_cam_state(n_classes=c), strict=False)
    return model


def device_augment(args):
    return getattr(args, "cam_augment", "device") != "host"


def make_datasets(args, seed):
    """(train, val) datasets as step/train_cam.py:44-52 configures them; raw items when the batch is built on the GPU."""
    raw = device_augment(args)
    c = _classes.num_classes(args)
    train = dataloader.VOC12ClassificationDataset(args.train_list, voc12_root=args.voc12_root,
                                                  resize_long=tuple(getattr(args, "cam_resize_long", (320, 640))), hor_flip=True,
                                                  crop_size=args.cam_crop_size, crop_method="random", raw=raw, seed=seed,
                                                  n_classes=c)
    val = dataloader.VOC12ClassificationDataset(args.val_list, voc12_root=args.voc12_root, crop_size=args.cam_crop_size,
                                                raw=raw, seed=seed, n_classes=c)
    return train, val


def train_step(model, optimizer, img, label):
    """One optimisation step on a batch already on the device; returns the loss as a device scalar."""
    loss = F.multilabel_soft_margin_loss(model.forward_train(img), label)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach()


def validate(model, loader, crop, device):
    """Mean multilabel soft-margin loss over the batches of `loader` (step/train_cam.py:14-36), one read-back."""
    print("validating ... ", flush=True, end="")
    model.eval()
    losses = []
    with torch.no_grad():
        for pack in loader:
            x = model(_train.device_images(pack, crop, device))
            losses.append(F.multilabel_soft_margin_loss(x, pack["label"].to(device, non_blocking=True)))
    model.train()
    loss = float(torch.stack(losses).mean()) if losses else float("nan")
    print("loss: %.4f" % loss)
    return loss


def run(args):
    """Returns {'first_loss': float, 'steps': int, 'val_losses': [one per epoch]}."""
    # the mode only (MIOpen stays as the caller has it), before the model is built or a convolution runs
    with _tuned.process_mode(fused_tail=int(getattr(args, "cam_fused_tail", 0) or 0)):
        return _run(args)


def _run(args):
    device = torch.device("cuda", torch.cuda.current_device())
    seed = int(getattr(args, "seed", 0))
    torch.manual_seed(seed)
    model = build_model(args)
    crop, batch = args.cam_crop_size, args.cam_batch_size

    train_dataset, val_dataset = make_datasets(args, seed)
    max_step = _train.max_steps("train_cam", "train_list", train_dataset, batch, args.cam_num_epoches)
    _train.max_steps("train_cam", "val_list", val_dataset, batch, 1)
    optimizer = _train.two_rate_optimizer(*model.trainable_parameters(), args.cam_learning_rate, args.cam_weight_decay, max_step)

    def make_loader(dataset, shuffle, seed):
        return _train.loader(dataset, batch, args.num_workers, shuffle, seed, dataloader.classification_collate)

    def step(pack):
        img = _train.device_images(pack, crop, device)
        return train_step(model, optimizer, img, pack["label"].to(device, non_blocking=True))

    val_losses = []
    first = _train.fit(model, optimizer, train_dataset, lambda s: make_loader(train_dataset, True, s), device, args.cam_num_epoches,
                       batch, seed, PRINT_EVERY, step, "loss:%.4f",
                       after_epoch=lambda ep: val_losses.append(validate(model, make_loader(val_dataset, False, seed), crop, device)))
    _train.save_state(model, args.cam_weights_name + ".pth")
    return {"first_loss": float(first), "steps": optimizer.global_step, "val_losses": val_losses}
