"""CAM classifier training (reference step/train_cam.py), single GPU, single process.

Reads  args.train_list, args.val_list, args.voc12_root (cls_labels.npy beside the lists), args.cam_crop_size,
       args.cam_batch_size, args.cam_num_epoches, args.cam_learning_rate, args.cam_weight_decay, args.num_workers,
       args.seed, args.cam_init_weights, args.cam_resize_long, args.cam_augment, args.cam_fused_tail
Writes args.cam_weights_name + '.pth' (the reference appends the suffix, step/train_cam.py:100, and make_cam reads the file
       under that name): the state dict of net.resnet50_cam.Net, which loads into CAM with strict=True

The reference's loop with three differences.  The input batch is built on the GPU (`--cam_augment device`, the default):
the loader workers hand over the decoded bytes and the augmentation's draws, and `ops.augment_batch` resizes, normalises,
mirrors, crops and pads the whole batch in two launches (irn_amd/csrc/augment.hip), bit for bit what the reference's
PIL / numpy pipeline gives for the same draws — `--cam_augment host` runs that pipeline in the workers instead.  Stages 1-2
of the trunk, which the reference detaches, run under `no_grad` (`Net.forward_train`).  And there is no nn.DataParallel:
one device.  The draws of an item come from (seed, epoch, index) and the shuffle from seed + epoch, so a run is fixed by
its seed whatever the number of loader workers; in the reproducible mode (IRN_DETERMINISTIC, default 1) the step sets the
process's mode before its first convolution like train_irn, and two runs write the same file.  Initial weights:
With `--cam_fused_tail 1` (default 0) the elementwise tail of every unit of the trained half — batch norm, residual add, ReLU
and their backward — is one differentiable HIP pass each way (`ops.bn_act`, irn_amd/csrc/bn_act.hip) instead of ATen's
composed kernels; reproducible like the default, other bits (one rounding per layer differs).
`--cam_init_weights` (a state dict loaded non-strictly: a bare ResNet-50 trunk such as the ImageNet one, or a full `Net`
state), else the seeded random state of net.weights; nothing is downloaded.
"""
import os

import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

from .. import _tuned
from ..misc import pyutils, torchutils
from ..net import weights
from ..net.resnet50_cam import Net
from ..voc12 import dataloader
from . import _classes

MAX_LOADER_WORKERS = 8
PRINT_EVERY = 100


def build_model(args):
    c = _classes.num_classes(args)
    model = Net(n_classes=c)
    init = getattr(args, "cam_init_weights", None)
    if init:
        state = torch.load(init, map_location="cpu", weights_only=True)
        if "conv1.weight" in state:          # a bare trunk: its keys are the `resnet50.` ones (the stages alias them)
            state = {"resnet50." + k: v for k, v in state.items() if not k.startswith("fc.")}
    else:
        state = weights.random_cam_state(n_classes=c)
    model.load_state_dict(state, strict=False)
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


def _loader(dataset, args, shuffle, seed):
    gen = torch.Generator().manual_seed(seed)
    return DataLoader(dataset, batch_size=args.cam_batch_size, shuffle=shuffle, drop_last=True, pin_memory=not dataset.raw,
                      num_workers=max(0, min(int(args.num_workers), MAX_LOADER_WORKERS)), generator=gen,
                      collate_fn=dataloader.classification_collate)


def device_batch(pack, crop, device):
    """Loader batch -> GPU fp32 [B,3,crop,crop]: raw items through `ops.augment_batch`, the reference's floats as they are."""
    if "aug" in pack:
        from .. import ops
        return ops.augment_batch(pack["img"], pack["aug"], crop, device=device)
    return pack["img"].to(device, non_blocking=True)


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
            x = model(device_batch(pack, crop, device))
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
    crop = args.cam_crop_size

    train_dataset, val_dataset = make_datasets(args, seed)
    max_step = (len(train_dataset) // args.cam_batch_size) * args.cam_num_epoches
    if max_step == 0:
        raise RuntimeError("train_cam: train_list holds fewer images than one batch of %d" % args.cam_batch_size)
    if len(val_dataset) < args.cam_batch_size:
        raise RuntimeError("train_cam: val_list holds fewer images than one batch of %d" % args.cam_batch_size)

    backbone_params, new_params = model.trainable_parameters()
    optimizer = torchutils.PolyOptimizer([
        {"params": backbone_params, "lr": args.cam_learning_rate, "weight_decay": args.cam_weight_decay},
        {"params": new_params, "lr": 10 * args.cam_learning_rate, "weight_decay": args.cam_weight_decay},
    ], lr=args.cam_learning_rate, weight_decay=args.cam_weight_decay, max_step=max_step)

    model = model.to(device)
    model.train()
    timer = pyutils.Timer()
    first, pending, val_losses = None, [], []
    for ep in range(args.cam_num_epoches):
        print("Epoch %d/%d" % (ep + 1, args.cam_num_epoches))
        train_dataset.set_epoch(ep)
        for it, pack in enumerate(_loader(train_dataset, args, True, seed + ep)):
            img = device_batch(pack, crop, device)
            label = pack["label"].to(device, non_blocking=True)
            pending.append(train_step(model, optimizer, img, label))
            if first is None:
                first = float(pending[0])
            if (optimizer.global_step - 1) % PRINT_EVERY == 0:
                timer.update_progress(optimizer.global_step / max_step)
                mean = float(torch.stack(pending).mean())          # the one read-back per 100 steps
                pending = []
                print("step:%5d/%5d" % (optimizer.global_step - 1, max_step),
                      "loss:%.4f" % mean,
                      "imps:%.1f" % ((it + 1) * args.cam_batch_size / timer.get_stage_elapsed()),
                      "lr: %.4f" % (optimizer.param_groups[0]["lr"]),
                      "etc:%s" % (timer.str_estimated_complete()), flush=True)
        val_losses.append(validate(model, _loader(val_dataset, args, False, seed), crop, device))
        timer.reset_stage()

    out = args.cam_weights_name + ".pth"
    out_dir = os.path.dirname(out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    torch.save(model.to("cpu").state_dict(), out)      # (on the host: the aliased entries stay one storage)
    torch.cuda.empty_cache()
    return {"first_loss": first, "steps": optimizer.global_step, "val_losses": val_losses}
