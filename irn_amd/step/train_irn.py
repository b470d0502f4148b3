"""IRNet training (reference step/train_irn.py), single GPU, single process.

Reads  args.train_list, args.infer_list, args.voc12_root, args.ir_label_out_dir (the PNGs of cam_to_ir_label),
       args.irn_crop_size, args.irn_batch_size, args.irn_num_epoches, args.irn_learning_rate, args.irn_weight_decay,
       args.num_workers, args.seed, args.irn_init_weights, args.irn_augment, args.irn_trunk
Writes args.irn_weights_name: the state dict the label steps load (EdgeDisplacement through net.weights.load_checkpoint)

The reference's loop with three differences.  The input batch is built on the GPU (`--irn_augment device`, the default):
the loader workers hand over the decoded image, the IR label map and the augmentation's draws, and `ops.augment_pair_batch`
rescales, normalises, mirrors and crops the images and gathers the reduced label maps for the whole batch
(irn_amd/csrc/augment.hip), bit for bit what the PIL / numpy pipeline gives for the same draws — `--irn_augment host` runs
that pipeline in the workers instead.  The displacement-mean pass follows the same choice.
The loss is `AffinityDisplacementLoss.fused_losses`: one HIP pass from the boundary, displacement and reduced label maps to
the five sums (irn_amd/csrc/aff_loss.hip), so the loader sends one uint8 map per image instead of three [|S|, N] float
tensors and no [B, |S|, N] tensor exists on the device.  And there is no nn.DataParallel: one device.  In the reproducible
mode (IRN_DETERMINISTIC, default 1; run_train.py --deterministic) the step sets the process's mode before its first
convolution like the label steps, the loss back-propagates through its ordered gather and the heads' `Upsample -> ReLU`
through `ops.upsample_bilinear`: no float atomic takes part in a gradient.  `--deterministic 0` keeps the faster scatter
kernels, whose gradients are reproducible to rounding only.  `--irn_trunk inference` (default `autograd`) runs the frozen
trunk of a step under `no_grad` on the label steps' inference path (`Net.forward_train`): the process then completes its
MIOpen database from the shipped one (`_tuned.miopen_setup`), a crop the database is tuned for goes through the
channels-last split-GEMM pass in rows of 16, any other crop — in the reproducible mode — through NCHW passes of 2 rows, which
can be slower than `autograd`.  Initial weights: `--irn_init_weights` (a state dict, loaded
non-strictly: an ImageNet trunk, or an earlier checkpoint), else the seeded random state of net.weights; nothing is
downloaded.
"""
import os

import torch
from torch.utils.data import DataLoader

from .. import _tuned
from ..misc import indexing, pyutils, torchutils
from ..net import weights
from ..net.resnet50_irn import AffinityDisplacementLoss
from ..voc12 import dataloader
from . import _classes

MAX_LOADER_WORKERS = 8


def build_model(args, path_index):
    model = AffinityDisplacementLoss(path_index)
    init = getattr(args, "irn_init_weights", None)
    if init:
        state = torch.load(init, map_location="cpu", weights_only=True)
    else:
        state = weights.random_irn_state()
    model.load_state_dict(state, strict=False)
    return model


def device_augment(args):
    return getattr(args, "irn_augment", "device") != "host"


def make_datasets(args, seed):
    """(train, infer) datasets as step/train_irn.py:33-38, 87-90 configures them; raw items when the batch is built on the GPU."""
    raw = device_augment(args)
    train = dataloader.VOC12AffinityDataset(args.train_list, label_dir=args.ir_label_out_dir, voc12_root=args.voc12_root,
                                            hor_flip=True, crop_size=args.irn_crop_size, crop_method="random",
                                            rescale=(0.5, 1.5), seed=seed, raw=raw)
    infer = dataloader.VOC12ImageDataset(args.infer_list, voc12_root=args.voc12_root, crop_size=args.irn_crop_size, raw=raw)
    return train, infer


def _loader(dataset, args, shuffle, seed):
    gen = torch.Generator().manual_seed(seed)
    raw = getattr(dataset, "raw", False)
    return DataLoader(dataset, batch_size=args.irn_batch_size, shuffle=shuffle, drop_last=True, pin_memory=not raw,
                      num_workers=max(0, min(int(args.num_workers), MAX_LOADER_WORKERS)), generator=gen,
                      collate_fn=dataloader.affinity_collate if raw else None)


def device_batch(pack, crop, device):
    """Loader batch of the training set -> (GPU fp32 [B,3,crop,crop], GPU uint8 [B,crop/4,crop/4]): raw items through
    `ops.augment_pair_batch`, the host pipeline's arrays as they are."""
    if "aug" in pack:
        from .. import ops
        return ops.augment_pair_batch(pack["img"], pack["label_map"], pack["aug"], crop, reduce=4, device=device)
    return pack["img"].to(device, non_blocking=True), pack["label"].to(device, non_blocking=True)


def device_images(pack, crop, device):
    """Loader batch of the displacement-mean pass -> GPU fp32 [B,3,crop,crop]."""
    if "aug" in pack:
        from .. import ops
        return ops.augment_batch(pack["img"], pack["aug"], crop, device=device)
    return pack["img"].to(device, non_blocking=True)


def irn_trunk(args):
    mode = getattr(args, "irn_trunk", "autograd") or "autograd"
    if mode not in ("autograd", "inference"):
        raise ValueError("train_irn: irn_trunk is 'autograd' or 'inference', got %r" % (mode,))
    return mode


def check_split_overflow(trunk):
    """`--irn_trunk inference`: the trunk ran through the split-precision GEMMs; an activation beyond fp16's range there
    invalidates the step (read-back: synchronises)."""
    if trunk == "inference":
        from .. import ops
        if ops.split_overflowed():
            raise RuntimeError("train_irn: an activation of the trunk was beyond fp16's range (|x| > 65504) or NaN inside the "
                               "split-precision convolutions; the steps since the last check are INVALID.  Run with "
                               "`run_train.py --split_gemm 0` (IRN_SPLIT_GEMM=0): the fp32 GEMMs have no such limit.")


def train_step(model, optimizer, img, label, trunk="autograd", n_classes=20):
    """One optimisation step on a batch already on the device; returns the four losses as a device tensor [4].  `n_classes`:
    the dataset's foreground classes (labels above it are ignored by the loss)."""
    kw = {} if trunk == "autograd" else {"trunk": trunk}
    if n_classes != 20:
        kw["n_classes"] = n_classes
    parts = model.fused_losses(img, label, **kw)
    pos_aff_loss, neg_aff_loss, dp_fg_loss, dp_bg_loss = parts
    total_loss = (pos_aff_loss + neg_aff_loss) / 2 + (dp_fg_loss + dp_bg_loss) / 2
    optimizer.zero_grad()
    total_loss.backward()
    optimizer.step()
    return torch.stack([p.detach() for p in parts])


def displacement_mean(model, loader, device):
    """Mean over the batches of `loader` of the per-batch channel means of the displacement field (step/train_irn.py:97-107)."""
    means = []
    with torch.no_grad():
        for pack in loader:
            _, dp = model(device_images(pack, loader.dataset.crop_size, device), False)
            means.append(torch.mean(dp, dim=(0, 2, 3)))
    if not means:
        raise RuntimeError("train_irn: infer_list holds fewer images than one batch of %d" % loader.batch_size)
    return torch.mean(torch.stack(means), dim=0)


def run(args):
    """Returns {'first_losses': [4 floats], 'first_counts': [bg, fg, neg pairs of the first batch], 'steps': int}: the losses
    and pair counts of the first step and the steps taken."""
    # the mode only, before the model is built or a convolution runs
    with _tuned.process_mode():
        if irn_trunk(args) == "inference":
            # the tuned channels-last pass is taken only in a process whose MIOpen database has been completed from the shipped
            # one; the default mode leaves MIOpen as it finds it, so that its solver choices do not move
            _tuned.miopen_setup(torch.cuda.current_device())
        return _run(args)


def _run(args):
    device = torch.device("cuda", torch.cuda.current_device())
    seed = int(getattr(args, "seed", 0))
    torch.manual_seed(seed)
    grid = args.irn_crop_size // 4
    path_index = indexing.PathIndex(radius=10, default_size=(grid, grid))
    model = build_model(args, path_index)

    trunk = irn_trunk(args)
    n_classes = _classes.num_classes(args)
    train_dataset, infer_dataset = make_datasets(args, seed)
    max_step = (len(train_dataset) // args.irn_batch_size) * args.irn_num_epoches
    if max_step == 0:
        raise RuntimeError("train_irn: train_list holds fewer images than one batch of %d" % args.irn_batch_size)

    edge_params, dp_params = model.trainable_parameters()
    optimizer = torchutils.PolyOptimizer([
        {"params": edge_params, "lr": 1 * args.irn_learning_rate, "weight_decay": args.irn_weight_decay},
        {"params": dp_params, "lr": 10 * args.irn_learning_rate, "weight_decay": args.irn_weight_decay},
    ], lr=args.irn_learning_rate, weight_decay=args.irn_weight_decay, max_step=max_step)

    model = model.to(device)
    model.train()
    timer = pyutils.Timer()
    first, first_counts, pending = None, None, []
    for ep in range(args.irn_num_epoches):
        print("Epoch %d/%d" % (ep + 1, args.irn_num_epoches))
        train_dataset.set_epoch(ep)
        for it, pack in enumerate(_loader(train_dataset, args, True, seed + ep)):
            img, label = device_batch(pack, args.irn_crop_size, device)
            pending.append(train_step(model, optimizer, img, label, trunk, n_classes))
            if first is None:
                first = [float(v) for v in pending[0].cpu()]
                first_counts = [int(v) for v in model.last_pair_counts.cpu()]
            if (optimizer.global_step - 1) % 50 == 0:
                timer.update_progress(optimizer.global_step / max_step)
                mean = torch.stack(pending).mean(0).cpu()          # the one read-back per 50 steps
                check_split_overflow(trunk)
                pending = []
                print("step:%5d/%5d" % (optimizer.global_step - 1, max_step),
                      "loss:%.4f %.4f %.4f %.4f" % tuple(float(v) for v in mean),
                      "imps:%.1f" % ((it + 1) * args.irn_batch_size / timer.get_stage_elapsed()),
                      "lr: %.4f" % (optimizer.param_groups[0]["lr"]),
                      "etc:%s" % (timer.str_estimated_complete()), flush=True)
        timer.reset_stage()

    check_split_overflow(trunk)                                    # before anything is saved
    model.eval()
    # the mean is that of the raw field: in eval mode `mean_shift` subtracts whatever the initial weights carried (zeros in
    # the reference, which always starts from a fresh module; an earlier checkpoint or the seeded random state do not)
    model.mean_shift.running_mean.zero_()
    print("Analyzing displacements mean ... ", end="")
    model.mean_shift.running_mean = displacement_mean(model, _loader(infer_dataset, args, False, seed), device)
    print("done.")

    out_dir = os.path.dirname(args.irn_weights_name)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    torch.save(model.to("cpu").state_dict(), args.irn_weights_name)      # (on the host: the aliased entries stay one storage)
    torch.cuda.empty_cache()
    return {"first_losses": first, "first_counts": first_counts, "steps": optimizer.global_step}
