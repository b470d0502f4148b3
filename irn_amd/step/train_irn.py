"""IRNet training (reference step/train_irn.py), single GPU, single process.

Reads  args.train_list, args.infer_list, args.voc12_root, args.ir_label_out_dir (the PNGs of cam_to_ir_label),
       args.irn_crop_size, args.irn_batch_size, args.irn_num_epoches, args.irn_learning_rate, args.irn_weight_decay,
       args.num_workers, args.seed, args.irn_init_weights, args.irn_augment, args.irn_trunk
Writes args.irn_weights_name: the state dict the label steps load (EdgeDisplacement through net.weights.load_checkpoint)

The reference's loop (the shared one, irn_amd/step/_train.py) with three differences.  The input batch is built on the GPU
(`--irn_augment device`, the default): the loader workers hand over the decoded image, the IR label map and the
augmentation's draws, and `ops.augment_pair_batch` rescales, normalises, mirrors and crops the images and gathers the reduced
label maps for the whole batch (irn_amd/csrc/augment.hip), bit for bit what the PIL / numpy pipeline gives for the same draws
— `--irn_augment host` runs that pipeline in the workers instead.  The displacement-mean pass follows the same choice.
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
import torch

from .. import _tuned
from ..misc import indexing
from ..net import weights
from ..net.resnet50_irn import AffinityDisplacementLoss
from ..voc12 import dataloader
from . import _classes, _train

PRINT_EVERY = 50


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


def collate(dataset):
    """Raw items (lists of unequal images) need `affinity_collate`; the host pipeline's arrays stack by default."""
    return dataloader.affinity_collate if getattr(dataset, "raw", False) else None


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
    _train.max_steps("train_irn", "infer_list", loader.dataset, loader.batch_size, 1)
    means = []
    with torch.no_grad():
        for pack in loader:
            _, dp = model(_train.device_images(pack, loader.dataset.crop_size, device), False)
            means.append(torch.mean(dp, dim=(0, 2, 3)))
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
    crop, batch = args.irn_crop_size, args.irn_batch_size
    model = build_model(args, indexing.PathIndex(radius=10, default_size=(crop // 4, crop // 4)))

    trunk = irn_trunk(args)
    n_classes = _classes.num_classes(args)
    train_dataset, infer_dataset = make_datasets(args, seed)
    max_step = _train.max_steps("train_irn", "train_list", train_dataset, batch, args.irn_num_epoches)
    optimizer = _train.two_rate_optimizer(*model.trainable_parameters(), args.irn_learning_rate, args.irn_weight_decay, max_step)

    def make_loader(dataset, shuffle, seed):
        return _train.loader(dataset, batch, args.num_workers, shuffle, seed, collate(dataset))

    first_counts = []

    def step(pack):
        img, label = _train.device_pair(pack, crop, device, reduce=4)
        losses = train_step(model, optimizer, img, label, trunk, n_classes)
        if not first_counts:
            first_counts.extend(int(v) for v in model.last_pair_counts.cpu())
        return losses

    first = _train.fit(model, optimizer, train_dataset, lambda s: make_loader(train_dataset, True, s), device, args.irn_num_epoches,
                       batch, seed, PRINT_EVERY, step, "loss:%.4f %.4f %.4f %.4f", on_report=lambda: check_split_overflow(trunk))

    check_split_overflow(trunk)                                    # before anything is saved
    model.eval()
    # the mean is that of the raw field: in eval mode `mean_shift` subtracts whatever the initial weights carried (zeros in
    # the reference, which always starts from a fresh module; an earlier checkpoint or the seeded random state do not)
    model.mean_shift.running_mean.zero_()
    print("Analyzing displacements mean ... ", end="")
    model.mean_shift.running_mean = displacement_mean(model, make_loader(infer_dataset, False, seed), device)
    print("done.")

    _train.save_state(model, args.irn_weights_name)
    return {"first_losses": [float(v) for v in first], "first_counts": first_counts, "steps": optimizer.global_step}
