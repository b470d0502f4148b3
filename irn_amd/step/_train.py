"""What the training steps (train_cam, train_irn, train_sem_seg) share, stated once and in explicit values: the loader, the
two batch builders, the initial state, the optimiser, the length check, the epoch / step loop and the saving.

The reproducibility contract lives here: the draws of an item come from (seed, epoch, index) — the loop hands the epoch to
`dataset.set_epoch` — and the shuffle of epoch `ep` from a generator seeded `seed + ep`, so a run is fixed by its seed
whatever the number of loader workers.  The loop reads the device once per `print_every` steps; nothing here calls
`torch.cuda.*` except `save_state`'s `empty_cache`, so `fit` runs on the CPU as well.
"""
import os

import torch
from torch.utils.data import DataLoader

from ..misc import pyutils, torchutils

MAX_LOADER_WORKERS = 8


def loader(dataset, batch_size, num_workers, shuffle, seed, collate_fn=None):
    """Whole batches only, in an order fixed by `seed`; a raw dataset's items (bytes and draws) are not pinned."""
    return DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, drop_last=True, pin_memory=not getattr(dataset, "raw", False),
                      num_workers=max(0, min(int(num_workers), MAX_LOADER_WORKERS)), generator=torch.Generator().manual_seed(seed),
                      collate_fn=collate_fn)


def device_images(pack, crop, device):
    """Loader batch -> fp32 [B,3,crop,crop] on the device: raw items through `ops.augment_batch`, the host pipeline's floats
    as they are."""
    if "aug" in pack:
        from .. import ops
        return ops.augment_batch(pack["img"], pack["aug"], crop, device=device)
    return pack["img"].to(device, non_blocking=True)


def device_pair(pack, crop, device, reduce):
    """Loader batch -> (fp32 [B,3,crop,crop], uint8 [B,crop/reduce,crop/reduce]) on the device: raw items through
    `ops.augment_pair_batch`, the host pipeline's arrays as they are."""
    if "aug" in pack:
        from .. import ops
        return ops.augment_pair_batch(pack["img"], pack["label_map"], pack["aug"], crop, reduce=reduce, device=device)
    return pack["img"].to(device, non_blocking=True), pack["label"].to(device, non_blocking=True).contiguous()


def init_state(path, drop=()):
    """The state dict at `path`, loaded on the CPU; a bare ResNet-50 trunk is re-keyed to the `resnet50.` names (the stages
    alias them) without its `fc.*`; keys that start with a prefix in `drop` are left out."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if "conv1.weight" in state:
        state = {"resnet50." + k: v for k, v in state.items() if not k.startswith("fc.")}
    return {k: v for k, v in state.items() if not k.startswith(tuple(drop))} if drop else state


def two_rate_optimizer(base_params, new_params, lr, weight_decay, max_step):
    """Poly-schedule SGD with `base_params` at `lr` and `new_params` at ten times it."""
    return torchutils.PolyOptimizer([{"params": base_params, "lr": lr, "weight_decay": weight_decay},
                                     {"params": new_params, "lr": 10 * lr, "weight_decay": weight_decay}],
                                    lr=lr, weight_decay=weight_decay, max_step=max_step)


def max_steps(step_name, what, dataset, batch_size, epochs):
    """Steps that `epochs` passes over `dataset` in whole batches take; none is an error that names the list `what`."""
    n = (len(dataset) // batch_size) * epochs
    if n == 0:
        raise RuntimeError("%s: %s holds fewer images than one batch of %d" % (step_name, what, batch_size))
    return n


def fit(model, optimizer, dataset, make_loader, device, epochs, batch_size, seed, print_every, step, loss_format,
        on_report=None, after_epoch=None):
    """The epoch / step loop.  `make_loader(seed)` gives one epoch's loader over `dataset`; `step(pack)` takes one
    optimisation step and returns its loss(es) as a device tensor, a scalar or [k], which stays on the device: the mean since
    the last report is read back once per `print_every` steps and printed through `loss_format`.  `on_report()` runs at each
    report behind that read-back, `after_epoch(ep)` behind each epoch.  Returns the first step's value (a CPU tensor)."""
    model.to(device).train()
    max_step = optimizer.max_step
    timer = pyutils.Timer()
    first, pending = None, []
    for ep in range(epochs):
        print("Epoch %d/%d" % (ep + 1, epochs))
        dataset.set_epoch(ep)
        for it, pack in enumerate(make_loader(seed + ep)):
            pending.append(step(pack))
            if first is None:
                first = pending[0].cpu()
            if (optimizer.global_step - 1) % print_every == 0:
                timer.update_progress(optimizer.global_step / max_step)
                mean = torch.stack(pending).mean(0).cpu()          # the one read-back per `print_every` steps
                if on_report is not None:
                    on_report()
                pending = []
                print("step:%5d/%5d" % (optimizer.global_step - 1, max_step),
                      loss_format % tuple(float(v) for v in mean.reshape(-1)),
                      "imps:%.1f" % ((it + 1) * batch_size / timer.get_stage_elapsed()),
                      "lr: %.4f" % (optimizer.param_groups[0]["lr"]),
                      "etc:%s" % (timer.str_estimated_complete()), flush=True)
        if after_epoch is not None:
            after_epoch(ep)
        timer.reset_stage()
    return first


def save_state(model, path):
    """The model's state dict to `path`, from the host: there the aliased entries stay one storage."""
    out_dir = os.path.dirname(path)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    torch.save(model.to("cpu").state_dict(), path)
    torch.cuda.empty_cache()
