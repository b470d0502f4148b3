"""Sharding primitive of the hot path (API mirror of reference misc/torchutils.py:66-68) and the optimiser of the
IRNet training step (`PolyOptimizer`, :9-31)."""
import numpy as np
import torch
from torch.utils.data import Subset


class PolyOptimizer(torch.optim.SGD):
    """Plain SGD (weight decay, no momentum) whose learning rates follow lr0 * (1 - step / max_step) ** 0.9 per parameter
    group, `step` being `global_step`, the number of `step()` calls so far.  At and beyond `max_step` nothing is updated
    (the schedule has reached zero there); `global_step` keeps counting."""

    def __init__(self, params, lr, weight_decay, max_step, power=0.9):
        super().__init__(params, lr=lr, weight_decay=weight_decay)
        self.global_step = 0
        self.max_step = int(max_step)
        self.power = power
        self._lr0 = [g["lr"] for g in self.param_groups]

    def step(self, closure=None):
        if self.global_step < self.max_step:
            mult = (1 - self.global_step / self.max_step) ** self.power
            for g, lr0 in zip(self.param_groups, self._lr0):
                g["lr"] = lr0 * mult
            super().step(closure)
        self.global_step += 1


def split_dataset(dataset, n_splits):
    """Strided shards: shard i holds items i, i+n, i+2n, ...  (one shard per GPU; no overlap, no
    communication between shards)."""
    return [Subset(dataset, np.arange(i, len(dataset), n_splits)) for i in range(n_splits)]


def shard_indices(n_items, rank, world_size):
    """Indices of `rank`'s strided shard — what split_dataset(...)[rank] iterates over."""
    return np.arange(rank, n_items, world_size)
