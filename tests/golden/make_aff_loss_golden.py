#!/usr/bin/env python3
"""Generate tests/golden/aff_loss.npz by running the reference's own training-loss code on the CPU.

What runs is the reference, unmodified (set up as in make_golden.py): `AffinityDisplacementLoss.forward`
(net/resnet50_irn.py:198-213) with `Net.forward` replaced by a function that hands back seeded boundary logits and a
displacement field (the trunk is not what is recorded), and `GetAffinityLabelFromIndices` (voc12/dataloader.py:80-106)
on the indices of the reference's `PathIndex`.  The four scalars are then formed as step/train_irn.py:58-64 forms them.
Radius 5, grid 12x16, batch 2.  Re-run:  python tests/golden/make_aff_loss_golden.py
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.join(OUT, "..", ".."))
sys.path.insert(0, os.path.join(OUT, ".."))

import make_golden  # noqa: E402


def main():
    from _aff_loss_ref import make_inputs
    make_golden._install_reference()
    from misc import indexing
    from net import resnet50_irn
    from voc12 import dataloader

    radius, batch, hp, wp = 5, 2, 12, 16
    sig, dp, label = make_inputs(radius, batch, hp, wp, seed=2024)
    logit = torch.from_numpy(np.log(sig / (1 - sig)).astype(np.float32))[:, None]
    dp = torch.from_numpy(dp)

    pi = indexing.PathIndex(radius=radius, default_size=(hp, wp))
    loss = resnet50_irn.AffinityDisplacementLoss.__new__(resnet50_irn.AffinityDisplacementLoss)
    torch.nn.Module.__init__(loss)
    loss.path_index = pi
    loss.n_path_lengths = len(pi.path_indices)
    for i, pind in enumerate(pi.path_indices):
        loss.register_buffer(resnet50_irn.AffinityDisplacementLoss.path_indices_prefix + str(i), torch.from_numpy(pind))
    loss.register_buffer("disp_target", torch.from_numpy(pi.search_dst).transpose(1, 0)[None, :, :, None].float())
    resnet50_irn.Net.forward = lambda self, x: (logit, dp)
    pos_aff_loss, neg_aff_loss, dp_fg_loss, dp_bg_loss = loss(None, True)

    get = dataloader.GetAffinityLabelFromIndices(pi.src_indices, pi.dst_indices)
    labs = [get(m) for m in label]
    bg_pos_label, fg_pos_label, neg_label = (torch.stack([lab[i] for lab in labs]) for i in range(3))

    bg_pos_aff_loss = torch.sum(bg_pos_label * pos_aff_loss) / (torch.sum(bg_pos_label) + 1e-5)
    fg_pos_aff_loss = torch.sum(fg_pos_label * pos_aff_loss) / (torch.sum(fg_pos_label) + 1e-5)
    pos = bg_pos_aff_loss / 2 + fg_pos_aff_loss / 2
    neg = torch.sum(neg_label * neg_aff_loss) / (torch.sum(neg_label) + 1e-5)
    fg = torch.sum(dp_fg_loss * torch.unsqueeze(fg_pos_label, 1)) / (2 * torch.sum(fg_pos_label) + 1e-5)
    bg = torch.sum(dp_bg_loss * torch.unsqueeze(bg_pos_label, 1)) / (2 * torch.sum(bg_pos_label) + 1e-5)

    np.savez_compressed(os.path.join(OUT, "aff_loss.npz"),
                        radius=np.int32(radius), edge=torch.sigmoid(logit)[:, 0].numpy(), dp=dp.numpy(), label=label,
                        losses=np.asarray([pos.item(), neg.item(), fg.item(), bg.item()], np.float32),
                        counts=np.asarray([bg_pos_label.sum().item(), fg_pos_label.sum().item(), neg_label.sum().item()], np.int64))


if __name__ == "__main__":
    main()
