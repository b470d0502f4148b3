"""Restatement of the IRNet training losses for the tests of the fused loss (irn_amd/csrc/aff_loss.hip).

`sums_and_counts` is the fp64 CPU statement of what `indexing.affinity_displacement_sums` returns: pair labels from
`PathIndex.src_indices / dst_indices` (reference voc12/dataloader.py:80-106), affinities as 1 - max_pool over the path
axis (net/resnet50_irn.py:162-175, so autograd sends a path's gradient to the first cell attaining the maximum, like the
kernels), pair displacements against `search_dst` (:177-196), the logarithms of :206-207 and the masked sums of
step/train_irn.py:58-64.  `losses` forms the four scalars of those lines from sums and counts.

`composed_sums` is the same on the GPU in fp32 through the operators the project had before the fused pass
(`edge_to_affinity`, `pair_displacement` and the arithmetic of `AffinityDisplacementLoss.forward`) with float masks and
`torch.sum`: the baseline whose distance from the fp64 statement sets the tolerance of the fused pass.
"""
import numpy as np
import torch
import torch.nn.functional as F

from irn_amd.misc import indexing


def pair_labels(label, path_index):
    """label: uint8 [hp, wp] -> (bg, fg, neg) bool [|S|, N]."""
    flat = np.asarray(label).reshape(-1).astype(np.int64)
    a = flat[path_index.src_indices][None]
    b = flat[path_index.dst_indices]
    valid = (a < 21) & (b < 21)
    same = a == b
    return valid & same & (a == 0), valid & same & (a > 0), valid & ~same


def batch_pair_labels(label, path_index):
    per = [pair_labels(m, path_index) for m in np.asarray(label)]
    return tuple(np.stack([p[i] for p in per]) for i in range(3))            # each [B, |S|, N]


def _affinity(edge, path_index):
    e = edge.reshape(edge.shape[0], -1)
    out = []
    for ind in path_index.path_indices:                                      # [n_paths, L, N] per path length
        ind = torch.from_numpy(np.ascontiguousarray(ind))
        dist = torch.index_select(e, 1, ind.reshape(-1)).view(e.shape[0], *ind.shape)
        out.append(1 - F.max_pool2d(dist, (dist.shape[2], 1)).squeeze(2))
    return torch.cat(out, 1)                                                 # [B, |S|, N]


def _pair_disp(dp, path_index):
    b = dp.shape[0]
    flat = dp.reshape(b, 2, -1)
    src = torch.from_numpy(np.ascontiguousarray(path_index.src_indices))
    dst = torch.from_numpy(np.ascontiguousarray(path_index.dst_indices))
    return flat[:, :, src][:, :, None] - flat[:, :, dst.reshape(-1)].view(b, 2, *dst.shape)     # [B, 2, |S|, N]


def sums_and_counts(edge, dp, label, radius):
    """edge [B,hp,wp], dp [B,2,hp,wp] (any float, CPU; taken to fp64, autograd flows to them), label uint8 [B,hp,wp]
    -> (sums fp64 [5], counts int64 numpy [3])."""
    hp, wp = edge.shape[-2:]
    pi = indexing.PathIndex(radius, (hp, wp))
    bg, fg, neg = (torch.from_numpy(m) for m in batch_pair_labels(label, pi))
    aff = _affinity(edge.double(), pi)
    pos_l = -torch.log(aff + 1e-5)
    neg_l = -torch.log(1. + 1e-5 - aff)
    pd = _pair_disp(dp.double(), pi)
    target = torch.as_tensor(pi.search_dst, dtype=torch.float64).t()[None, :, :, None]       # [1, 2, |S|, 1] (dy, dx)
    fg_l = torch.abs(pd - target)
    bg_l = torch.abs(pd)
    sums = torch.stack([(pos_l * bg).sum(), (pos_l * fg).sum(), (neg_l * neg).sum(),
                        (fg_l * fg[:, None]).sum(), (bg_l * bg[:, None]).sum()])
    counts = np.asarray([int(bg.sum()), int(fg.sum()), int(neg.sum())], np.int64)
    return sums, counts


def losses(sums, counts):
    """The four scalars of step/train_irn.py:58-64 from the five sums and (bg, fg, neg) counts."""
    n = [float(c) for c in counts] if not torch.is_tensor(counts) else counts.to(sums.dtype)
    pos = sums[0] / (n[0] + 1e-5) / 2 + sums[1] / (n[1] + 1e-5) / 2
    return pos, sums[2] / (n[2] + 1e-5), sums[3] / (2 * n[1] + 1e-5), sums[4] / (2 * n[0] + 1e-5)


def total_loss(sums, counts):
    pos, neg, fg, bg = losses(sums, counts)
    return (pos + neg) / 2 + (fg + bg) / 2


def reference(edge, dp, label, radius):
    """numpy inputs -> dict(sums [5], counts [3], losses [4], grad_edge, grad_dp): fp64, gradients of the total loss."""
    e = torch.from_numpy(np.asarray(edge)).double().requires_grad_(True)
    d = torch.from_numpy(np.asarray(dp)).double().requires_grad_(True)
    sums, counts = sums_and_counts(e, d, label, radius)
    total_loss(sums, counts).backward()
    return {"sums": sums.detach().numpy(), "counts": counts,
            "losses": np.asarray([float(v) for v in losses(sums.detach(), counts)]),
            "grad_edge": e.grad.numpy(), "grad_dp": d.grad.numpy()}


def composed_sums(edge, dp, label, radius):
    """GPU fp32 tensors (label uint8, on the GPU too) -> (sums fp32 [5], counts fp32 [3]) through the composed operators."""
    b, hp, wp = label.shape
    pi = indexing.PathIndex(radius, (hp, wp))
    bg, fg, neg = (torch.from_numpy(m.astype(np.float32)).to(edge.device) for m in batch_pair_labels(label.cpu().numpy(), pi))
    aff = indexing.edge_to_affinity(edge.reshape(b, -1), radius=radius, size=(hp, wp))
    pos_l = (-1) * torch.log(aff + 1e-5)
    neg_l = (-1) * torch.log(1. + 1e-5 - aff)
    pd = indexing.pair_displacement(dp, radius)
    target = torch.as_tensor(pi.search_dst, dtype=torch.float32, device=edge.device).t()[None, :, :, None]
    fg_l = torch.abs(pd - target)
    bg_l = torch.abs(pd)
    sums = torch.stack([torch.sum(bg * pos_l), torch.sum(fg * pos_l), torch.sum(neg * neg_l),
                        torch.sum(fg_l * fg[:, None]), torch.sum(bg_l * bg[:, None])])
    return sums, torch.stack([bg.sum(), fg.sum(), neg.sum()])


def make_inputs(radius, batch, hp, wp, seed, block=4):
    """Random edge in (0,1), random dp, labels from {0, 3, 7, 255} in blocks of `block` cells (all four pair classes occur)."""
    rng = np.random.RandomState(seed)
    edge = rng.uniform(0.02, 0.98, (batch, hp, wp)).astype(np.float32)
    dp = (rng.randn(batch, 2, hp, wp) * 3).astype(np.float32)
    coarse = rng.choice(np.asarray([0, 3, 7, 255], np.uint8), (batch, -(-hp // block), -(-wp // block)), p=[0.4, 0.25, 0.2, 0.15])
    label = np.repeat(np.repeat(coarse, block, 1), block, 2)[:, :hp, :wp]
    return edge, dp, np.ascontiguousarray(label)


def write_voc(root, n, h=120, w=140, seed=0):
    """n synthetic JPEGs and IR-label PNGs (0 / class+1 / 255 in blocks) under root; returns (list file, label dir)."""
    import os

    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "ir_label"))
    names = []
    for i in range(n):
        name = "2007_%06d" % (i + 1)
        names.append(name)
        img = np.clip(rng.randint(0, 255, (h // 8 + 1, w // 8 + 1, 3)).repeat(8, 0).repeat(8, 1)[:h, :w] + rng.randint(-9, 9, (h, w, 3)), 0, 255)
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=92)
        lab = rng.choice(np.asarray([0, 3, 7, 255], np.uint8), (h // 16 + 1, w // 16 + 1)).repeat(16, 0).repeat(16, 1)[:h, :w]
        Image.fromarray(lab).save(os.path.join(root, "ir_label", name + ".png"))
    lst = os.path.join(root, "train.txt")
    with open(lst, "w") as f:
        f.write("\n".join(names) + "\n")
    return lst, os.path.join(root, "ir_label")
