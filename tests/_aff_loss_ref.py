"""Restatement of the IRNet training losses for the tests of the fused loss (irn_amd/csrc/aff_loss.hip).

`sums_and_counts` is the fp64 CPU statement of what `indexing.affinity_displacement_sums` returns: pair labels from
`PathIndex.src_indices / dst_indices` (reference voc12/dataloader.py:80-106), affinities as 1 - max_pool over the path
axis (net/resnet50_irn.py:162-175, so autograd sends a path's gradient to the first cell attaining the maximum, like the
kernels), pair displacements against `search_dst` (:177-196), the logarithms of :206-207 and the masked sums of
step/train_irn.py:58-64.  `losses` forms the four scalars of those lines from sums and counts.

`make_degenerate_inputs` is the second input family (quantised edges, integer displacements, labels on both sides of the
ignore threshold), `degeneracy` counts what it is there to provoke, `addend_magnitudes` gives the per-cell scale of a
rounding bound on the gradients.

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


def _pair_disp(dp, path_index, sign=-1.0):
    """dp at the source minus (`sign` = -1) dp at the destination; `sign` = 1 adds the two (`addend_magnitudes`)."""
    b = dp.shape[0]
    flat = dp.reshape(b, 2, -1)
    src = torch.from_numpy(np.ascontiguousarray(path_index.src_indices))
    dst = torch.from_numpy(np.ascontiguousarray(path_index.dst_indices))
    return flat[:, :, src][:, :, None] + sign * flat[:, :, dst.reshape(-1)].view(b, 2, *dst.shape)     # [B, 2, |S|, N]


def _constants(fp32_constants):
    """(1e-5, 1 + 1e-5) as fp64 numbers, or the fp32 roundings of the two that fp32 arithmetic works with (1.00001f - 1.0f
    is 1.00136e-5, not 1e-5: where an edge saturates, that difference is the whole term)."""
    if fp32_constants:
        return float(np.float32(1e-5)), float(np.float32(1. + 1e-5))
    return 1e-5, 1. + 1e-5


def _terms(edge, dp, label, radius, fp32_constants=False):
    """The per-pair tensors of the loss in fp64: masks (bg, fg, neg) [B,|S|,N], pos_l / neg_l [B,|S|,N], the pair
    displacement [B,2,|S|,N] and its fg target [1,2,|S|,1]."""
    hp, wp = edge.shape[-2:]
    pi = indexing.PathIndex(radius, (hp, wp))
    masks = tuple(torch.from_numpy(m) for m in batch_pair_labels(label, pi))
    eps, one_eps = _constants(fp32_constants)
    aff = _affinity(edge.double(), pi)
    pos_l = -torch.log(aff + eps)
    neg_l = -torch.log(one_eps - aff)
    pd = _pair_disp(dp.double(), pi)
    target = torch.as_tensor(pi.search_dst, dtype=torch.float64).t()[None, :, :, None]       # [1, 2, |S|, 1] (dy, dx)
    return pi, masks, pos_l, neg_l, pd, target


def sums_and_counts(edge, dp, label, radius, fp32_constants=False):
    """edge [B,hp,wp], dp [B,2,hp,wp] (any float, CPU; taken to fp64, autograd flows to them), label uint8 [B,hp,wp]
    -> (sums fp64 [5], counts int64 numpy [3]).  `fp32_constants`: see `_constants` (the arithmetic stays fp64)."""
    _, (bg, fg, neg), pos_l, neg_l, pd, target = _terms(edge, dp, label, radius, fp32_constants)
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


def total_loss_coefficients(counts):
    """d total_loss / d sums[0..4]: what the backward of the total loss hands to the operator as `grad_sums` (fp64 numpy)."""
    s = torch.zeros(5, dtype=torch.float64, requires_grad=True)
    total_loss(s, counts).backward()
    return s.grad.numpy()


def reference(edge, dp, label, radius, fp32_constants=False, coef=None):
    """numpy inputs -> dict(sums [5], counts [3], losses [4], grad_edge, grad_dp): fp64; the gradients are those of the total
    loss, or of `(coef * sums).sum()` where five coefficients are given."""
    e = torch.from_numpy(np.asarray(edge)).double().requires_grad_(True)
    d = torch.from_numpy(np.asarray(dp)).double().requires_grad_(True)
    sums, counts = sums_and_counts(e, d, label, radius, fp32_constants)
    if coef is None:
        total_loss(sums, counts).backward()
    else:
        (sums * torch.as_tensor(np.asarray(coef, np.float64))).sum().backward()
    return {"sums": sums.detach().numpy(), "counts": counts,
            "losses": np.asarray([float(v) for v in losses(sums.detach(), counts)]),
            "grad_edge": e.grad.numpy(), "grad_dp": d.grad.numpy()}


def addend_magnitudes(edge, dp, label, radius, coef, fp32_constants=False):
    """Per cell, the sum of the |addends| that make up its gradient of `(coef * sums).sum()`: (edge map, dp map), fp64.
    What a per-cell rounding bound scales with — a cell whose figure is 0 receives no gradient at all.
    Every addend of the edge gradient is coef / (aff + 1e-5) >= 0 for an equal pair and -coef / (1 + 1e-5 - aff) <= 0 for an
    unequal one, so their magnitudes are the gradient of |c0| s0 + |c1| s1 - |c2| s2.  An addend of the dp gradient is
    +-coef * sgn(residual), + at the source and - at the destination: the magnitudes are the gradient of
    |c| * [residual != 0] * (dp[source] + dp[destination]) summed over the pairs."""
    w = np.abs(np.asarray(coef, np.float64))
    e = torch.from_numpy(np.asarray(edge)).double().requires_grad_(True)
    d = torch.from_numpy(np.asarray(dp)).double().requires_grad_(True)
    pi, (bg, fg, neg), pos_l, neg_l, pd, target = _terms(e, d, label, radius, fp32_constants)
    both = _pair_disp(d, pi, sign=1.0)
    nz_fg, nz_bg = ((pd - target) != 0).detach().double(), (pd != 0).detach().double()
    total = w[0] * (pos_l * bg).sum() + w[1] * (pos_l * fg).sum() - w[2] * (neg_l * neg).sum() \
        + w[3] * (both * nz_fg * fg[:, None]).sum() + w[4] * (both * nz_bg * bg[:, None]).sum()
    total.backward()
    return e.grad.numpy(), d.grad.numpy()


def degeneracy(edge, dp, label, radius):
    """How many counted pairs (bg, fg or neg) have a path maximum attained by two or more cells, and how many fg / bg pairs
    have a displacement residual component of exactly 0: (tied, fg_zero, bg_zero)."""
    e = torch.from_numpy(np.asarray(edge)).double()
    pi, (bg, fg, neg), _, _, pd, target = _terms(e, torch.from_numpy(np.asarray(dp)), label, radius)
    flat = e.reshape(e.shape[0], -1)
    tied = []
    for ind in pi.path_indices:
        ind = torch.from_numpy(np.ascontiguousarray(ind))
        dist = torch.index_select(flat, 1, ind.reshape(-1)).view(flat.shape[0], *ind.shape)          # [B, n, L, N]
        tied.append((dist == dist.max(dim=2, keepdim=True).values).sum(2) >= 2)
    tied = torch.cat(tied, 1) & (bg | fg | neg)
    fg_zero = (((pd - target) == 0).any(1) & fg).sum()
    bg_zero = ((pd == 0).any(1) & bg).sum()
    return int(tied.sum()), int(fg_zero), int(bg_zero)


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


# (radius, batch, hp, wp).  The table-driven forward (every radius but 5 and 10) at the smallest and the largest legal radius
# (3x3 sources each) and at two ordinary radii off the tile grid; source rectangles of exactly one 8x32 tile and of one cell
# more each way, at radius 5 and 3; radius 10 with a source rectangle of exactly one tile.
GENERIC_AND_SEAM_SHAPES = ((2, 2, 4, 5), (16, 1, 18, 33), (3, 2, 11, 37), (7, 1, 20, 50),
                           (5, 1, 12, 40), (5, 1, 13, 41), (3, 1, 10, 36), (10, 1, 17, 50))
COEFFICIENT_SHAPE = (5, 2, 13, 41)              # two images, two tiles each way: the coefficients one at a time
# shape -> seed of `make_degenerate_inputs` at which every pair class, a tied path and exactly-zero fg and bg residuals occur
# (tests/test_aff_loss_cpu.py checks each entry; 3x3 sources are few, so not every seed serves)
DEGENERATE_SEED = {
    (2, 2, 4, 5): 206, (16, 1, 18, 33): 1618, (3, 2, 11, 37): 311, (7, 1, 20, 50): 720,
    (5, 1, 12, 40): 512, (5, 1, 13, 41): 513, (3, 1, 10, 36): 310, (10, 1, 17, 50): 1017,
    COEFFICIENT_SHAPE: 513,
}
assert set(DEGENERATE_SEED) == set(GENERIC_AND_SEAM_SHAPES) | {COEFFICIENT_SHAPE}


def make_degenerate_inputs(radius, batch, hp, wp, seed):
    """The inputs at which the rules of the kernels show: edge from {0, 0.25, 0.5, 0.75, 1} (most paths have tied maxima, and
    both saturations occur: edge == 1 is aff == 0, edge == 0 along a whole path is aff == 1), integer-valued dp in [-2, 2]
    (residuals of exactly 0 and of exactly (dy, dx)), labels in 2x2 blocks from {0, 1, 20, 21, 254, 255} (both sides of the
    ignore threshold; about a quarter of the cells ignored)."""
    rng = np.random.RandomState(seed)
    edge = rng.choice(np.asarray([0, 0.25, 0.5, 0.75, 1.0], np.float32), (batch, hp, wp))
    dp = rng.randint(-2, 3, (batch, 2, hp, wp)).astype(np.float32)
    coarse = rng.choice(np.asarray([0, 1, 20, 21, 254, 255], np.uint8), (batch, -(-hp // 2), -(-wp // 2)),
                        p=[0.35, 0.2, 0.2, 0.09, 0.08, 0.08])
    label = np.repeat(np.repeat(coarse, 2, 1), 2, 2)[:, :hp, :wp]
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
