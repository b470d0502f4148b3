"""Restatement of the fused segmentation loss (irn_amd/csrc/seg_loss.hip) for tests/test_gpu_seg_loss.py: fp64 on the CPU,
composed torch ops, gradients from autograd.  Importing it touches no GPU.

    upsampled(x, f, H, W)          F.interpolate(x, scale_factor=f, bilinear, align_corners=False)[..., :H, :W]
    sums_counts_grad(x, lab, f, coef)   per-image cross-entropy sums, valid-pixel counts, d(sum_b coef[b] * sums[b]) / dx
    make_case(shape, seed, ...)    random normal logits of scale 3 and the issue's label mix
"""
import numpy as np
import torch
import torch.nn.functional as F

# (B, C, h, w, factor, H, W): the smallest shapes at which each part of the kernels can go wrong
SHAPES = (
    (1, 2, 1, 1, 4, 4, 4),            # a single coarse cell, clamped on all four sides
    (2, 21, 3, 5, 8, 24, 40),
    (1, 21, 3, 5, 8, 19, 37),         # a window that is not the full grid
    (3, 21, 19, 23, 2, 38, 46),       # more coarse cells than one 8x8 workgroup tile in both directions: seams and halos
    (1, 21, 19, 23, 16, 304, 368),
    (1, 81, 4, 4, 16, 64, 64),        # LDS at the class cap
    (2, 21, 6, 6, 1, 6, 6),           # factor 1
)


def upsampled(x, f, H, W):
    return F.interpolate(x, scale_factor=f, mode="bilinear", align_corners=False)[..., :H, :W]


def mapped_labels(label, C):
    """int64 labels with every byte >= C turned into 255 (the ignore index)."""
    lab = label.long()
    return torch.where(lab >= C, torch.full_like(lab, 255), lab)


def sums_counts_grad(x, label, f, coef=None, dtype=torch.float64, device="cpu"):
    """x: fp32 [B,C,h,w] (CPU), label: uint8 [B,H,W] (CPU) -> (sums [B], counts int64 [B], grad [B,C,h,w]) computed in
    `dtype` on `device` by the composed ops; coef [B] (default ones) weighs the images' sums in the scalar differentiated."""
    B, C = x.shape[:2]
    H, W = label.shape[1:]
    xs = x.to(device=device, dtype=dtype).requires_grad_(True)
    lab = mapped_labels(label, C).to(device)
    z = upsampled(xs, f, H, W)
    sums = torch.stack([F.cross_entropy(z[b:b + 1], lab[b:b + 1], ignore_index=255, reduction="sum") for b in range(B)])
    cf = torch.ones(B) if coef is None else coef
    (sums * cf.to(device=device, dtype=dtype)).sum().backward()
    counts = (lab != 255).sum(dim=(1, 2))
    return sums.detach().cpu(), counts.cpu(), xs.grad.detach().cpu()


def make_labels(B, C, H, W, rng, void=0.2, foreign=0.05):
    """Uniform in 0..C-1, `void` of the pixels 255, `foreign` of them bytes in C..254 (labels of another class list)."""
    lab = rng.integers(0, C, size=(B, H, W))
    u = rng.random((B, H, W))
    lab[u < void] = 255
    if C < 255:
        pick = (u >= void) & (u < void + foreign)
        lab[pick] = rng.integers(C, 255, size=int(pick.sum()))
    return torch.from_numpy(lab.astype(np.uint8))


def make_case(shape, seed):
    B, C, h, w, f, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, h, w, generator=g) * 3.0
    label = make_labels(B, C, H, W, np.random.default_rng(seed))
    coef = torch.rand(B, generator=g) + 0.5
    return x, label, coef
