"""fp64 restatement of the backward of the trunk's fused training tail (irn_bn_act_backward, ops.bn_act), given the ReLU
mask: with z = (x - mean) / sqrt(var + eps) * weight + bias (+ r), r = res or the shortcut's batch norm of res, and
dz = grad_out * mask,

    grad_x = dz * scale                 scale = weight / sqrt(var + eps)
    grad_res = dz  or  dz * res_scale
    S0[c] = sum dz,  S1[c] = sum dz * x,  S2[c] = sum dz * res                    (over images and plane)
    grad_weight = (S1 - mean * S0) / sqrt(var + eps),  grad_bias = S0            (the shortcut's layer: S2, its mean / var)

Everything here is numpy float64 on whatever it is given; nothing is rounded."""
import numpy as np


def _per_channel(v, ndim):
    return np.asarray(v, dtype=np.float64).reshape((1, -1) + (1,) * (ndim - 2))


def relu_mask(out):
    """torch's threshold_backward: the gradient passes where out > 0 and where out is NaN."""
    out = np.asarray(out)
    return ~(out <= 0)


def sums(grad_out, mask, x, res=None):
    """(S0, S1, S2 or None) float64 [C], and the sums of the terms' magnitudes (for error bounds)."""
    dz = np.where(mask, np.asarray(grad_out, dtype=np.float64), 0.0)
    axes = (0,) + tuple(range(2, dz.ndim))
    terms = [dz, dz * np.asarray(x, dtype=np.float64)] + ([] if res is None else [dz * np.asarray(res, dtype=np.float64)])
    s = [t.sum(axis=axes) for t in terms]
    mags = [np.abs(t).sum(axis=axes) for t in terms]
    return (s + [None])[:3], (mags + [None])[:3]


def grads(grad_out, mask, scale, res_scale=None):
    """(grad_x, grad_res) float64, exact products of the masked gradient and the (fp32) constants."""
    dz = np.where(mask, np.asarray(grad_out, dtype=np.float64), 0.0)
    gx = dz * _per_channel(scale, dz.ndim)
    gr = dz if res_scale is None else dz * _per_channel(res_scale, dz.ndim)
    return gx, gr


def param_grads(s0, s1, mean, var, eps):
    """(grad_weight, grad_bias) float64 [C]."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    return (s1 - mean * s0) / np.sqrt(var + eps), s0
