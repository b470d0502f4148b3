#!/usr/bin/env python3
"""The differentiable fused tail (`ops.bn_act`: fold, one forward pass, one backward pass + the channel sums) against the
composed autograd ops it replaces (F.batch_norm(training=False) -> add -> ReLU and ATen's backward of each), forward +
backward with gradients for x, the residual and the layer's weight and bias.  Prints one JSON line per case.

    python tools/bn_act_train_bench.py [--reps 20] [--warmup 3]

Shapes: the tails of the trained stages at batch 16, crop 512 — [16,256,32,32], [16,1024,32,32], [16,2048,32,32] — and
[16,256,64,64], each without a residual, with one, and with a batch norm on the residual (a stage's first unit).  Device time
between two events around forward + backward, median over `--reps` after `--warmup`, the two paths alternating call by call.
`bytes` is what the fused path must move (forward: x (+ res) read, out written; backward: grad_out, out, x (+ res for its own
batch norm) read, grad_x (+ grad_res) written), `gb_per_s` that over the fused median.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(16, 256, 32, 32), (16, 1024, 32, 32), (16, 2048, 32, 32), (16, 256, 64, 64)]
MODES = ("plain", "residual", "residual_bn")
EPS = 1e-5


def make_case(shape, mode, dev):
    g = torch.Generator().manual_seed(1)
    c = shape[1]
    t = {"x": torch.randn(shape, generator=g), "grad_out": torch.randn(shape, generator=g)}
    if mode != "plain":
        t["res"] = torch.randn(shape, generator=g)
    for p in ("", "r_") if mode == "residual_bn" else ("",):
        t[p + "weight"], t[p + "bias"] = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
        t[p + "mean"], t[p + "var"] = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    t = {k: v.to(dev) for k, v in t.items()}
    for k in ("x", "res", "weight", "bias", "r_weight", "r_bias"):
        if k in t:
            t[k].requires_grad_(True)
    return t


def fused(t, mode):
    from irn_amd import ops
    rbn = (t["r_weight"], t["r_bias"], t["r_mean"], t["r_var"], EPS) if mode == "residual_bn" else None
    return ops.bn_act(t["x"], t["weight"], t["bias"], t["mean"], t["var"], EPS, t.get("res"), True, rbn)


def composed(t, mode):
    y = F.batch_norm(t["x"], t["mean"], t["var"], t["weight"], t["bias"], False, 0.0, EPS)
    if mode == "residual":
        y = y + t["res"]
    elif mode == "residual_bn":
        y = y + F.batch_norm(t["res"], t["r_mean"], t["r_var"], t["r_weight"], t["r_bias"], False, 0.0, EPS)
    return F.relu(y)


def timed(fn, t, mode):
    for v in t.values():
        v.grad = None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(t, mode).backward(t["grad_out"])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def moved_bytes(shape, mode):
    n = 4
    for v in shape:
        n *= v
    fwd = {"plain": 2, "residual": 3, "residual_bn": 3}[mode]
    bwd = {"plain": 3 + 1, "residual": 3 + 2, "residual_bn": 4 + 2}[mode]
    return (fwd + bwd) * n


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", default=20, type=int)
    p.add_argument("--warmup", default=3, type=int)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bn_act_train_bench needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    for shape in SHAPES:
        for mode in MODES:
            t = make_case(shape, mode, dev)
            ms = {"fused": [], "composed": []}
            for r in range(a.warmup + a.reps):
                for name, fn in (("fused", fused), ("composed", composed)):          # alternating
                    v = timed(fn, t, mode)
                    if r >= a.warmup:
                        ms[name].append(v)
            nbytes = moved_bytes(shape, mode)
            out = {"shape": list(shape), "mode": mode, "reps": a.reps, "bytes": nbytes}
            for name in ms:
                out[name + "_ms_median"] = statistics.median(ms[name])
                out[name + "_ms_min"], out[name + "_ms_max"] = min(ms[name]), max(ms[name])
            out["gb_per_s"] = nbytes / (out["fused_ms_median"] * 1e-3) / 1e9
            out["composed_over_fused"] = out["composed_ms_median"] / out["fused_ms_median"]
            print(json.dumps({"bn_act_train": out}), flush=True)


if __name__ == "__main__":
    main()
