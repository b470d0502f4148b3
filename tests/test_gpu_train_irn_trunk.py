"""IRNet training with the frozen trunk on the inference path (`Net.forward_train`, run_train.py --irn_trunk inference) at the
shapes of tests/test_gpu_train_reproducible.py: crop 96, batch 2, radius 10.  The trunk runs under `no_grad` and hands the
heads plain NCHW tensors; outputs and head gradients are as close to fp64 as those of `forward` under autograd, in the
default layout and through the channels-last -> NCHW seam; two steps give identical bits; two fresh processes write the same
checkpoint; `--irn_trunk autograd` is the run without the flag."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _aff_loss_ref as R  # noqa: E402
from _train_cases import reproducible_mode, run_child  # noqa: E402,F401

pytestmark = pytest.mark.gpu
HEADS = ("fc_edge", "fc_dp")


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def images():
    return torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(5))


@pytest.fixture(scope="module")
def fp64_yardstick(images):
    """`Net.forward` in fp64 on the CPU, composed ops, and the gradients of a fixed linear functional of (edge, dp) — computed
    once for both layouts."""
    return _run("forward", torch.float64, torch.device("cpu"), images)


def _functional(edge, dp):
    g = torch.Generator().manual_seed(9)
    ge, gd = torch.randn(edge.shape, generator=g), torch.randn(dp.shape, generator=g)
    return (edge * ge.to(edge)).sum() + (dp * gd.to(dp)).sum()


def _run(method, dtype, dev, images):
    from irn_amd.net import weights
    from irn_amd.net.resnet50_irn import Net
    model = Net()
    model.load_state_dict(weights.random_irn_state(), strict=False)
    model = model.to(dev, dtype).train()
    edge, dp = getattr(model, method)(images.to(dev, dtype))
    assert edge.grad_fn is not None and dp.grad_fn is not None
    _functional(edge, dp).backward()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert grads and all(k.startswith(HEADS) for k in grads), [k for k in grads if not k.startswith(HEADS)]
    assert set(grads) == {k for k, _ in model.named_parameters() if k.startswith(HEADS)}
    return edge.detach(), dp.detach(), grads


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def test_the_trunk_runs_without_autograd_and_hands_over_plain_nchw_features(reproducible_mode, images, monkeypatch):
    from irn_amd.net import weights
    from irn_amd.net.resnet50_irn import Net
    model = Net()
    model.load_state_dict(weights.random_irn_state(), strict=False)
    model = model.to(_dev()).train()
    seen = []
    heads = model.heads
    monkeypatch.setattr(model, "heads", lambda *f: (seen.append(f), heads(*f))[1])
    edge, dp = model.forward_train(images.to(_dev()))
    assert edge.grad_fn is not None and dp.grad_fn is not None
    assert edge.shape == (2, 1, 24, 24) and dp.shape == (2, 2, 24, 24)
    (feats,) = seen
    assert [int(f.shape[1]) for f in feats] == [64, 256, 512, 1024, 2048]
    assert all(not f.requires_grad and f.grad_fn is None and f.is_contiguous() for f in feats)
    _functional(edge, dp).backward()
    with_grad = [k for k, p in model.named_parameters() if p.grad is not None]
    assert with_grad and all(k.startswith(HEADS) for k in with_grad)
    assert torch.backends.cudnn.deterministic is True                              # the mode's resting state


@pytest.mark.parametrize("layout", ["default", "channels_last"])
def test_forward_train_is_as_close_to_fp64_as_forward_under_autograd(reproducible_mode, images, fp64_yardstick, layout, monkeypatch):
    """Yardstick: fp64 on the CPU.  (A) `forward` under autograd in fp32 on the GPU, (B) `forward_train`.  Measure: relative
    L2 distance from fp64 of edge, dp and EVERY head parameter's gradient; err(B) <= 4 * err(A) (the margin of
    tests/test_gpu_train_cam.py).  `channels_last`: the trunk of (B) forced onto the channels-last path (fused GEMMs), so that
    the channels-last -> `to_nchw` -> heads seam runs; (A) under autograd is NCHW whatever the switch says."""
    from irn_amd.net import resnet50 as _r50
    if layout == "channels_last":
        monkeypatch.setattr(_r50, "CHANNELS_LAST_MODE", "1")
    before = dict(_r50.PASS_STATS)
    e64, d64, g64 = fp64_yardstick
    ea, da, ga = _run("forward", torch.float32, _dev(), images)
    mid = dict(_r50.PASS_STATS)
    eb, db, gb = _run("forward_train", torch.float32, _dev(), images)
    after = dict(_r50.PASS_STATS)
    assert mid["nchw"] == before["nchw"] + 1 and mid["channels_last"] == before["channels_last"]
    key = "channels_last" if layout == "channels_last" else "nchw"
    assert after[key] == mid[key] + 1, (mid, after)
    assert g64.keys() == ga.keys() == gb.keys()
    errs = {"edge": (_rel(ea, e64), _rel(eb, e64)), "dp": (_rel(da, d64), _rel(db, d64))}
    errs.update({k + ".grad": (_rel(ga[k], g64[k]), _rel(gb[k], g64[k])) for k in g64})
    worst = max(errs, key=lambda k: errs[k][1] / max(errs[k][0], 1e-300))
    print("\n%s: relative L2 error against fp64, forward (A) / forward_train (B): edge %.3e / %.3e, dp %.3e / %.3e; worst ratio "
          "B/A at %s: %.3e / %.3e" % ((layout,) + errs["edge"] + errs["dp"] + (worst,) + errs[worst]))
    bad = {k: v for k, v in errs.items() if not v[1] <= 4 * v[0]}
    assert not bad, "forward_train further from fp64 than 4x forward under autograd: %s" % bad


def test_two_steps_from_one_state_give_identical_gradient_bits(reproducible_mode):
    import copy
    from irn_amd.misc import indexing, torchutils
    from irn_amd.net import weights
    from irn_amd.net.resnet50_irn import AffinityDisplacementLoss
    from irn_amd.step import train_irn
    model = AffinityDisplacementLoss(indexing.PathIndex(10, (24, 24)))
    model.load_state_dict(weights.random_irn_state(), strict=False)
    model = model.to(_dev()).train()
    state = copy.deepcopy(model.state_dict())
    img = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(5)).to(_dev())
    label = torch.from_numpy(R.make_inputs(10, 2, 24, 24, seed=12)[2]).to(_dev())
    heads = [(k, p) for k, p in model.named_parameters() if k.startswith(HEADS)]
    trunk = [p for k, p in model.named_parameters() if not k.startswith(HEADS)]

    def step():
        model.load_state_dict(state)
        edge_params, dp_params = model.trainable_parameters()
        opt = torchutils.PolyOptimizer([{"params": edge_params, "lr": 0.1, "weight_decay": 1e-4},
                                        {"params": dp_params, "lr": 1.0, "weight_decay": 1e-4}], lr=0.1, weight_decay=1e-4, max_step=4)
        losses = train_irn.train_step(model, opt, img, label, "inference")
        return losses.clone(), {k: p.grad.clone() for k, p in heads}

    l1, g1 = step()
    l2, g2 = step()
    assert all(p.grad is None for p in trunk)
    assert torch.isfinite(l1).all() and torch.equal(l1, l2)
    assert all(torch.isfinite(v).all() for v in g1.values()) and any(v.abs().max() > 0 for v in g1.values())
    differing = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not differing, "head parameters whose .grad differs between two identical steps: %s" % differing
    with pytest.raises(ValueError):
        model.fused_losses(img, label, trunk="fast")


def _argv(root, lst, label_dir, out, workers, log, extra=()):
    return ["--voc12_root", root, "--train_list", lst, "--infer_list", lst, "--ir_label_out_dir", label_dir, "--irn_crop_size", "96",
            "--irn_batch_size", "2", "--irn_num_epoches", "1", "--num_workers", str(workers), "--irn_weights_name", out,
            "--log_name", log, "--train_irn_pass", "True", "--seed", "4"] + list(extra)


def test_two_processes_on_the_inference_trunk_write_the_same_checkpoint(tmp_path):
    """`run_train.py --train_irn_pass True --irn_trunk inference` in two fresh processes, the loader without workers and with
    two: the same first-step losses and the same state dict, tensor for tensor."""
    root = str(tmp_path)
    lst, label_dir = R.write_voc(root, 4)                      # four 120x140 images; crop 96 -> grid 24x24; batch 2 -> 2 steps
    runs = []
    for tag, workers in (("a", 0), ("b", 2)):
        out = os.path.join(root, "sess_" + tag, "res50_irn.pth")
        argv = _argv(root, lst, label_dir, out, workers, os.path.join(root, "log_" + tag), ("--irn_trunk", "inference"))
        res, stdout = run_child("run_train", argv, out + ".json")                                # stops at the first failure
        assert "'irn_trunk': 'inference'" in stdout
        res = res["train_irn"]
        assert res["steps"] == 2
        runs.append((res["first_losses"], torch.load(out, map_location="cpu", weights_only=True)))
    (losses0, state0), (losses1, state1) = runs
    print("\nfirst-step losses a: %s / b: %s" % (losses0, losses1))
    assert "mean_shift.running_mean" in state0 and np.isfinite(losses0).all() and losses0 == losses1
    assert list(state0) == list(state1)
    assert all(torch.isfinite(v).all() for v in state0.values())
    differing = [k for k in state0 if not torch.equal(state0[k], state1[k])]
    assert not differing, "the two runs differ in %s" % differing


def test_trunk_autograd_is_the_run_without_the_flag(tmp_path):
    import run_train
    from irn_amd.step import train_irn
    root = str(tmp_path)
    lst, label_dir = R.write_voc(root, 4)
    runs = {}
    for tag, extra in (("none", ()), ("autograd", ("--irn_trunk", "autograd"))):
        out = os.path.join(root, "sess_" + tag, "res50_irn.pth")
        args = run_train.build_parser().parse_args(_argv(root, lst, label_dir, out, 0, os.path.join(root, "log"), extra))
        res = train_irn.run(args)
        assert res["steps"] == 2 and np.isfinite(res["first_losses"]).all()
        runs[tag] = (res["first_losses"], torch.load(out, map_location="cpu", weights_only=True))
    assert runs["none"][0] == runs["autograd"][0]
    assert all(torch.equal(runs["none"][1][k], runs["autograd"][1][k]) for k in runs["none"][1])
