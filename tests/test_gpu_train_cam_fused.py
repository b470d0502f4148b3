"""The CAM training step with the fused training tail (`resnet50.TRAIN_FUSED_TAIL`, run_train_cam.py --cam_fused_tail 1) at
the shapes of tests/test_gpu_train_cam.py: crop 64, batch 2, random initial weights.  Two identical steps give identical bits
and leave stages 1-2 alone; logits and every trained parameter's gradient are as close to fp64 as the composed fp32 path's;
two fresh processes write the same checkpoint; `--cam_fused_tail 0` is the run without the flag."""
import os
import struct
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as A  # noqa: E402
from _train_cases import reproducible_mode, run_child  # noqa: E402,F401

pytestmark = pytest.mark.gpu
FROZEN = ("resnet50.conv1.", "resnet50.bn1.", "resnet50.layer1.", "resnet50.layer2.")


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(5)
    img = torch.randn(2, 3, 64, 64, generator=g)
    label = torch.zeros(2, 20)
    label[0, [3, 7]] = 1
    label[1, 14] = 1
    return img, label


def test_two_fused_steps_give_the_same_bits_and_leave_stages_1_2_alone(reproducible_mode, batch, monkeypatch):
    import copy
    from irn_amd import ops
    from irn_amd.misc import torchutils
    from irn_amd.net import resnet50 as _r50, weights
    from irn_amd.net.resnet50_cam import Net
    from irn_amd.step import train_cam
    monkeypatch.setattr(_r50, "TRAIN_FUSED_TAIL", True)
    calls = []
    real = ops.bn_act
    monkeypatch.setattr(ops, "bn_act", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    model = Net()
    model.load_state_dict(weights.random_cam_state(), strict=False)
    model = model.to(_dev()).train()
    state = copy.deepcopy(model.state_dict())
    img, label = (t.to(_dev()) for t in batch)
    named = dict(model.named_parameters())
    frozen = [k for k in named if k.startswith(FROZEN)]
    trained = [k for k in named if not k.startswith(FROZEN)]
    assert len(frozen) >= 60 and len(trained) >= 80

    def step():
        model.load_state_dict(state)
        backbone, new = model.trainable_parameters()
        opt = torchutils.PolyOptimizer([{"params": backbone, "lr": 0.1, "weight_decay": 1e-4},
                                        {"params": new, "lr": 1.0, "weight_decay": 1e-4}], lr=0.1, weight_decay=1e-4, max_step=4)
        loss = train_cam.train_step(model, opt, img, label)
        return loss.clone(), {k: named[k].grad.clone() for k in trained}

    l1, g1 = step()
    assert len(calls) == 3 * (6 + 3)                                              # every tail of stages 3-4 took the fused pass
    assert all(named[k].grad is None for k in frozen)
    assert all(torch.equal(named[k].detach(), state[k]) for k in frozen), "a stage 1-2 parameter moved"
    l2, g2 = step()
    assert torch.isfinite(l1) and torch.equal(l1, l2)
    assert all(torch.isfinite(v).all() for v in g1.values()) and all(v.abs().max() > 0 for v in g1.values())
    differing = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not differing, "parameters whose .grad differs between two identical fused steps: %s" % differing


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def test_fused_tail_is_as_close_to_fp64_as_the_composed_path(reproducible_mode, batch, monkeypatch):
    """Yardstick: fp64 on the CPU, composed ops.  (A) `forward_train` in fp32 on the GPU with the composed tail, (B) the same
    with TRAIN_FUSED_TAIL.  Measure: relative L2 distance from fp64 of the logits and of EVERY trained parameter's gradient;
    err(B) <= 4 * err(A), the margin tests/test_gpu_train_cam.py uses for the same kind of comparison."""
    from irn_amd.net import resnet50 as _r50, weights
    from irn_amd.net.resnet50_cam import Net
    img, label = batch
    state = weights.random_cam_state()

    def run(dtype, dev, fused):
        monkeypatch.setattr(_r50, "TRAIN_FUSED_TAIL", fused)
        model = Net()
        model.load_state_dict(state, strict=False)
        model = model.to(dev, dtype).train()
        logits = model.forward_train(img.to(dev, dtype))
        F.multilabel_soft_margin_loss(logits, label.to(dev, dtype)).backward()
        grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        assert not any(k.startswith(FROZEN) for k in grads) and len(grads) >= 80
        return logits, grads

    l64, g64 = run(torch.float64, torch.device("cpu"), False)
    la, ga = run(torch.float32, _dev(), False)
    lb, gb = run(torch.float32, _dev(), True)
    assert g64.keys() == ga.keys() == gb.keys()
    errs = {"logits": (_rel(la, l64), _rel(lb, l64))}
    errs.update({k + ".grad": (_rel(ga[k], g64[k]), _rel(gb[k], g64[k])) for k in g64})
    worst = max(errs, key=lambda k: errs[k][1] / max(errs[k][0], 1e-300))
    print("\nrelative L2 error against fp64, composed (A) / fused (B): logits %.3e / %.3e; worst ratio B/A at %s: %.3e / %.3e; "
          "largest A %.3e, largest B %.3e" % (errs["logits"] + (worst,) + errs[worst] + (max(v[0] for v in errs.values()),
                                                                                          max(v[1] for v in errs.values()))))
    bad = {k: v for k, v in errs.items() if not v[1] <= 4 * v[0]}
    assert not bad, "fused tail further from fp64 than 4x the composed path: %s" % bad


def _argv(root, lst, out, workers, log, extra=()):
    return ["--voc12_root", root, "--train_list", lst, "--val_list", lst, "--cam_crop_size", "64", "--cam_batch_size", "2",
            "--cam_num_epoches", "1", "--cam_resize_long", "48", "96", "--num_workers", str(workers), "--cam_weights_name", out,
            "--log_name", log, "--seed", "4",
            # (the seeded random weights need a small rate to keep both steps finite: tests/test_gpu_train_cam.py)
            "--cam_learning_rate", "1e-5"] + list(extra)


def test_two_processes_with_the_fused_tail_write_the_same_checkpoint(tmp_path):
    """`run_train_cam.py --cam_fused_tail 1` in two fresh processes, the loader without workers and with two: the same state
    dict, tensor for tensor, and it trained."""
    from irn_amd.net import weights
    from irn_amd.net.resnet50_cam import Net
    root = str(tmp_path)
    lst = A.write_voc(root, 4)                                 # four 120x140 images; batch 2 -> 2 steps
    runs = []
    for tag, workers in (("a", 0), ("b", 2)):
        out = os.path.join(root, "sess_" + tag, "res50_cam")
        argv = _argv(root, lst, out, workers, os.path.join(root, "log_" + tag), ("--cam_fused_tail", "1"))
        res, stdout = run_child("run_train_cam", argv, out + ".json")                            # stops at the first failure
        assert "'cam_fused_tail': 1" in stdout
        res = res["train_cam"]
        assert res["steps"] == 2 and np.isfinite(res["val_losses"]).all()
        runs.append((res, torch.load(out + ".pth", map_location="cpu", weights_only=True)))
    (res0, state0), (res1, state1) = runs
    print("\nfirst loss a: %r / b: %r" % (res0["first_loss"], res1["first_loss"]))
    assert np.isfinite(res0["first_loss"]) and res0["first_loss"] == res1["first_loss"] and res0["val_losses"] == res1["val_losses"]
    assert list(state0) == list(state1) == list(Net().state_dict().keys())
    assert all(torch.isfinite(v).all() for v in state0.values()), "the run diverged"
    differing = [k for k in state0 if not torch.equal(state0[k], state1[k])]
    assert not differing, "the two runs differ in %s" % differing
    initial = weights.random_cam_state()
    assert not torch.equal(state0["resnet50.layer3.0.bn3.weight"], initial["resnet50.layer3.0.bn3.weight"])   # a batch norm trained
    assert torch.equal(state0["resnet50.layer2.0.conv1.weight"], initial["resnet50.layer2.0.conv1.weight"])


def test_flag_zero_is_the_run_without_the_flag_and_the_switch_is_put_back(tmp_path):
    import run_train_cam
    from irn_amd.net import resnet50 as _r50
    from irn_amd.step import train_cam
    root = str(tmp_path)
    lst = A.write_voc(root, 4)
    losses = {}
    for tag, extra in (("none", ()), ("zero", ("--cam_fused_tail", "0")), ("one", ("--cam_fused_tail", "1"))):
        args = run_train_cam.build_parser().parse_args(
            _argv(root, lst, os.path.join(root, "sess_" + tag, "res50_cam"), 0, os.path.join(root, "log"), extra))
        args.cam_resize_long = tuple(args.cam_resize_long)
        res = train_cam.run(args)
        assert _r50.TRAIN_FUSED_TAIL is False                                     # restored on return
        assert res["steps"] == 2 and np.isfinite(res["first_loss"])
        losses[tag] = struct.pack("<d", res["first_loss"])
        print("\n%s: first loss %r" % (tag, res["first_loss"]))
    assert losses["none"] == losses["zero"]
    rel = abs(struct.unpack("<d", losses["one"])[0] / struct.unpack("<d", losses["zero"])[0] - 1)
    assert rel < 1e-4, rel                                                        # the same loss up to rounding
