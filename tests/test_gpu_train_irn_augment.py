"""`train_irn` with its input batch built on the device against the same step with the host pipeline: `run_train.py
--train_irn_pass True` in two fresh processes with one seed — `--irn_augment host` without loader workers, `--irn_augment
device` with two — on four synthetic images (crop 96, batch 2, one epoch) reports the same first-step losses and writes the
same state dict, tensor for tensor, the displacement mean included."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _aff_loss_ref as R  # noqa: E402
from _train_cases import run_child  # noqa: E402

pytestmark = pytest.mark.gpu
def test_device_and_host_pipelines_write_the_same_checkpoint(tmp_path):
    root = str(tmp_path)
    lst, label_dir = R.write_voc(root, 4)                      # four 120x140 images; crop 96 -> grid 24x24; batch 2 -> 2 steps
    runs = []
    for augment, workers in (("host", 0), ("device", 2)):
        out = os.path.join(root, "sess_" + augment, "res50_irn.pth")
        argv = ["--voc12_root", root, "--train_list", lst, "--infer_list", lst, "--ir_label_out_dir", label_dir,
                "--irn_crop_size", "96", "--irn_batch_size", "2", "--irn_num_epoches", "1", "--num_workers", str(workers),
                "--irn_weights_name", out, "--log_name", os.path.join(root, "log_" + augment), "--train_irn_pass", "True", "--seed", "4",
                "--irn_augment", augment]
        res, stdout = run_child("run_train", argv, out + ".json")                                # stops at the first failure
        assert "'irn_augment': '%s'" % augment in stdout
        res = res["train_irn"]
        assert res["steps"] == 2
        runs.append((res["first_losses"], torch.load(out, map_location="cpu", weights_only=True)))
    (losses_h, state_h), (losses_d, state_d) = runs
    print("\nfirst-step losses host: %s / device: %s" % (losses_h, losses_d))
    assert np.isfinite(losses_h).all() and losses_h == losses_d
    assert list(state_h) == list(state_d) and "mean_shift.running_mean" in state_h
    assert all(torch.isfinite(v).all() for v in state_h.values())
    differing = [k for k in state_h if not torch.equal(state_h[k], state_d[k])]
    assert not differing, "the host and the device pipelines differ in %s" % differing
    assert state_h["mean_shift.running_mean"].abs().max() > 0
