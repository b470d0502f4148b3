"""Scaffolding the training tests share (tests/test_gpu_train_*.py): the process's reproducible mode as a fixture, imported
by name, and one way of running a training command in a fresh process."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import importlib, json, sys
res = importlib.import_module(sys.argv[1]).main(sys.argv[3:])
json.dump(res, open(sys.argv[2], "w"), default=lambda v: v.tolist())
"""


@pytest.fixture()
def reproducible_mode(monkeypatch):
    """The process's mode as the training steps' `run` establishes it, put back afterwards."""
    from irn_amd.net import resnet50 as _r50
    from irn_amd.step import _common
    saved = (torch.backends.cudnn.deterministic, _r50.DETERMINISTIC)
    monkeypatch.setenv("IRN_DETERMINISTIC", "1")
    _common.apply_deterministic_setting()
    yield
    torch.backends.cudnn.deterministic, _r50.DETERMINISTIC = saved


def run_child(module_name, argv, out_json, timeout=300):
    """`<module_name>.main(argv)` (run_train, run_train_cam, run_train_seg) in a fresh process started at the repository root,
    in the default mode; what `main` returned goes through `out_json`.  -> (that dict, the process's output)."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("IRN_DETERMINISTIC", None)                         # the default mode is the reproducible one
    done = subprocess.run([sys.executable, "-c", CHILD, module_name, out_json] + list(argv), cwd=ROOT, env=env, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, "%s %s failed:\n%s" % (module_name, out_json, done.stdout[-3000:])      # stop at the first failure
    return json.load(open(out_json)), done.stdout
