"""Host side of the reproducible training step: the two C entries behind it (irn_aff_loss_backward_ordered,
irn_upsample_bilinear_backward) refuse bad arguments before a device is touched, the Python tier refuses CPU tensors, and
header, library and irn_amd/_lib.py agree on both.  None of it needs a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from irn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("irn_aff_loss_backward_ordered", "irn_upsample_bilinear_backward")


def test_header_library_and_bindings_agree_on_the_new_entries():
    src = open(os.path.join(ROOT, "include", "irn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "include/irn_hip.h does not declare %s" % name
        assert hasattr(_lib.lib, name), "the library does not export %s" % name
        assert name in _lib.EXPORTS
    # the ordered backward takes the arguments of the atomic one; the header states the contract next to the other's
    ordered, atomic = _lib.lib.irn_aff_loss_backward_ordered, _lib.lib.irn_aff_loss_backward
    assert ordered.argtypes == atomic.argtypes and ordered.restype == atomic.restype
    assert len(_lib.lib.irn_upsample_bilinear_backward.argtypes) == 9
    comment = src[src.index("reproducible to rounding, NOT bit for bit"):src.index("size_t irn_aff_loss_workspace_bytes")]
    assert "irn_aff_loss_backward_ordered" in comment and "No atomics" in comment and "identical bits" in comment


def test_ordered_backward_refuses_bad_arguments_before_any_device():
    L = _lib.lib
    one = C.c_void_p(64)                                     # never dereferenced on these paths
    need = L.irn_aff_loss_workspace_bytes(2, 33, 47, 5)

    def bwd(edge=one, dp=one, label=one, batch=2, hp=33, wp=47, radius=5, coef=one, ge=one, gd=one, ws=one, ws_bytes=need):
        return L.irn_aff_loss_backward_ordered(edge, dp, label, batch, hp, wp, radius, 21, coef, ge, gd, ws, ws_bytes, None)

    for name in ("edge", "dp", "label", "coef", "ge", "gd", "ws"):
        assert bwd(**{name: None}) == 1, name
        assert b"irn_aff_loss_backward_ordered" in L.irn_last_error()
    assert bwd(batch=0) == 1
    assert bwd(radius=1) == 1 and bwd(radius=17) == 1 and b"radius" in L.irn_last_error()
    assert bwd(hp=4) == 1 and b"too small" in L.irn_last_error()          # hp <= rf
    assert bwd(wp=8) == 1 and b"too small" in L.irn_last_error()          # wp <= 2 rf
    assert bwd(ws_bytes=need - 1) == 3 and b"workspace" in L.irn_last_error()      # IRN_ERR_STATE


def test_upsample_backward_refuses_bad_arguments_before_any_device():
    L = _lib.lib
    one = C.c_void_p(64)

    def bwd(grad_out=one, out=one, n_planes=1, h=4, w=4, factor=2, relu=1, grad_in=one):
        return L.irn_upsample_bilinear_backward(grad_out, out, n_planes, h, w, factor, relu, grad_in, None)

    assert bwd(grad_out=None) == 1 and b"irn_upsample_bilinear_backward" in L.irn_last_error()
    assert bwd(grad_in=None) == 1
    assert bwd(out=None) == 1 and b"ReLU" in L.irn_last_error()            # the mask needs the forward's output
    assert bwd(factor=0) == 1 and b"factor" in L.irn_last_error()
    assert bwd(factor=65) == 1 and bwd(factor=-2) == 1
    assert bwd(h=0) == 1 and bwd(w=0) == 1 and bwd(n_planes=-1) == 1
    assert bwd(n_planes=0) == 0                                            # nothing to do is not an error
    assert bwd(n_planes=0, out=None, relu=0) == 0


def test_python_tier_refuses_cpu_tensors_and_keeps_its_defaults():
    from irn_amd import ops
    from irn_amd.misc import indexing
    e, d, lab = torch.rand(1, 7, 11), torch.randn(1, 2, 7, 11), torch.zeros(1, 7, 11, dtype=torch.uint8)
    for ordered in (False, True):
        with pytest.raises(ValueError):
            indexing.affinity_displacement_sums(e.requires_grad_(True), d, lab, 5, ordered=ordered)
    assert inspect.signature(indexing.affinity_displacement_sums).parameters["ordered"].default is False
    with pytest.raises(ValueError):
        ops.upsample_bilinear(torch.zeros(1, 1, 4, 4, requires_grad=True), 2, relu=True)


def test_train_irn_restores_the_callers_mode(monkeypatch):
    """`train_irn.run` establishes the process's mode before anything else and puts the caller's flags back, also when the
    step fails (here: at its first statement behind the mode, for want of a GPU or of arguments)."""
    import argparse
    from irn_amd.net import resnet50 as _r50
    from irn_amd.step import train_irn
    seen = {}

    def fake_run(args):
        seen["mode"] = (torch.backends.cudnn.deterministic, _r50.DETERMINISTIC)
        raise RuntimeError("stop here")

    monkeypatch.setattr(train_irn, "_run", fake_run)
    for env, want in (("1", (True, True)), ("0", (False, False))):
        monkeypatch.setenv("IRN_DETERMINISTIC", env)
        for before in ((False, None), (True, None)):
            monkeypatch.setattr(torch.backends.cudnn, "deterministic", before[0])
            monkeypatch.setattr(_r50, "DETERMINISTIC", before[1])
            with pytest.raises(RuntimeError, match="stop here"):
                train_irn.run(argparse.Namespace())
            assert seen["mode"] == want
            assert (torch.backends.cudnn.deterministic, _r50.DETERMINISTIC) == before
