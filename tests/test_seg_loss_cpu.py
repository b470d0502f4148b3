"""What of the segmentation training path can be checked without a GPU: the four C entries of irn_amd/csrc/seg_loss.hip refuse
bad arguments before a device is touched, the Python tier refuses CPU tensors, run_train_seg.py has its flags, and
net.resnet50_seg.Net takes a CAM checkpoint for its trunk."""
import ctypes as C

import pytest
import torch

from irn_amd import _lib

L = _lib.lib
one = C.c_void_p(64)                   # never dereferenced on these paths
odd = C.c_void_p(66)                   # aligned to nothing wider than 2 bytes
GEOM = (2, 21, 3, 5, 8, 24, 40)        # batch, C, h, w, factor, H, W
ARG, STATE = 1, 3


def _need():
    return L.irn_seg_loss_workspace_bytes(*GEOM)


def _forward(geom=GEOM, logits=one, label=one, sums=one, counts=one, lse=None, ws=one, ws_bytes=None):
    return L.irn_seg_loss_forward(logits, label, *geom, sums, counts, lse, ws, _need() if ws_bytes is None else ws_bytes, None)


def _backward(geom=GEOM, logits=one, label=one, lse=one, coef=one, grad=one, ws=one, ws_bytes=None):
    return L.irn_seg_loss_backward(logits, label, lse, coef, *geom, grad, ws, _need() if ws_bytes is None else ws_bytes, None)


def _argmax(geom=GEOM, logits=one, out=one):
    return L.irn_seg_argmax(logits, *geom, out, None)


def _bad_geometries():
    b, c, h, w, f, hh, ww = GEOM
    return {"batch 0": (0, c, h, w, f, hh, ww), "batch 65536": (65536, c, h, w, f, hh, ww),
            "C 1": (b, 1, h, w, f, hh, ww), "C 82": (b, 82, h, w, f, hh, ww),
            "factor 0": (b, c, h, w, 0, hh, ww), "factor 65": (b, c, h, w, 65, hh, ww),
            "H 0": (b, c, h, w, f, 0, ww), "H above h * factor": (b, c, h, w, f, h * f + 1, ww),
            "W 0": (b, c, h, w, f, hh, 0), "W above w * factor": (b, c, h, w, f, hh, w * f + 1),
            "h 0": (b, c, 0, w, f, hh, ww), "w 0": (b, c, h, 0, f, hh, ww)}


def test_workspace_bytes_is_zero_for_bad_geometry():
    assert _need() == 2 * 1 * 16                     # one 8x8 tile per image: an fp64 sum and an int64 count each
    assert L.irn_seg_loss_workspace_bytes(1, 21, 19, 23, 2, 38, 46) == 9 * 16
    assert L.irn_seg_loss_workspace_bytes(1, 21, 19, 23, 2, 16, 17) == 2 * 16      # the window's tiles only
    for what, geom in _bad_geometries().items():
        assert L.irn_seg_loss_workspace_bytes(*geom) == 0, what


@pytest.mark.parametrize("entry, call", [("irn_seg_loss_forward", _forward), ("irn_seg_loss_backward", _backward),
                                         ("irn_seg_argmax", _argmax)])
def test_bad_geometry_is_refused_before_a_device_is_touched(entry, call):
    for what, geom in _bad_geometries().items():
        assert call(geom=geom) == ARG, what
        assert entry.encode() in L.irn_last_error(), what


def test_null_pointers_are_refused():
    for kw in ({"logits": None}, {"label": None}, {"sums": None}, {"counts": None}, {"ws": None}):
        assert _forward(**kw) == ARG and b"irn_seg_loss_forward: null pointer" in L.irn_last_error(), kw
    for kw in ({"logits": None}, {"label": None}, {"lse": None}, {"coef": None}, {"grad": None}, {"ws": None}):
        assert _backward(**kw) == ARG and b"irn_seg_loss_backward: null pointer" in L.irn_last_error(), kw
    for kw in ({"logits": None}, {"out": None}):
        assert _argmax(**kw) == ARG and b"irn_seg_argmax: null pointer" in L.irn_last_error(), kw


def test_misaligned_pointers_are_refused():
    for kw in ({"sums": odd}, {"counts": C.c_void_p(68)}, {"ws": C.c_void_p(68)}, {"lse": C.c_void_p(68)}, {"logits": odd}):
        assert _forward(**kw) == ARG and b"aligned" in L.irn_last_error() and b"irn_seg_loss_forward" in L.irn_last_error(), kw
    for kw in ({"grad": odd}, {"lse": C.c_void_p(68)}, {"coef": odd}, {"ws": C.c_void_p(68)}):
        assert _backward(**kw) == ARG and b"aligned" in L.irn_last_error() and b"irn_seg_loss_backward" in L.irn_last_error(), kw
    assert _argmax(logits=odd) == ARG and b"irn_seg_argmax" in L.irn_last_error()


def test_a_small_workspace_is_a_state_error():
    assert _forward(ws_bytes=_need() - 1) == STATE
    assert b"irn_seg_loss_forward" in L.irn_last_error() and b"irn_seg_loss_workspace_bytes" in L.irn_last_error()
    assert _backward(ws_bytes=0) == STATE and b"irn_seg_loss_backward" in L.irn_last_error()


def test_the_python_tier_refuses_cpu_tensors_wrong_dtypes_and_strides():
    from irn_amd import ops
    x, lab = torch.zeros(1, 3, 2, 2), torch.zeros(1, 4, 4, dtype=torch.uint8)
    for fn, args in ((ops.seg_loss_sums, (x, lab, 2)), (ops.seg_cross_entropy, (x, lab, 2)), (ops.seg_argmax, (x, 2, (4, 4)))):
        with pytest.raises(ValueError, match="seg_"):
            fn(*args)
    with pytest.raises(ValueError, match="seg_argmax"):
        ops.seg_argmax(None, 2, (4, 4))
    from irn_amd import seg_loss
    with pytest.raises(ValueError, match="seg_loss_sums"):
        seg_loss._need_logits("seg_loss_sums", x.double(), 2)


def test_run_train_seg_has_the_flags():
    import run_train_seg
    args = run_train_seg.build_parser().parse_args(["--voc12_root", "x"])
    assert (args.train_sem_seg_pass, args.infer_sem_seg_pass, args.eval_seg_pass) == (True, False, False)
    assert args.seg_label_dir is None and args.seg_crop_size == 512 and args.seg_batch_size == 16
    assert tuple(args.seg_rescale) == (0.5, 1.5) and args.seg_augment == "device" and args.seg_loss == "fused"
    assert args.seg_init_weights is None
    for name in ("seg_num_epoches", "seg_learning_rate", "seg_weight_decay", "seg_weights_name", "seg_pred_dir", "seed",
                 "num_classes", "sem_seg_out_dir"):
        assert hasattr(args, name), name
    args = run_train_seg.build_parser().parse_args(["--voc12_root", "x", "--seg_loss", "composed", "--seg_augment", "host",
                                                    "--eval_seg_pass", "True", "--seg_rescale", "0.75", "1.25"])
    assert args.seg_loss == "composed" and args.seg_augment == "host" and args.eval_seg_pass is True
    assert list(args.seg_rescale) == [0.75, 1.25]
    with pytest.raises(SystemExit):
        run_train_seg.build_parser().parse_args(["--voc12_root", "x", "--seg_loss", "other"])


def test_the_seg_net_takes_a_cam_checkpoint_for_its_trunk():
    from irn_amd.net import resnet50_cam, resnet50_seg, weights
    cam_state = weights.random_cam_state()
    assert list(cam_state) == list(resnet50_cam.Net().state_dict())
    net = resnet50_seg.Net(20)
    res = net.load_state_dict(cam_state, strict=False)
    assert res.missing_keys and all(k.startswith("head.") for k in res.missing_keys)
    assert all(k.startswith(("classifier.", "newly_added.")) for k in res.unexpected_keys)
    assert torch.equal(net.resnet50.layer3[2].conv2.weight, cam_state["resnet50.layer3.2.conv2.weight"])
    assert net.resnet50.layer4[1].conv2.dilation == (2, 2) and net.resnet50.layer4[0].conv2.stride == (1, 1)
    backbone, head = net.trainable_parameters()
    assert len(head) == 8 and len(backbone) + len(head) == len(list(net.parameters()))
    assert tuple(net(torch.zeros(1, 3, 48, 64)).shape) == (1, 21, 3, 4)
    seg_state = weights.random_seg_state()
    assert list(seg_state) == list(net.state_dict()) and resnet50_seg.Net(20).load_state_dict(seg_state, strict=True)


def test_net_80_has_81_outputs():
    from irn_amd.net import resnet50_seg
    net = resnet50_seg.Net(80)
    assert all(m.out_channels == 81 and m.bias is not None for m in net.head.branches)
    assert [m.dilation for m in net.head.branches] == [(6, 6), (12, 12), (18, 18), (24, 24)]
    with pytest.raises(ValueError):
        resnet50_seg.Net(81)
    with pytest.raises(ValueError, match="head has 81 outputs"):
        resnet50_seg.Net(20).load_state_dict(net.state_dict(), strict=False)
