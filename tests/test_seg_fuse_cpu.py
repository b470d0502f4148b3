"""What of the multi-scale inference path can be checked without a GPU: irn_seg_fuse and irn_crf_prob refuse bad arguments before
a device is touched (null device pointers stand in wherever the entry never dereferences them), the Python tier refuses CPU
tensors and bad lists, the step's flags parse, and the oracle's taps are those of the integer-factor upsampling at Hs == H."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from irn_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _seg_fuse_ref as R  # noqa: E402

L = _lib.lib
one = 64                               # never dereferenced on these paths
ARG, STATE = 1, 3
GOOD = dict(maps=(one, one), h=(3, 5), w=(4, 6), Hs=(40, 70), Ws=(50, 90), C=21, stride=16, H=70, W=90, label=one, prob=one)


def _fuse(**kw):
    a = dict(GOOD, **kw)
    m = a.get("M", None if a["maps"] is None else len(a["maps"]))
    arr = lambda v: None if v is None else _lib.i32_array(v)        # noqa: E731
    return L.irn_seg_fuse(None if a["maps"] is None else _lib.ptr_array(a["maps"]), arr(a["h"]), arr(a["w"]), arr(a["Hs"]),
                          arr(a["Ws"]), m, a["C"], a["stride"], a["H"], a["W"], a["label"], a["prob"], None)


def _refused(what, **kw):
    assert _fuse(**kw) == ARG, what
    assert b"irn_seg_fuse" in L.irn_last_error(), (what, L.irn_last_error())
    return L.irn_last_error()


def test_seg_fuse_refuses_every_bad_argument_before_a_device_is_touched():
    for name in ("maps", "h", "w", "Hs", "Ws"):
        assert b"null pointer" in _refused(name + " NULL", **{name: None, "M": 2})
    assert b"null pointer" in _refused("both outputs NULL", label=None, prob=None)
    assert b"maps[1]" in _refused("a NULL map", maps=(one, None))
    assert b"aligned" in _refused("a misaligned map", maps=(one, 66))
    assert b"aligned" in _refused("a misaligned prob", prob=66)
    for m in (0, 17, -1):
        assert b"M " in _refused("M %d" % m, M=m)
    for c in (1, 82, 0):
        assert b"C " in _refused("C %d" % c, C=c)
    for s in (0, 65):
        assert b"stride" in _refused("stride %d" % s, stride=s)
    for kw in ({"H": 0}, {"W": 0}, {"H": 32769}, {"W": 40000}):
        assert b"output" in _refused(str(kw), **kw)
    for kw in ({"h": (0, 5)}, {"w": (4, 0)}, {"h": (3, 32769)}):
        assert b"cells" in _refused(str(kw), **kw)
    for kw in ({"Hs": (0, 70)}, {"Ws": (50, -3)}, {"Hs": (49, 70)}, {"Ws": (50, 97)}):      # 49 > 3 * 16, 97 > 6 * 16
        assert b"Hs, Ws" in _refused(str(kw), **kw)
    assert b"finer" in _refused("a map finer than the output", H=2, Hs=(33, 70), h=(3, 5))    # 33 > 16 * 2
    assert b"finer" in _refused("a map finer than the output", W=3, Ws=(50, 49))              # 50 > 16 * 3


def test_a_geometry_that_fits_no_tile_is_refused_before_a_device_is_touched():
    n = 16
    msg = _refused("81 classes, 16 maps at ratio 1", maps=(one,) * n, h=(4,) * n, w=(4,) * n, Hs=(64,) * n, Ws=(64,) * n, C=81, H=4, W=4)
    assert b"geometry" in msg and b"LDS" in msg


def _crf(rgb=one, prob=one, l=21, h=24, w=32, t=1, labels=one, ws=one, ws_bytes=None):
    need = L.irn_crf_prob_workspace_bytes(h, w, l)
    return L.irn_crf_prob(rgb, prob, l, h, w, t, labels, None, ws, need if ws_bytes is None else ws_bytes, None)


def test_crf_prob_workspace_and_refusals():
    for l in (-1, 0, 1, 33, 64):
        assert L.irn_crf_prob_workspace_bytes(24, 32, l) == 0, l
    for l in (2, 21, 32):
        assert L.irn_crf_prob_workspace_bytes(24, 32, l) > 0, l
    assert L.irn_crf_prob_workspace_bytes(0, 32, 21) == 0 == L.irn_crf_prob_workspace_bytes(24, 0, 21)
    for kw in ({"l": 1}, {"l": 33}, {"t": -1}, {"h": 0}, {"w": 0}, {"rgb": None}, {"prob": None}, {"labels": None}, {"ws": None}):
        assert _crf(**kw) == ARG, kw
        assert b"irn_crf_prob" in L.irn_last_error(), (kw, L.irn_last_error())
    assert _crf(ws_bytes=L.irn_crf_prob_workspace_bytes(24, 32, 21) - 1) == STATE
    assert b"irn_crf_prob" in L.irn_last_error() and b"workspace" in L.irn_last_error()


def test_the_python_tier_refuses_cpu_tensors_and_bad_lists():
    from irn_amd import ops
    x = torch.zeros(3, 2, 2)
    for args, kw in ((([x], [(32, 32)], 16, (32, 32)), {}),                             # a CPU tensor
                     (([], [], 16, (32, 32)), {}), (([x] * 17, [(32, 32)] * 17, 16, (32, 32)), {}),
                     ((x, [(32, 32)], 16, (32, 32)), {}),                               # not a list
                     (([x], [(32, 32), (16, 16)], 16, (32, 32)), {}), (([x], None, 16, (32, 32)), {}),
                     (([x], [(32, 32)], 0, (32, 32)), {}), (([x], [(32, 32)], 16.0, (32, 32)), {}), (([x], [(32, 32)], True, (32, 32)), {}),
                     (([x], [(32, 32)], 16, (32, 32)), {"want_label": False}),
                     (([x], [32], 16, (32, 32)), {}), (([x], [(32, 32)], 16, 32), {}), (([x], [(32, 32)], 16, (0, 32)), {})):
        with pytest.raises(ValueError, match="seg_fuse"):
            ops.seg_fuse(*args, **kw)
    img = np.zeros((4, 4, 3), np.uint8)
    for prob in (torch.zeros(3, 4, 4), None, np.zeros((3, 4, 4), np.float32)):
        with pytest.raises(ValueError, match="crf_prob"):
            ops.crf_prob(img, prob)


def test_run_train_seg_has_the_inference_flags():
    import run_train_seg
    from irn_amd.step import infer_sem_seg
    parse = run_train_seg.build_parser().parse_args
    args = parse(["--voc12_root", "x"])
    assert list(args.seg_infer_scales) == [1.0] and args.seg_crf_iters == 0
    assert infer_sem_seg.modes(args, 20) == ([1.0], 0)
    args = parse(["--voc12_root", "x", "--seg_infer_scales", "0.5", "0.75", "1", "1.25", "1.5", "--seg_crf_iters", "10"])
    assert infer_sem_seg.modes(args, 20) == ([0.5, 0.75, 1.0, 1.25, 1.5], 10)
    assert infer_sem_seg.modes(args, 31) == ([0.5, 0.75, 1.0, 1.25, 1.5], 10)
    with pytest.raises(ValueError, match=r"--seg_crf_iters 10 with --num_classes 32.*32 labels"):
        infer_sem_seg.modes(args, 32)
    args.seg_crf_iters = 0
    assert infer_sem_seg.modes(args, 80)[1] == 0                        # without the CRF every class count stays allowed
    for bad in ([0.0], [-1.0], [4.5], [float("nan")], [1.0] * 17, []):
        args.seg_infer_scales = bad
        with pytest.raises(ValueError, match="--seg_infer_scales"):
            infer_sem_seg.modes(args, 20)
    args.seg_infer_scales, args.seg_crf_iters = [1.0], -1
    with pytest.raises(ValueError, match="--seg_crf_iters"):
        infer_sem_seg.modes(args, 20)


@pytest.mark.parametrize("factor", [1, 2, 3, 4, 7, 8, 16, 64])
def test_the_oracles_taps_at_full_size_are_those_of_the_integer_factor(factor):
    for n in (1, 2, 5, 23):
        for n_out in sorted({1, factor, n * factor - factor // 2, n * factor}):
            if n_out < 1 or (n_out + factor - 1) // factor > n:
                continue
            # Hs == H: the ratio Hs / (stride * H) is 1 / stride whatever H is, and rounds to the same float32
            assert R.ratio(n_out, factor, n_out) == np.float32(1.0 / factor)
            got, want = R.taps(n_out, n, R.ratio(n_out, factor, n_out)), R.integer_factor_taps(n_out, n, factor)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (factor, n, n_out)


def test_the_oracle_refuses_a_tap_past_the_map():
    with pytest.raises(AssertionError, match="past an axis"):
        R.taps(64, 3, R.ratio(64, 16, 64))                                # 64 outputs at 1/16 need four cells
    p = R.fuse(*R.case_maps((9, 7, 2, (1, 2), 16)), 16, (9, 7))
    assert p.shape == (2, 9, 7) and np.allclose(p.sum(0), 1.0, atol=1e-12)
