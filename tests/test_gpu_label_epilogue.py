"""irn_label_epilogue and irn_cam_merge (irn_amd/csrc/label.hip) at the launch shapes of production and at the extremes of
the bounded maximum search, bit for bit against the oracle (which tests/test_label_cases_cpu.py pins on torch for these
very inputs): peaks in corner cells, in the last row / column and in the part the crop removes, plateaus, hot pixels in
noise, subnormal and huge magnitudes, negative and all-zero maps (NaN scores), partial 4-pixel groups on unaligned
planes; batches of 256 and 4097 images, where the threads of the maximum passes stride over several cells; an image large
enough for the argmax pass to stride; refusals that must leave the outputs untouched."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import irn_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _label_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = LC.label_cases()
MERGE = LC.merge_cases()


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _run_prefilled(cases):
    """irn_label_epilogue on caller-owned outputs filled with 0xA5 bytes beforehand: a pixel the kernel does not write keeps
    that pattern, whatever an earlier call left in the allocator's blocks.  Same result layout as `_run`."""
    from irn_amd._lib import _stream, check, i32_array, lib, ptr_array
    assert len({float(c[3]) for c in cases}) == 1
    rws = [_t(c[0]).reshape(c[0].shape[0], c[0].shape[-2], c[0].shape[-1]) for c in cases]
    keys = [_t(c[2]) for c in cases]
    cs, hs, ws = ([r.shape[i] for r in rws] for i in range(3))
    ohs, ows = [c[1][0] for c in cases], [c[1][1] for c in cases]

    def filled(shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return torch.full((n,), 0xA5, dtype=torch.uint8, device=_dev()).view(dtype).view(shape)

    out = {"labels": [filled((oh, ow), torch.uint8) for oh, ow in zip(ohs, ows)],
           "argmax": [filled((oh, ow), torch.int32) for oh, ow in zip(ohs, ows)],
           "rw_up": [filled((c, oh, ow), torch.float32) for c, oh, ow in zip(cs, ohs, ows)]}
    scratch = torch.empty(max(len(cases), 64), dtype=torch.int32, device=_dev())
    check(lib.irn_label_epilogue(len(cases), ptr_array([r.data_ptr() for r in rws]), i32_array(cs), i32_array(hs), i32_array(ws),
                                 i32_array(ohs), i32_array(ows), float(cases[0][3]), ptr_array([k.data_ptr() for k in keys]),
                                 ptr_array([t.data_ptr() for t in out["labels"]]), ptr_array([t.data_ptr() for t in out["argmax"]]),
                                 ptr_array([t.data_ptr() for t in out["rw_up"]]), scratch.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return out


def _run(cases, packed=False):
    from irn_amd import ops
    assert len({float(c[3]) for c in cases}) == 1
    return ops.label_epilogue([_t(c[0]) for c in cases], [c[1] for c in cases], cases[0][3], keys=[_t(c[2]) for c in cases],
                              want_argmax=True, want_rw_up=True, packed=packed)


def _host(out, j):
    return out["rw_up"][j].cpu().numpy(), out["labels"][j].cpu().numpy(), out["argmax"][j].cpu().numpy()


def _assert_equals_oracle(got, ref, what):
    (g_up, g_lab, g_idx), (up, lab, idx) = got, ref
    assert g_up.shape == up.shape and g_lab.shape == lab.shape and g_idx.shape == idx.shape, what
    assert np.array_equal(g_up, up, equal_nan=True), what
    assert np.array_equal(g_idx, idx), what
    assert np.array_equal(g_lab, lab), what
    if up.max() == 1.0:                                 # the bounded search found the very float the full evaluation finds
        assert g_up.max() == 1.0, what


def _assert_same(a, b, ja, jb, what):
    for key in ("rw_up", "labels", "argmax"):
        x, y = a[key][ja], b[key][jb]
        assert x.shape == y.shape and torch.equal(x, y), (what, key)


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_case_vs_oracle(name, case):
    rw, size, keys, bg = case
    _assert_equals_oracle(_host(_run([case]), 0), O.sem_seg_epilogue(rw, size, keys, bg), name)


def test_all_zero_map_gets_the_first_class_as_the_reference_does():
    rw, size, keys, bg = dict(CASES)["all_zero"]
    up, lab, idx = _host(_run([(rw, size, keys, bg)]), 0)
    assert np.isnan(up).all() and (idx == 1).all() and (lab == keys[0] + 1).all()


def test_packed_labels_on_unaligned_rows():
    """The partial-group cases as ONE call with packed labels: image i's label map starts at the sum of the sizes before
    it (9, 27, 54 ... bytes), its argmax and rw_up planes at odd multiples of 4 bytes."""
    cases = [c for _, c in LC.align_cases()]
    out = _run(cases, packed=True)
    assert any(t.data_ptr() % 4 for t in out["labels"])
    assert out["labels_flat"].numel() == sum(c[1][0] * c[1][1] for c in cases)
    flat = out["labels_flat"].cpu().numpy()
    off = 0
    for j, (rw, size, keys, bg) in enumerate(cases):
        ref = O.sem_seg_epilogue(rw, size, keys, bg)
        _assert_equals_oracle(_host(out, j), ref, "packed %d" % j)
        assert np.array_equal(flat[off:off + ref[1].size].reshape(size), ref[1]), j
        off += ref[1].size


def test_production_batch_of_256_images():
    """16 workgroups per image in the maximum passes, c*h*w up to 10 080 cells: most threads stride over several cells."""
    cases = LC.production_batch()
    out = _run(cases)
    for j, (rw, size, keys, bg) in enumerate(cases):
        _assert_equals_oracle(_host(out, j), O.sem_seg_epilogue(rw, size, keys, bg), "image %d" % j)
    for j, case in enumerate(cases):
        _assert_same(out, _run([case]), j, 0, "image %d alone" % j)


def test_batch_of_4097_tiny_images():
    """More images than the 4096 workgroups of a maximum pass: one workgroup per image."""
    from irn_amd import ops
    rws, sizes, keys = LC.tiny_batch()
    n = len(sizes)
    dev_rws, dev_keys = _t(rws), _t(keys)
    out = ops.label_epilogue([dev_rws[i] for i in range(n)], sizes, LC.BG, keys=[dev_keys] * n, want_argmax=True, want_rw_up=True)
    forced = [0, 1, 4095, n - 2, n - 1]
    sample = sorted(forced + [int(i) for i in np.random.RandomState(3).permutation(n) if i not in forced][:59])
    assert len(sample) == 64
    for i in sample:
        _assert_equals_oracle(_host(out, i), O.sem_seg_epilogue(rws[i], sizes[i], keys, LC.BG), "image %d" % i)
    for i in sample[::4]:
        _assert_same(out, _run([(rws[i], sizes[i], keys, LC.BG)]), i, 0, "image %d alone" % i)


@functools.lru_cache(maxsize=None)
def _big(out_w):
    case = LC.big_case(out_w)
    return case, O.sem_seg_epilogue(*case)


@pytest.mark.parametrize("out_w", [528, 527])
def test_argmax_pass_second_iteration(out_w):
    """549 120 (548 080) pixels in 4-pixel groups exceed 512 workgroups x 256 threads: output rows >= 993 are written by a
    thread's second iteration, and hold the global maximum and a label region of their own.  Run on pre-filled outputs
    (an unwritten row cannot pass) and through the wrapper."""
    case, ref = _big(out_w)
    assert (ref[1][993:] == case[2][2] + 1).any() and ref[0][:, 993:].max() == 1.0 and ref[0][:, :993].max() < 1.0
    _assert_equals_oracle(_host(_run_prefilled([case]), 0), ref, "out_w %d, pre-filled" % out_w)
    _assert_equals_oracle(_host(_run([case]), 0), ref, "out_w %d" % out_w)


def test_mixed_batch_equals_single_calls():
    """The widest output, the most source cells and the smallest image come from different jobs of one call."""
    cases = LC.mixed_batch()
    for out in (_run_prefilled(cases), _run(cases)):
        _assert_equals_oracle(_host(out, 0), _big(528)[1], "big")
        for j, case in enumerate(cases):
            if j:
                _assert_equals_oracle(_host(out, j), O.sem_seg_epilogue(*case), j)
            _assert_same(out, _run_prefilled([case]), j, 0, "image %d alone" % j)


def test_refusals_write_nothing():
    """out_h > 4h, and labels without keys: the call fails before anything is launched, also for the valid image in front."""
    from irn_amd import ops
    from irn_amd._lib import IrnHipError, _stream, check, i32_array, lib, ptr_array
    good, bad = CASES[0][1], dict(CASES)["hot_seed0"]
    c, h, w = [good[0].shape[0], bad[0].shape[0]], [good[0].shape[2], bad[0].shape[2]], [good[0].shape[3], bad[0].shape[3]]
    rws = [_t(good[0]), _t(bad[0])]
    keys = [_t(good[2]), _t(bad[2])]
    oh, ow = [good[1][0], 4 * h[1]], [good[1][1], 4 * w[1]]
    bufs = {"labels": [torch.full((oh[i] + 1, ow[i]), 0xCD, dtype=torch.uint8, device=_dev()) for i in range(2)],
            "argmax": [torch.full((oh[i] + 1, ow[i]), -7, dtype=torch.int32, device=_dev()) for i in range(2)],
            "rw_up": [torch.full((c[i], oh[i] + 1, ow[i]), -7.0, device=_dev()) for i in range(2)]}
    scratch = torch.zeros(64, dtype=torch.int32, device=_dev())

    def call(out_h, with_keys):
        return lib.irn_label_epilogue(2, ptr_array([r.data_ptr() for r in rws]), i32_array(c), i32_array(h), i32_array(w),
                                      i32_array(out_h), i32_array(ow), 0.25,
                                      ptr_array([k.data_ptr() for k in keys]) if with_keys else None,
                                      ptr_array([t.data_ptr() for t in bufs["labels"]]), ptr_array([t.data_ptr() for t in bufs["argmax"]]),
                                      ptr_array([t.data_ptr() for t in bufs["rw_up"]]), scratch.data_ptr(), _stream())

    with pytest.raises(IrnHipError, match="bad sizes"):
        check(call([oh[0], 4 * h[1] + 1], True))
    with pytest.raises(IrnHipError, match="without keys"):
        check(call(oh, False))
    torch.cuda.synchronize()
    assert all(bool((t == 0xCD).all()) for t in bufs["labels"]) and all(bool((t == -7).all()) for t in bufs["argmax"])
    assert all(bool((t == -7.0).all()) for t in bufs["rw_up"])
    # ... and the same buffers are filled by the call that is in order
    check(call(oh, True))
    torch.cuda.synchronize()
    assert np.array_equal(bufs["labels"][1][:oh[1]].cpu().numpy(), O.sem_seg_epilogue(bad[0], (oh[1], ow[1]), bad[2], 0.25)[1])
    assert bool((bufs["labels"][1][oh[1]:] == 0xCD).all())
    # the wrapper refuses both as well
    with pytest.raises(IrnHipError):
        ops.label_epilogue([rws[1]], [(4 * h[1] + 1, ow[1])], 0.25, keys=[keys[1]])
    with pytest.raises(ValueError):
        ops.label_epilogue([rws[1]], [(oh[1], ow[1])], 0.25)


# ---------------------------------------------------------------------------------------------------------------------
# irn_cam_merge
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,case", MERGE, ids=[n for n, _ in MERGE])
def test_cam_merge_vs_oracle(name, case):
    from irn_amd import ops
    outputs, size, label = case
    keys, lo, hi = ops.cam_merge([_t(o) for o in outputs], size, torch.from_numpy(label))
    r_keys, r_lo, r_hi = O.cam_merge(outputs, size, label)
    assert np.array_equal(keys.cpu().numpy(), r_keys)
    assert lo.shape == r_lo.shape and np.array_equal(lo.cpu().numpy(), r_lo), name
    assert hi.shape == r_hi.shape and np.array_equal(hi.cpu().numpy(), r_hi), name


def test_cam_merge_refuses_nine_scales():
    from irn_amd import ops
    from irn_amd._lib import IrnHipError
    outputs, size, label = dict(MERGE)["eight_scales"]
    with pytest.raises(IrnHipError, match="1..8 scales"):
        ops.cam_merge([_t(o) for o in outputs + outputs[:1]], size, torch.from_numpy(label))
