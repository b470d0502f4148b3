"""The references of tests/test_gpu_label_epilogue.py, checked where no GPU is needed: on every input of
tests/_label_cases.py the oracle (oracle/irn_oracle.py sem_seg_epilogue) equals, bit for bit and NaN for NaN, torch on the
CPU computing what step/make_sem_seg_labels.py:43-49 computes.  The CAM-merge inputs are only checked for what they aim at
(the oracle's cam_merge is pinned on torch by tests/golden/cam_merge.npz, not here: every merge case has a target with
H + W <= 128, see below).  The lattice restatement is checked at the dimensions the GPU test adds (d = 1, 3, 4).

One finding is pinned here.  ATen's CPU bilinear interpolation has TWO kernels: the generic one, whose arithmetic the
oracle and label.hip restate (and tests/golden pins), and a vectorised one that multiplies the four tap weights out
first; the installed torch 2.10 takes the second whenever the interpolated output has H + W <= 128 (before any crop),
whatever the memory layout or the thread count (observed by bisecting sizes, not read from its source), and its results differ from the generic kernel's in the last bits (1 .. 3 ulp, more
under cancellation).  No image of the pipeline is that small, so the project follows the generic kernel at EVERY size.
For the sources of these cases with h + w <= 32 the generic kernel is reached by padding the source on the right with
copies of its last column: every tap of the first 4w output columns then reads the same values with the same weights
(the clamped right neighbour of the last column is that column again).  The direct call is compared as well: it must
give the same argmax and labels on every case, and the same scores wherever ATen takes the generic kernel."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import irn_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _densecrf_ref as R  # noqa: E402
import _label_cases as LC  # noqa: E402

CASES = LC.label_cases()


def takes_generic_kernel(h, w):
    return 4 * h + 4 * w > 128


def torch_epilogue(rw, out_size, keys, bg_thres, generic=True):
    """The label epilogue as torch computes it on the CPU: x4 bilinear interpolation (align_corners=False), crop, division
    by torch.max, a constant background plane padded in front, torch.argmax, keys look-up.  With `generic` a small source
    is padded so that ATen interpolates it with its generic kernel (module docstring).
    Returns (scores [C,H,W] fp32, labels uint8 [H,W], argmax [H,W])."""
    oh, ow = out_size
    c, h, w = rw.shape[0], rw.shape[-2], rw.shape[-1]
    x = torch.from_numpy(rw).reshape(c, 1, h, w)
    if generic and not takes_generic_kernel(h, w):
        x = F.pad(x, (0, 32, 0, 0), mode="replicate")
    up = F.interpolate(x, scale_factor=4, mode="bilinear", align_corners=False)[:, 0, :oh, :ow]
    scores = up / torch.max(up)
    idx = torch.argmax(F.pad(scores, (0, 0, 0, 0, 1, 0), value=bg_thres), dim=0).numpy()
    lut = np.concatenate([[0], np.asarray(keys, np.int64) + 1])
    return scores.numpy(), lut[idx].astype(np.uint8), idx


def _check(case, name):
    rw, size, keys, bg = case
    up, lab, idx = O.sem_seg_epilogue(rw, size, keys, bg)
    t_up, t_lab, t_idx = torch_epilogue(rw, size, keys, bg)
    assert up.dtype == np.float32 and up.shape == t_up.shape == (rw.shape[0],) + tuple(size), name
    assert np.array_equal(up, t_up, equal_nan=True), name
    assert np.array_equal(idx, t_idx), name
    assert np.array_equal(lab, t_lab), name
    # the call exactly as the step makes it
    d_up, d_lab, d_idx = torch_epilogue(rw, size, keys, bg, generic=False)
    assert np.array_equal(idx, d_idx) and np.array_equal(lab, d_lab), name
    if takes_generic_kernel(*rw.shape[-2:]):
        assert np.array_equal(up, d_up, equal_nan=True), name
    return t_up, t_lab, t_idx


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_oracle_epilogue_equals_torch_cpu(name, case):
    _check(case, name)


def test_all_zero_map_is_labelled_by_the_first_class():
    """0 / 0 = NaN in every channel, and torch.argmax takes a NaN for the maximum: the reference labels an all-zero score
    map keys[0] + 1 everywhere, not background."""
    case = dict(CASES)["all_zero"]
    up, lab, idx = _check(case, "all_zero")
    print("all-zero score map: the reference writes label %s (keys %s), argmax %s" % (np.unique(lab).tolist(), case[2].tolist(), np.unique(idx).tolist()))
    assert np.isnan(up).all()
    assert (idx == 1).all() and (lab == case[2][0] + 1).all()


def test_cases_reach_what_they_aim_at():
    """The builders' own claims: a crop that loses the peak lowers the maximum, the scaled maps are subnormal / huge."""
    d = dict(CASES)
    for y, x in ((31, 31), (31, 5), (5, 31)):
        rw = d["cropped_at_%d_%d_to_121x121" % (y, x)][0]
        full = O.upsample_bilinear(rw, 4).max()
        for size in ((121, 121), (123, 123)):
            assert O.upsample_bilinear(rw, 4, size).max() < full, (y, x, size)
    tiny = d["magnitude_1e-38_seed0"][0]
    assert (tiny[tiny > 0] < np.finfo(np.float32).tiny).mean() > 0.5 and tiny.max() > 0
    assert d["magnitude_1e+30_seed0"][0].max() > 1e31 and np.isfinite(d["magnitude_1e+30_seed0"][0]).all()
    assert d["sign_all_negative"][0].max() < 0 and d["sign_mixed"][0].min() < 0 < d["sign_mixed"][0].max()
    for _, (rw, (oh, ow), _, _) in LC.align_cases():
        assert (rw.shape[0] * oh * ow) % 2 == ow % 2 and (oh * ow) % 4 != 0


def test_no_output_exceeds_the_largest_corner_of_its_cell():
    """What the bounded maximum search of label.hip rests on, on every input of this file: an interpolated value is never
    above the largest of the four source values it is taken from, rounding included (so the search's margin is idle)."""
    batch = LC.tiny_batch()
    inputs = [c[0] for _, c in CASES] + [c[0] for c in LC.production_batch()[::16]] + [LC.big_case()[0]] + list(batch[0][:64])
    for rw in inputs:
        x = rw.reshape(rw.shape[0], rw.shape[-2], rw.shape[-1])
        h, w = x.shape[1:]
        y0, y1, _, _ = O._bilinear_axis(h, 4 * h, 4)
        x0, x1, _, _ = O._bilinear_axis(w, 4 * w, 4)
        corners = [x[:, ya][:, :, xa] for ya in (y0, y1) for xa in (x0, x1)]
        assert (O.upsample_bilinear(rw, 4) <= np.maximum.reduce(corners)).all(), rw.shape


def test_batches_equal_torch_cpu_on_a_sample():
    prod = LC.production_batch()
    assert len(prod) == 256 and {c[0].shape[0] for c in prod} == set(range(1, 8))
    for i in range(0, 256, 37):
        _check(prod[i], "production %d" % i)
    rws, sizes, keys = LC.tiny_batch()
    assert rws.shape == (4097, 2, 1, 8, 8)
    for i in (0, 2048, 4096):
        _check((rws[i], sizes[i], keys, LC.BG), "tiny %d" % i)
    for i, case in enumerate(LC.mixed_batch()[1:]):
        _check(case, "mixed %d" % i)


@pytest.mark.parametrize("out_w", [528, 527])
def test_big_case_equals_torch_cpu_and_needs_the_second_iteration(out_w):
    case = LC.big_case(out_w)
    up, lab, idx = _check(case, "big")
    first = 4 * 256 * 512 // (4 * ((out_w + 3) // 4)) + 1          # first output row only the second iteration reaches
    assert first == 993
    y, x = np.unravel_index(np.argmax(up.max(axis=0)), up.shape[1:])
    assert y >= first and up[:, y, x].max() == 1.0
    assert (lab[first:] == case[2][2] + 1).sum() > 1000 and (lab[:first] == case[2][0] + 1).sum() > 1000
    assert not (lab[:first] == case[2][2] + 1).any()


# ---------------------------------------------------------------------------------------------------------------------
# CAM merge
# ---------------------------------------------------------------------------------------------------------------------

MERGE = LC.merge_cases()


def test_merge_cases_reach_what_they_aim_at():
    d = dict(MERGE)
    outputs, size, label = d["max_in_cropped_margin"]
    full = sum(O.resize_bilinear(o, (32, 32)) for o in outputs)
    assert full[5, :17, :18].max() < 0.5 * full[5].max() and full[8, :17, :18].max() < 0.5 * full[8].max()
    _, lo, hi = O.cam_merge(*d["zero_and_negative_channels"])
    assert not lo[0].any() and not hi[0].any()                     # 0 / 1e-5
    assert lo[1].min() > 0.99 and hi[1].min() > 0.99               # negative / (negative maximum + 1e-5) >= ~1
    assert len(d["eight_scales"][0]) == 8


# ---------------------------------------------------------------------------------------------------------------------
# the lattice restatement at d = 1, 3, 4
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 37, 3072])
@pytest.mark.parametrize("d", [1, 3, 4])
def test_lattice_restatement_handles_d(d, n):
    lat = R.Lattice(R.random_features(n, d))
    assert lat.keys.shape == (lat.m, d) and lat.nbr.shape == (d + 1, lat.m, 2) and lat.offset.shape == (n, d + 1)
    assert (lat.bary >= -1e-6).all() and np.allclose(lat.bary.sum(1), 1.0, atol=1e-5)
    assert (lat.full_keys.sum(axis=2) == 0).all()
    for r in range(d + 1):
        assert ((lat.full_keys[:, r, :] - r) % (d + 1) == 0).all()
    assert lat.m == len({tuple(k) for k in lat.keys.tolist()})
    assert np.array_equal(lat.keys[lat.offset.reshape(-1)], lat.full_keys[:, :, :d].reshape(-1, d))
    for j in range(d + 1):
        n1 = lat.nbr[j, :, 0]
        ok = n1 >= 0
        assert np.array_equal(lat.nbr[j, n1[ok], 1], np.nonzero(ok)[0])
    assert (lat.compute(np.ones((n, 1))) > 0).all()
