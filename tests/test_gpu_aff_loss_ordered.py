"""The ordered backward of the fused loss (irn_aff_loss_backward_ordered, `affinity_displacement_sums(..., ordered=True)`) on
the GPU: identical bits from call to call, every cell written, an image's gradients independent of its batch, and the values
against the fp64 restatement (tests/_aff_loss_ref.py).

Tolerances are those of tests/test_gpu_aff_loss.py, whose helpers and recorded constants this file uses: the bar of a
gradient is FACTOR = 4 times the distance of the COMPOSED fp32 path from the restatement on the same inputs — recorded
there for the shapes that file runs (`COMPOSED_GRAD_ABS`, `GENERIC_GRAD_ABS`, the `*_CELL_C` constants), measured in the same
run with its `_composed` / `composed_cell_c` for the shape and the edge maps that only this file runs.  The factor covers a
different summation order and nothing else; no bar is derived from the kernel under test.  The ordered and the atomic
backward each lie within the bar of the restatement, and are also required to lie within it of each other.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _aff_loss_ref as R  # noqa: E402
import test_gpu_aff_loss as T  # noqa: E402

pytestmark = pytest.mark.gpu

# (radius, batch, hp, wp): 3x3 sources; tile seams in both axes; close to the smallest radius-10 grid; a generic radius with a
# source rectangle of exactly one tile; a radius-10 grid with seams in both axes, 5 x 3 output tiles per image
SHAPES = ((5, 2, 7, 11), (5, 3, 33, 47), (10, 1, 12, 21), (3, 1, 10, 36), (10, 2, 40, 70))
IDS = lambda s: "r%d_b%d_%dx%d" % s  # noqa: E731
FACTOR = T.FACTOR


def _dev():
    return torch.device("cuda", 0)


def _inputs(shape):
    radius, batch, hp, wp = shape
    return R.make_inputs(radius, batch, hp, wp, seed=100 * radius + hp, block=2 if hp < 16 else 4)


def _autograd(inputs, radius, ordered, coef=None):
    """Gradients of the total loss (or of `(coef * sums).sum()`) through the operator, as numpy."""
    from irn_amd.misc import indexing
    edge, dp, label = inputs
    e = torch.from_numpy(edge).to(_dev()).requires_grad_(True)
    d = torch.from_numpy(dp).to(_dev()).requires_grad_(True)
    sums, counts = indexing.affinity_displacement_sums(e, d, torch.from_numpy(label).to(_dev()), radius, ordered=ordered)
    T._backward(sums, counts, coef)
    return {"sums": sums.detach().cpu().numpy(), "counts": counts.cpu().numpy(),
            "grad_edge": e.grad.cpu().numpy(), "grad_dp": d.grad.cpu().numpy()}


def _entry(inputs, radius, coef, entry="irn_aff_loss_backward_ordered"):
    """The C entry itself on outputs filled with NaN beforehand: (grad_edge, grad_dp) as device tensors."""
    from irn_amd._lib import _stream, check, lib
    edge, dp, label = (torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) for a in inputs)
    b, hp, wp = label.shape
    need = lib.irn_aff_loss_workspace_bytes(b, hp, wp, radius)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())
    co = torch.as_tensor(np.asarray(coef, np.float32), device=_dev())
    ge, gd = torch.full_like(edge, float("nan")), torch.full_like(dp, float("nan"))
    check(getattr(lib, entry)(edge.data_ptr(), dp.data_ptr(), label.data_ptr(), b, hp, wp, radius, 21, co.data_ptr(),
                              ge.data_ptr(), gd.data_ptr(), ws.data_ptr(), C.c_size_t(need), _stream()))
    torch.cuda.synchronize()
    return ge, gd


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, the fp64 restatement (once per shape), the coefficients of the total loss, and both backwards."""
    inputs = _inputs(shape)
    ref = R.reference(*inputs, shape[0])
    return inputs, ref, R.total_loss_coefficients(ref["counts"]), _autograd(inputs, shape[0], True), _autograd(inputs, shape[0], False)


def _recorded_or_measured(shape):
    """The composed path's max-abs distance (grad_edge, grad_dp) from the restatement: what test_gpu_aff_loss.py records for
    the shape, else measured now on the same inputs the way its `composed_errors` does."""
    inputs, ref, _, _, _ = _case(shape)
    _, c_ge, c_gd = T._errors(T._composed(*inputs, shape[0]), ref)
    for table in (T.COMPOSED_GRAD_ABS, T.GENERIC_GRAD_ABS):
        if shape in table:
            return table[shape], (c_ge, c_gd), "recorded"
    return (c_ge, c_gd), (c_ge, c_gd), "measured in this run"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_five_calls_give_the_same_bits_and_write_every_cell(shape):
    inputs, _, coef, _, _ = _case(shape)
    first = _entry(inputs, shape[0], coef)
    assert not torch.isnan(first[0]).any() and not torch.isnan(first[1]).any(), "a cell was left unwritten"
    for _ in range(4):
        again = _entry(inputs, shape[0], coef)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    assert first[0].abs().max() > 0 and first[1].abs().max() > 0


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] > 1], ids=IDS)
def test_an_images_gradients_do_not_depend_on_its_batch(shape):
    inputs, _, coef, _, _ = _case(shape)
    ge, gd = _entry(inputs, shape[0], coef)
    for i in range(shape[1]):
        one = tuple(a[i:i + 1] for a in inputs)
        ge1, gd1 = _entry(one, shape[0], coef)                            # the same coefficients in both calls
        assert torch.equal(ge1[0], ge[i]) and torch.equal(gd1[0], gd[i]), "image %d" % i


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gradients_vs_restatement_and_vs_the_atomic_backward(shape):
    inputs, ref, _, got, atomic = _case(shape)
    assert (ref["counts"] > 0).all(), "the inputs must exercise all three pair classes"
    assert np.array_equal(got["counts"], ref["counts"]) and got["sums"].tobytes() == atomic["sums"].tobytes()
    (b_ge, b_gd), (c_ge, c_gd), origin = _recorded_or_measured(shape)
    _, ge, gd = T._errors(got, ref)
    _, a_ge, a_gd = T._errors(atomic, ref)
    d_ge = float(np.abs(got["grad_edge"] - atomic["grad_edge"]).max())
    d_gd = float(np.abs(got["grad_dp"] - atomic["grad_dp"]).max())
    print("\nshape %s (grad_edge, grad_dp)\n  ordered  vs restatement %.3e %.3e\n  atomic   vs restatement %.3e %.3e\n"
          "  ordered  vs atomic      %.3e %.3e\n  composed vs restatement %.3e %.3e (this run); bar = %g x %.3e %.3e (%s)"
          % (shape, ge, gd, a_ge, a_gd, d_ge, d_gd, c_ge, c_gd, FACTOR, b_ge, b_gd, origin))
    assert np.isfinite(got["grad_edge"]).all() and np.isfinite(got["grad_dp"]).all()
    assert ge <= FACTOR * b_ge, "grad_edge: max-abs error %.3e, bound %.3e" % (ge, FACTOR * b_ge)
    assert gd <= FACTOR * b_gd, "grad_dp: max-abs error %.3e, bound %.3e" % (gd, FACTOR * b_gd)
    assert d_ge <= FACTOR * b_ge, "grad_edge: ordered - atomic %.3e, bound %.3e" % (d_ge, FACTOR * b_ge)
    assert d_gd <= FACTOR * b_gd, "grad_dp: ordered - atomic %.3e, bound %.3e" % (d_gd, FACTOR * b_gd)


def _tie_inputs(shape, levels):
    """Every label 0 (every pair a bg pair); the edge constant (one level: every path one long tie) or drawn from two levels
    (most paths have several cells at their maximum, and the first of them is rarely the path's first cell)."""
    edge, dp, label = T._constant_edge_inputs(shape)
    if levels == 2:
        edge = np.random.RandomState(7 + shape[2]).choice(np.asarray([0.25, 0.75], np.float32), edge.shape)
    return edge, dp, label


@pytest.mark.parametrize("levels", (1, 2), ids=("constant", "two_level"))
@pytest.mark.parametrize("shape", T.TIE_SHAPES, ids=IDS)
def test_tied_path_maxima_send_the_gradient_to_the_first_table_cell(shape, levels):
    inputs = _tie_inputs(shape, levels)
    ref = R.reference(*inputs, shape[0], fp32_constants=True)
    got = _autograd(inputs, shape[0], True)
    assert np.array_equal(got["counts"], ref["counts"]) and ref["counts"][0] > 0 and (ref["counts"][1:] == 0).all()
    mags = T._total_loss_magnitudes(inputs, ref, shape[0])
    composed = T.composed_cell_c(inputs, shape[0], ref, mags)
    # the constant map is the existing tie test's, with its recorded figure; the two-level map is measured here
    recorded = T.TIE_CELL_C[shape] if levels == 1 else composed
    support, want = got["grad_edge"] != 0, ref["grad_edge"] != 0
    print("\nshape %s, %d level(s): cells with a gradient %d (restatement %d), differing %d; composed cell c %.3f %.3f (this run)"
          % ((shape, levels, int(support.sum()), int(want.sum()), int((support != want).sum())) + composed))
    assert want.any() and not want.all()
    assert np.array_equal(support, want), "the affinity gradient of a tied path lands on other cells than its first table cell"
    T._assert_cells(got, ref, mags, recorded, "%d-level edge" % levels)


def test_each_coefficient_on_its_own_and_an_all_ignore_map():
    shape = R.COEFFICIENT_SHAPE
    radius = shape[0]
    inputs = T._inputs_at(shape, "degenerate")
    print()
    for i in range(5):
        coef = np.eye(5)[i]
        ref = R.reference(*inputs, radius, fp32_constants=True, coef=coef)
        got = _autograd(inputs, radius, True, coef=coef)
        mags = R.addend_magnitudes(*inputs, radius, coef, fp32_constants=True)
        assert mags[0].any() == (i < 3) and mags[1].any() == (i >= 3)      # the log terms reach edge only, the others dp only
        T._assert_cells(got, ref, mags, T.COEFFICIENT_CELL_C, "sums[%d]" % i)
    # nothing counts: exact zeros in every cell, written over the NaNs, whatever the coefficients
    edge, dp, label = inputs
    ge, gd = _entry((edge, dp, np.full_like(label, 255)), radius, np.asarray([0.3, 0.7, 1.1, 0.5, 0.9]))
    assert (ge == 0).all() and (gd == 0).all()
    got = _autograd((edge, dp, np.full_like(label, 255)), radius, True)
    assert (got["sums"] == 0).all() and (got["counts"] == 0).all()
    assert (got["grad_edge"] == 0).all() and (got["grad_dp"] == 0).all()
