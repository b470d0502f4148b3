"""The fused affinity / displacement loss (irn_amd/csrc/aff_loss.hip, `indexing.affinity_displacement_sums`,
`AffinityDisplacementLoss.fused_losses`) and the training step built on it, on the GPU.

Tolerances.  Counts are exact.  Sums and gradients are compared with the fp64 restatement (tests/_aff_loss_ref.py); the
bound is not invented: `COMPOSED_SUM_REL` / `COMPOSED_GRAD_ABS` record how far the COMPOSED fp32 path (the operators and arithmetic of
`AffinityDisplacementLoss.forward` plus masked `torch.sum`, as they exist without the fused pass) is from the same
restatement on the same inputs — the worst relative error of each of the five sums over the shapes, and per shape the
max-abs error of the two gradient maps of the total loss.  The fused pass is allowed 4x that: the factor covers a different summation order and
nothing more.  Every test prints what it measured before it asserts.

The second half of the file runs the table-driven radii and the tile seams on two input families.  On the "degenerate"
family (quantised edges, integer displacements, labels on both sides of the ignore threshold) the restatement takes 1e-5
and 1 + 1e-5 at their fp32 values, and gradients are bounded per cell: c * eps * the sum of the |addends| of the cell, c
again 4x what the composed path needs (DEGENERATE_CELL_C and its neighbours), and exactly 0 where no addend arrives.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _aff_loss_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# (radius, batch, hp, wp): smallest legal grid (3x3 sources), no tile multiple, smallest legal grid, the training shape
SHAPES = ((5, 2, 7, 11), (5, 3, 33, 47), (10, 1, 12, 21), (10, 2, 128, 128))

# Measured on an MI355X with `composed_errors` below (inputs as in `_case`): the composed fp32 path against the fp64 restatement.
# Relative error of sums[0..4], the worst over the four shapes (per shape: 3.3e-8 5.6e-9 1.9e-8 3.9e-8 1.1e-7 / 5.8e-8 4.7e-8
# 8.6e-8 8.2e-8 1.4e-8 / 8.5e-8 3.7e-8 1.4e-7 1.9e-8 8.5e-9 / 9.3e-9 3.3e-8 1.2e-7 7.8e-8 7.4e-8):
COMPOSED_SUM_REL = (8.473e-08, 4.727e-08, 1.443e-07, 8.231e-08, 1.107e-07)
# max-abs error of (grad_edge, grad_dp) of the total loss; gradients scale with 1 / pair count, so per shape:
COMPOSED_GRAD_ABS = {
    (5, 2, 7, 11): (2.681e-06, 1.637e-08),
    (5, 3, 33, 47): (1.323e-07, 3.623e-10),
    (10, 1, 12, 21): (1.654e-05, 7.115e-08),
    (10, 2, 128, 128): (3.757e-07, 1.790e-10),
}
# (the fused pass measured in the same run: sums 6.2e-8 6.8e-8 2.0e-7 3.0e-9 1.5e-9 at worst; grad_edge equal to the composed
# path's figure to three digits at every shape, grad_dp 8.9e-9 / 1.2e-10 / 7.1e-8 / 4.2e-11)
FACTOR = 4.0


def _dev():
    return torch.device("cuda", 0)


def _backward(sums, counts, coef):
    """Back-propagate the total loss, or `(coef * sums).sum()` where five coefficients are given (as `R.reference`)."""
    if coef is None:
        R.total_loss(sums, counts).backward()
    else:
        (sums * torch.as_tensor(np.asarray(coef), dtype=sums.dtype, device=sums.device)).sum().backward()


def _fused(edge, dp, label, radius, backward=True, coef=None):
    from irn_amd.misc import indexing
    e = torch.from_numpy(edge).to(_dev()).requires_grad_(backward)
    d = torch.from_numpy(dp).to(_dev()).requires_grad_(backward)
    sums, counts = indexing.affinity_displacement_sums(e, d, torch.from_numpy(label).to(_dev()), radius)
    out = {"sums": sums.detach().cpu().numpy(), "counts": counts.cpu().numpy()}
    if backward:
        _backward(sums, counts, coef)
        out["grad_edge"], out["grad_dp"] = e.grad.cpu().numpy(), d.grad.cpu().numpy()
    out["losses"] = np.asarray([float(v) for v in R.losses(sums.detach(), counts)])
    return out


def _composed(edge, dp, label, radius, coef=None):
    e = torch.from_numpy(edge).to(_dev()).requires_grad_(True)
    d = torch.from_numpy(dp).to(_dev()).requires_grad_(True)
    sums, counts = R.composed_sums(e, d, torch.from_numpy(label).to(_dev()), radius)
    _backward(sums, counts, coef)
    return {"sums": sums.detach().cpu().numpy().astype(np.float64), "grad_edge": e.grad.cpu().numpy(), "grad_dp": d.grad.cpu().numpy()}


def _errors(got, ref):
    rel = tuple(float(abs(got["sums"][i] - ref["sums"][i]) / abs(ref["sums"][i])) for i in range(5))
    return rel, float(np.abs(got["grad_edge"] - ref["grad_edge"]).max()), float(np.abs(got["grad_dp"] - ref["grad_dp"]).max())


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, the fp64 restatement (computed once per shape) and the fused result."""
    radius, batch, hp, wp = shape
    edge, dp, label = R.make_inputs(radius, batch, hp, wp, seed=100 * radius + hp, block=2 if hp < 16 else 4)
    return (edge, dp, label), R.reference(edge, dp, label, radius), _fused(edge, dp, label, radius)


def composed_errors(shape):
    """What the constants above record (run this file with -s to see the figures)."""
    (edge, dp, label), ref, _ = _case(shape)
    return _errors(_composed(edge, dp, label, shape[0]), ref)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d_b%d_%dx%d" % s)
def test_counts_sums_and_gradients_vs_restatement(shape):
    _, ref, got = _case(shape)
    assert (ref["counts"] > 0).all(), "the inputs must exercise all three pair classes"
    assert np.array_equal(got["counts"], ref["counts"])
    rel, ge, gd = _errors(got, ref)
    c_rel, c_ge, c_gd = composed_errors(shape)
    print("\nshape %s\n  fused    rel(sums) %s grad_edge %.3e grad_dp %.3e\n  composed rel(sums) %s grad_edge %.3e grad_dp %.3e"
          % (shape, " ".join("%.3e" % v for v in rel), ge, gd, " ".join("%.3e" % v for v in c_rel), c_ge, c_gd))
    b_rel, (b_ge, b_gd) = COMPOSED_SUM_REL, COMPOSED_GRAD_ABS[shape]
    for i in range(5):
        assert rel[i] <= FACTOR * b_rel[i], "sums[%d]: relative error %.3e, bound %.3e" % (i, rel[i], FACTOR * b_rel[i])
    assert ge <= FACTOR * b_ge, "grad_edge: max-abs error %.3e, bound %.3e" % (ge, FACTOR * b_ge)
    assert gd <= FACTOR * b_gd, "grad_dp: max-abs error %.3e, bound %.3e" % (gd, FACTOR * b_gd)
    assert np.isfinite(got["grad_edge"]).all() and np.isfinite(got["grad_dp"]).all()


# ------------------------------------------------------------------------------------------------
# generic radii, tile seams, tied maxima, saturated edges, zero residuals, the ignore threshold
# ------------------------------------------------------------------------------------------------
# The eight shapes of R.GENERIC_AND_SEAM_SHAPES, each on two input families: "random" (`R.make_inputs`, as above) and
# "degenerate" (`R.make_degenerate_inputs`: quantised edges, integer displacements, labels on both sides of the ignore
# threshold).  The constants are again the COMPOSED fp32 path against the fp64 restatement, measured on an MI355X with
# `composed_errors_at` / `composed_cell_c`; on the degenerate family the restatement takes 1e-5 and 1 + 1e-5 at their fp32
# values (`fp32_constants=True`): where an edge saturates, 1.00001f - 1.0f = 1.00136e-5 is the whole term, and against the
# exact constants the composed path's sums[2] is off by the relative error given in the last comment line of each block.
#
# random family: relative error of sums[0..4], the worst over the eight shapes (per shape, in the order of the table:
# 6.0e-8 2.2e-8 5.1e-8 3.1e-8 9.1e-9 / 6.7e-8 4.7e-8 2.3e-7 3.5e-8 1.2e-8 / 8.2e-10 3.8e-8 2.8e-8 5.1e-8 5.1e-8 / 8.0e-9
# 1.0e-7 1.1e-7 2.5e-9 6.4e-8 / 8.0e-8 1.6e-8 1.3e-7 1.8e-9 8.1e-9 / 6.4e-9 3.9e-8 2.2e-8 5.0e-8 1.1e-8 / 2.4e-9 7.0e-8
# 1.5e-7 2.4e-8 9.7e-9 / 9.6e-9 5.3e-8 1.4e-7 2.2e-8 6.0e-8):
GENERIC_SUM_REL = (8.026e-08, 9.959e-08, 2.287e-07, 5.108e-08, 6.394e-08)
# max-abs error of (grad_edge, grad_dp) of the total loss, per shape as above:
GENERIC_GRAD_ABS = {
    (2, 2, 4, 5): (9.115e-08, 7.238e-09),
    (16, 1, 18, 33): (2.395e-05, 4.721e-08),
    (3, 2, 11, 37): (1.207e-07, 4.085e-10),
    (7, 1, 20, 50): (1.481e-06, 2.098e-09),
    (5, 1, 12, 40): (1.186e-06, 1.764e-09),
    (5, 1, 13, 41): (8.324e-07, 1.331e-09),
    (3, 1, 10, 36): (3.250e-07, 7.537e-10),
    (10, 1, 17, 50): (1.992e-05, 7.008e-09),
}
# degenerate family, restatement with the fp32 constants: relative error of sums[0..4], the worst over the eight shapes
# (the displacement sums are sums of small integers, exact on both sides; per shape:
# 4.6e-8 6.0e-8 1.1e-7 0 0 / 7.7e-9 9.4e-8 3.4e-8 0 0 / 5.1e-8 3.1e-8 4.7e-8 0 0 /
# 1.1e-7 2.4e-8 6.6e-8 0 0 / 2.1e-8 4.3e-8 2.8e-8 0 0 / 2.5e-8 2.0e-9 5.9e-8 0 0 /
# 1.5e-7 4.2e-8 5.2e-8 0 0 / 4.7e-8 3.2e-8 1.8e-8 0 0;
# against the restatement with the exact constants the worst is 1.5e-7 9.6e-8 9.5e-5 0 0):
DEGENERATE_SUM_REL = (1.473e-07, 9.371e-08, 1.063e-07, 0.0, 0.0)
# Gradients on the degenerate family are bounded per cell: |error| <= c * eps * (sum of the |addends| of that cell, from
# `R.addend_magnitudes`), and a cell without addends is exactly 0 — a global max-abs bound would be set by the c / 1e-5
# terms of saturated edges and hide a misrouted small gradient.  c of the composed path for (grad_edge, grad_dp) under the
# total loss, per shape (`composed_cell_c`; a dp figure of 0 is exact: sums of few equal small numbers):
DEGENERATE_CELL_C = {
    (2, 2, 4, 5): (0.880, 0.420),
    (16, 1, 18, 33): (7.704, 8.366),
    (3, 2, 11, 37): (6.753, 1.443),
    (7, 1, 20, 50): (28.123, 4.728),
    (5, 1, 12, 40): (6.074, 0.827),
    (5, 1, 13, 41): (19.154, 2.037),
    (3, 1, 10, 36): (3.846, 0.925),
    (10, 1, 17, 50): (70.429, 10.616),
}
# ... at R.COEFFICIENT_SHAPE, the worst over the five unit coefficients and the all-ones coefficients (per case:
# 2.20 0.00 / 0.65 0.00 / 6.67 0.00 / 0.00 0.00 / 0.00 0.00 / 2.31 0.00):
COEFFICIENT_CELL_C = (6.666, 0.000)
# ... and on the two constant-edge grids of the tie test:
TIE_CELL_C = {
    (5, 1, 13, 41): (1.382, 6.877),
    (3, 1, 10, 36): (0.704, 1.405),
}
# (the fused pass measured in the same run: random sums 5.6e-8 5.3e-8 2.6e-7 8.8e-9 9.1e-9 at worst, grad_edge / grad_dp at
# most 1.04 / 1.00 times the composed path's figure; degenerate sums 1.4e-7 1.4e-7 3.5e-8 0 0 at worst, cell c at most
# 69.29 / 8.38)
EPS32 = float(np.finfo(np.float32).eps)
FAMILIES = ("random", "degenerate")


def _inputs_at(shape, family):
    radius, batch, hp, wp = shape
    if family == "random":
        return R.make_inputs(radius, batch, hp, wp, seed=100 * radius + hp, block=2 if hp < 16 else 4)
    return R.make_degenerate_inputs(radius, batch, hp, wp, R.DEGENERATE_SEED[shape])


@functools.lru_cache(maxsize=None)
def _case_at(shape, family):
    """Inputs, the fp64 restatement (with the fp32 constants on the degenerate family) and the fused result."""
    edge, dp, label = _inputs_at(shape, family)
    ref = R.reference(edge, dp, label, shape[0], fp32_constants=family == "degenerate")
    return (edge, dp, label), ref, _fused(edge, dp, label, shape[0])


def composed_errors_at(shape, family):
    (edge, dp, label), ref, _ = _case_at(shape, family)
    return _errors(_composed(edge, dp, label, shape[0]), ref)


def _cell_c(got, ref, mags):
    """The c of the per-cell bound that `got` needs: max over the cells of |error| / (eps * sum of |addends|), for
    (grad_edge, grad_dp); infinite if a cell without addends is not exactly 0."""
    out = []
    for name, mag in zip(("grad_edge", "grad_dp"), mags):
        err = np.abs(got[name].astype(np.float64) - ref[name])
        if (err[mag == 0] != 0).any():
            out.append(float("inf"))
        else:
            out.append(float((err[mag > 0] / (EPS32 * mag[mag > 0])).max()) if (mag > 0).any() else 0.0)
    return tuple(out)


def _assert_cells(got, ref, mags, recorded, what):
    """The per-cell bound with FACTOR * `recorded` (the composed path's c); prints the c that `got` needs first."""
    c = _cell_c(got, ref, mags)
    print("  %s: fused cell c (grad_edge, grad_dp) %.3f %.3f, composed recorded %.3f %.3f" % ((what,) + c + tuple(recorded)))
    for name, mag, need, rec in zip(("grad_edge", "grad_dp"), mags, c, recorded):
        assert np.isfinite(got[name]).all()
        assert (got[name][mag == 0] == 0).all(), "%s %s: a cell that no addend reaches is not 0" % (what, name)
        assert need <= FACTOR * rec, "%s %s: per-cell c %.3f, bound %.3f" % (what, name, need, FACTOR * rec)


def _total_loss_magnitudes(inputs, ref, radius):
    return R.addend_magnitudes(*inputs, radius, R.total_loss_coefficients(ref["counts"]), fp32_constants=True)


def composed_cell_c(inputs, radius, ref, mags, coef=None):
    """What the three CELL_C constants record: the c of the composed path, for the total loss or five coefficients."""
    return _cell_c(_composed(*inputs, radius, coef=coef), ref, mags)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", R.GENERIC_AND_SEAM_SHAPES, ids=lambda s: "r%d_b%d_%dx%d" % s)
def test_generic_radii_and_tile_seams_vs_restatement(shape, family):
    inputs, ref, got = _case_at(shape, family)
    assert (ref["counts"] > 0).all(), "the inputs must exercise all three pair classes"
    if family == "degenerate":
        tied, fg_zero, bg_zero = R.degeneracy(*inputs, shape[0])
        assert tied > 0 and fg_zero > 0 and bg_zero > 0, "the inputs must have tied path maxima and exactly-zero residuals"
    rel, ge, gd = _errors(got, ref)
    c_rel, c_ge, c_gd = composed_errors_at(shape, family)
    print("\nshape %s %s: counts %s, restatement %s\n  fused    rel(sums) %s grad_edge %.3e grad_dp %.3e\n"
          "  composed rel(sums) %s grad_edge %.3e grad_dp %.3e"
          % (shape, family, got["counts"].tolist(), ref["counts"].tolist(), " ".join("%.3e" % v for v in rel), ge, gd,
             " ".join("%.3e" % v for v in c_rel), c_ge, c_gd))
    assert np.array_equal(got["counts"], ref["counts"])
    b_rel = GENERIC_SUM_REL if family == "random" else DEGENERATE_SUM_REL
    for i in range(5):
        assert rel[i] <= FACTOR * b_rel[i], "sums[%d]: relative error %.3e, bound %.3e" % (i, rel[i], FACTOR * b_rel[i])
    assert np.isfinite(got["grad_edge"]).all() and np.isfinite(got["grad_dp"]).all()
    if family == "random":
        b_ge, b_gd = GENERIC_GRAD_ABS[shape]
        assert ge <= FACTOR * b_ge, "grad_edge: max-abs error %.3e, bound %.3e" % (ge, FACTOR * b_ge)
        assert gd <= FACTOR * b_gd, "grad_dp: max-abs error %.3e, bound %.3e" % (gd, FACTOR * b_gd)
    else:
        mags = _total_loss_magnitudes(inputs, ref, shape[0])
        print("  composed cell c (grad_edge, grad_dp) %.3f %.3f" % composed_cell_c(inputs, shape[0], ref, mags))
        _assert_cells(got, ref, mags, DEGENERATE_CELL_C[shape], "total loss")


def _constant_edge_inputs(shape):
    """Every label 0 and the edge constant: every path is one long tie, every pair a bg pair."""
    radius, batch, hp, wp = shape
    _, dp, _ = R.make_degenerate_inputs(radius, batch, hp, wp, R.DEGENERATE_SEED[shape])
    return np.full((batch, hp, wp), 0.5, np.float32), dp, np.zeros((batch, hp, wp), np.uint8)


TIE_SHAPES = ((5, 1, 13, 41), (3, 1, 10, 36))


@pytest.mark.parametrize("shape", TIE_SHAPES, ids=lambda s: "r%d_b%d_%dx%d" % s)
def test_tied_path_maxima_send_the_gradient_to_the_first_table_cell(shape):
    inputs = _constant_edge_inputs(shape)
    ref = R.reference(*inputs, shape[0], fp32_constants=True)
    got = _fused(*inputs, shape[0])
    assert np.array_equal(got["counts"], ref["counts"]) and ref["counts"][0] > 0 and (ref["counts"][1:] == 0).all()
    support, want = got["grad_edge"] != 0, ref["grad_edge"] != 0
    mags = _total_loss_magnitudes(inputs, ref, shape[0])
    print("\nshape %s: cells with a gradient %d (restatement %d), differing %d; composed cell c %.3f %.3f"
          % ((shape, int(support.sum()), int(want.sum()), int((support != want).sum()))
             + composed_cell_c(inputs, shape[0], ref, mags)))
    assert want.any() and not want.all()
    assert np.array_equal(support, want), "the affinity gradient of a tied path lands on other cells than its first table cell"
    _assert_cells(got, ref, mags, TIE_CELL_C[shape], "constant edge")


def test_each_coefficient_on_its_own():
    """`sums[i].backward()` for each i against the restatement's gradient of sums[i], and the five add up to the gradient of
    `sums.sum()`: each result is within its per-cell bound B_i of the restatement's, the magnitudes (so the bounds) of the five
    add up to those of the all-ones coefficients, and the restatement's five gradients add up to its sixth exactly — so the
    sum of the five (formed in fp64) is within twice the all-ones bound of the all-ones result."""
    shape = R.COEFFICIENT_SHAPE
    radius = shape[0]
    inputs = _inputs_at(shape, "degenerate")
    assert (R.reference(*inputs, radius)["counts"] > 0).all()
    total = {"grad_edge": 0.0, "grad_dp": 0.0}
    print()
    for i in range(5):
        coef = np.eye(5)[i]
        ref = R.reference(*inputs, radius, fp32_constants=True, coef=coef)
        got = _fused(*inputs, radius, coef=coef)
        mags = R.addend_magnitudes(*inputs, radius, coef, fp32_constants=True)
        print("  sums[%d]: composed cell c %.3f %.3f" % ((i,) + composed_cell_c(inputs, radius, ref, mags, coef)))
        assert mags[0].any() == (i < 3) and mags[1].any() == (i >= 3)      # the log terms reach edge only, the others dp only
        _assert_cells(got, ref, mags, COEFFICIENT_CELL_C, "sums[%d]" % i)
        for name in total:
            total[name] = total[name] + got[name].astype(np.float64)
    ones = np.ones(5)
    got = _fused(*inputs, radius, coef=ones)
    mags = R.addend_magnitudes(*inputs, radius, ones, fp32_constants=True)
    ref = R.reference(*inputs, radius, fp32_constants=True, coef=ones)
    print("  sums.sum(): composed cell c %.3f %.3f" % composed_cell_c(inputs, radius, ref, mags, ones))
    _assert_cells(got, ref, mags, COEFFICIENT_CELL_C, "sums.sum()")
    for name, mag, rec in zip(("grad_edge", "grad_dp"), mags, COEFFICIENT_CELL_C):
        err = np.abs(total[name] - got[name])
        print("  %s: the five unit results against sums.sum(): worst |difference| / (eps * magnitude) %.3f"
              % (name, float((err[mag > 0] / (EPS32 * mag[mag > 0])).max())))
        assert (err <= 2 * FACTOR * rec * EPS32 * mag).all(), name


def test_wrapper_layouts_give_the_same_bits_and_bad_labels_are_refused():
    from irn_amd.misc import indexing
    shape = (3, 2, 11, 37)
    radius, batch, hp, wp = shape
    edge, dp, label = (torch.from_numpy(a).to(_dev()) for a in _inputs_at(shape, "degenerate"))
    sums, counts = indexing.affinity_displacement_sums(edge, dp, label, radius)
    assert (counts > 0).all()

    def wide(t):
        """`t` as a slice of a tensor three columns wider and one row taller: same values, other strides."""
        w = torch.full(t.shape[:-2] + (hp + 1, wp + 3), 77, dtype=t.dtype, device=t.device)
        w[..., :hp, 2:wp + 2] = t
        v = w[..., :hp, 2:wp + 2]
        assert not v.is_contiguous() and torch.equal(v, t)
        return v

    for name, args in (("[B,1,Hp,Wp] edge", (edge[:, None], dp, label)), ("strided edge", (wide(edge), dp, label)),
                       ("strided dp", (edge, wide(dp), label)), ("strided label", (edge, dp, wide(label))),
                       ("all strided", (wide(edge)[:, None], wide(dp), wide(label)))):
        s, c = indexing.affinity_displacement_sums(*args, radius)
        assert s.cpu().numpy().tobytes() == sums.cpu().numpy().tobytes() and torch.equal(c, counts), name
    for bad in (label.to(torch.int64), label.to(torch.int32), label.to(torch.float32)):
        with pytest.raises(ValueError):
            indexing.affinity_displacement_sums(edge, dp, bad, radius)
    for bad in (label[:, :, :-1], label[:, :-1], label[:1], label.reshape(batch, wp, hp), label[:, None]):
        with pytest.raises(ValueError):
            indexing.affinity_displacement_sums(edge, dp, bad, radius)


@functools.lru_cache(maxsize=None)
def _model(hp, wp):
    from irn_amd.misc import indexing
    from irn_amd.net import weights
    from irn_amd.net.resnet50_irn import AffinityDisplacementLoss
    model = AffinityDisplacementLoss(indexing.PathIndex(5, (hp, wp)))
    model.load_state_dict(weights.random_irn_state(), strict=False)
    return model.to(_dev()).train()


def test_fused_losses_agree_with_the_composed_module():
    """`fused_losses` against `forward(x, True)` + the masked sums of the training loop, on the module, at 33x47."""
    shape = SHAPES[1]
    radius, batch, hp, wp = shape
    model = _model(hp, wp)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(batch, 3, 4 * hp, 4 * wp, generator=g).to(_dev())
    label = torch.from_numpy(R.make_inputs(radius, batch, hp, wp, seed=9)[2]).to(_dev())
    fused = [float(v.detach()) for v in model.fused_losses(x, label)]
    pos_l, neg_l, fg_l, bg_l = model(x, True)          # (autograd on, like fused_losses: the same kernels in the network)
    bg, fg, neg = (torch.from_numpy(m.astype(np.float32)).to(_dev()) for m in R.batch_pair_labels(label.cpu().numpy(), model.path_index))
    sums = torch.stack([torch.sum(bg * pos_l), torch.sum(fg * pos_l), torch.sum(neg * neg_l),
                        torch.sum(fg_l * fg[:, None]), torch.sum(bg_l * bg[:, None])])
    composed = [float(v) for v in R.losses(sums.detach(), torch.stack([bg.sum(), fg.sum(), neg.sum()]))]
    print("\nfused %s\ncomposed %s" % (fused, composed))
    b_rel = COMPOSED_SUM_REL
    # each loss is a sum over a count (two of them for the first)
    bounds = (max(b_rel[0], b_rel[1]), b_rel[2], b_rel[3], b_rel[4])
    for f, c, b in zip(fused, composed, bounds):
        assert np.isfinite(f) and abs(f - c) <= FACTOR * b * abs(c), (f, c, b)


def test_degenerate_label_maps():
    radius, batch, hp, wp = SHAPES[1]
    edge, dp, label = R.make_inputs(radius, batch, hp, wp, seed=11)
    got = _fused(edge, dp, np.full_like(label, 255), radius)
    assert (got["sums"] == 0).all() and (got["counts"] == 0).all()
    assert (got["grad_edge"] == 0).all() and (got["grad_dp"] == 0).all()
    assert np.isfinite(got["losses"]).all() and (got["losses"] == 0).all()
    got = _fused(edge, dp, np.zeros_like(label), radius)
    n_pairs = batch * 34 * (hp - 4) * (wp - 8)
    assert got["counts"].tolist() == [n_pairs, 0, 0]
    assert got["sums"][0] > 0 and got["sums"][4] > 0 and (got["sums"][[1, 2, 3]] == 0).all()
    ref = R.reference(edge, dp, np.zeros_like(label), radius)
    assert np.allclose(got["sums"], ref["sums"], rtol=1e-5)       # (the tight comparison is the parametrised test's)
    assert np.abs(got["grad_edge"]).max() > 0 and np.abs(got["grad_dp"]).max() > 0


def test_forward_is_bit_reproducible():
    (edge, dp, label), _, first = _case(SHAPES[3])
    again = _fused(edge, dp, label, SHAPES[3][0], backward=False)
    assert first["sums"].tobytes() == again["sums"].tobytes() and np.array_equal(first["counts"], again["counts"])


def test_peak_memory_stays_below_one_pair_tensor():
    from irn_amd.misc import indexing
    radius, batch, hp, wp = 10, 4, 128, 128
    edge, dp, label = R.make_inputs(radius, batch, hp, wp, seed=5)
    e = torch.from_numpy(edge).to(_dev()).requires_grad_(True)
    d = torch.from_numpy(dp).to(_dev()).requires_grad_(True)
    lab = torch.from_numpy(label).to(_dev())
    one_tensor = batch * 152 * 13090 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    sums, counts = indexing.affinity_displacement_sums(e, d, lab, radius)
    R.total_loss(sums, counts).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("\nfused forward + backward: peak rise %d bytes; one [B,152,13090] fp32 tensor: %d bytes" % (rise, one_tensor))
    assert e.grad is not None and d.grad is not None
    assert rise < one_tensor


# ------------------------------------------------------------------------------------------------
# the step, end to end
# ------------------------------------------------------------------------------------------------

def _train_args(root, lst, label_dir, out):
    return ["--voc12_root", root, "--train_list", lst, "--infer_list", lst, "--ir_label_out_dir", label_dir,
            "--irn_crop_size", "96", "--irn_batch_size", "2", "--irn_num_epoches", "1", "--num_workers", "2",
            "--irn_weights_name", out, "--log_name", os.path.join(root, "log_" + os.path.basename(out)), "--train_irn_pass", "True", "--seed", "4"]


def _run_train(argv):
    import run_train
    stdout = sys.stdout
    try:
        return run_train.main(argv)["train_irn"]
    finally:
        sys.stdout = stdout                                   # run_train tees stdout into its log like run_sample


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("voc"))
    lst, label_dir = R.write_voc(root, 6)                      # six 120x140 images; crop 96 -> grid 24x24
    out = os.path.join(root, "sess", "res50_irn.pth")
    return {"root": root, "lst": lst, "label_dir": label_dir, "out": out, "result": _run_train(_train_args(root, lst, label_dir, out))}


def test_train_irn_end_to_end(trained):
    from irn_amd.net import weights
    from irn_amd.net.resnet50_irn import EdgeDisplacement, Net
    from irn_amd.voc12 import dataloader
    res = trained["result"]
    assert res["steps"] == 3 and np.isfinite(res["first_losses"]).all() and len(res["first_losses"]) == 4
    state = torch.load(trained["out"], map_location="cpu", weights_only=True)
    init = weights.random_irn_state()
    heads = [k for k in init if k.startswith(("fc_edge", "fc_dp"))]
    trunk = [k for k in init if not k.startswith(("fc_", "edge_layers", "dp_layers", "mean_shift"))]
    assert len(trunk) > 300 and all(torch.equal(state[k], init[k]) for k in trunk)         # bit-unchanged
    assert any(not torch.equal(state[k], init[k]) for k in heads if k.startswith("fc_edge"))
    assert any(not torch.equal(state[k], init[k]) for k in heads if k.startswith("fc_dp"))
    assert all(torch.isfinite(state[k]).all() for k in heads)
    model = weights.load_checkpoint(EdgeDisplacement, trained["out"], strict=False)       # the label steps' way in
    assert torch.equal(model.mean_shift.running_mean, state["mean_shift.running_mean"])
    assert torch.equal(model.fc_dp7[0].weight, state["fc_dp7.0.weight"])
    # the displacement mean, recomputed from the saved weights: mean over the batches of the per-batch channel means
    net = Net()
    net.load_state_dict(state, strict=False)
    net.mean_shift.running_mean.zero_()
    net = net.to(_dev()).eval()
    ds = dataloader.VOC12ImageDataset(trained["lst"], voc12_root=trained["root"], crop_size=96)
    means = []
    with torch.no_grad():
        for i in range(0, 6, 2):
            x = torch.from_numpy(np.stack([ds[i]["img"], ds[i + 1]["img"]])).to(_dev())
            means.append(net(x)[1].mean(dim=(0, 2, 3)))
    expect = torch.stack(means).mean(0).cpu()
    got = state["mean_shift.running_mean"]
    print("\nrunning_mean %s recomputed %s" % (got.tolist(), expect.tolist()))
    assert got.abs().max() > 0
    # the same kernels on the same inputs; a convolution algorithm chosen differently moves an fp32 mean by ~1e-6 relative
    assert torch.allclose(got, expect, rtol=1e-5, atol=1e-6)


def test_same_seed_same_first_step(trained):
    """The data side is a function of the seed alone, bit for bit and whatever the number of loader workers; the first-step
    losses of two runs with one seed agree to fp32 rounding of the network.  The bound: the losses are fp32 network outputs,
    and a second run in one process may be served by another MIOpen convolution algorithm than the first (which searched);
    convolutions of up to 2048 x 9 fp32 terms re-associated differ by ~1e-6 relative, so 1e-5 (~150 fp32 ulps) is allowed —
    another seed changes crops and flips and moves the losses in their second digit."""
    from irn_amd.step import _train, train_irn
    from irn_amd.voc12 import dataloader

    def first_batch(seed, workers):
        ds = dataloader.VOC12AffinityDataset(trained["lst"], label_dir=trained["label_dir"], voc12_root=trained["root"], hor_flip=True,
                                             crop_size=96, crop_method="random", rescale=(0.5, 1.5), seed=seed)
        pack = next(iter(_train.loader(ds, 2, workers, True, seed, train_irn.collate(ds))))
        return pack["name"], pack["img"], pack["label"]

    a, b, c = first_batch(4, 2), first_batch(4, 0), first_batch(5, 0)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not torch.equal(a[1], c[1])
    out = trained["out"] + ".again"
    again = _run_train(_train_args(trained["root"], trained["lst"], trained["label_dir"], out))
    print("\nfirst-step losses %s / %s" % (trained["result"]["first_losses"], again["first_losses"]))
    assert np.allclose(again["first_losses"], trained["result"]["first_losses"], rtol=1e-5, atol=0)
