"""The fused affinity / displacement loss with a class count (`indexing.affinity_displacement_sums(..., n_classes=C)`,
irn_aff_loss_*_ignore with ignore_from = C + 1), on the two smallest shapes of tests/test_gpu_aff_loss.py.

The loss depends only on which labels are equal, which are 0 and which are ignored.  So an 80-class map with labels from
{0, 7, 21, 50, 80, 255} must give, bit for bit, what the default call gives on the same map relabelled {0, 1, 2, 3, 4, 255}
(the default call is the behaviour pinned on the reference in tests/test_gpu_aff_loss.py): the forward sums and counts and
the two gradients of the ordered backward identical, the atomic backward within the bound that file holds it to (4x the
composed path's own error, `FACTOR * COMPOSED_GRAD_ABS[shape]`).  Without the class count the labels 21, 50 and 80 are
ignored like 255 and the counts differ."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _aff_loss_ref as R  # noqa: E402
from test_gpu_aff_loss import COMPOSED_GRAD_ABS, FACTOR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ((5, 2, 7, 11), (10, 1, 12, 21))
WIDE = np.uint8([0, 7, 21, 50, 80, 255])
NARROW = np.uint8([0, 1, 2, 3, 4, 255])


def _dev():
    return torch.device("cuda", 0)


def _inputs(shape):
    """edge, dp as `R.make_inputs`; the label map as an index map into WIDE / NARROW, in blocks of two cells."""
    radius, batch, hp, wp = shape
    edge, dp, _ = R.make_inputs(radius, batch, hp, wp, seed=7 * radius + wp, block=2)
    rng = np.random.RandomState(hp * wp)
    coarse = rng.choice(6, (batch, -(-hp // 2), -(-wp // 2)), p=[0.3, 0.15, 0.15, 0.15, 0.15, 0.1])
    return edge, dp, np.ascontiguousarray(np.repeat(np.repeat(coarse, 2, 1), 2, 2)[:, :hp, :wp])


def _run(edge, dp, label, radius, ordered, **kw):
    from irn_amd.misc import indexing
    e = torch.from_numpy(edge).to(_dev()).requires_grad_(True)
    d = torch.from_numpy(dp).to(_dev()).requires_grad_(True)
    sums, counts = indexing.affinity_displacement_sums(e, d, torch.from_numpy(label).to(_dev()), radius, ordered=ordered, **kw)
    R.total_loss(sums, counts).backward()
    return {"sums": sums.detach().cpu().numpy(), "counts": counts.cpu().numpy(), "grad_edge": e.grad.cpu().numpy(),
            "grad_dp": d.grad.cpu().numpy()}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d_b%d_%dx%d" % s)
def test_eighty_class_labels_equal_the_relabelled_default_call(shape):
    edge, dp, idx = _inputs(shape)
    radius = shape[0]
    wide, narrow = WIDE[idx], NARROW[idx]
    assert set(np.unique(wide)) == set(WIDE.tolist()), "every label of the set must occur"
    for ordered in (True, False):
        got = _run(edge, dp, wide, radius, ordered, n_classes=80)
        want = _run(edge, dp, narrow, radius, ordered)
        print("\nshape %s ordered %s counts %s" % (shape, ordered, got["counts"]))
        assert (want["counts"] > 0).all(), "the inputs must exercise all three pair classes"
        assert np.array_equal(got["counts"], want["counts"])
        assert got["sums"].tobytes() == want["sums"].tobytes()
        if ordered:
            assert got["grad_edge"].tobytes() == want["grad_edge"].tobytes()
            assert got["grad_dp"].tobytes() == want["grad_dp"].tobytes()
        else:
            b_ge, b_gd = COMPOSED_GRAD_ABS[shape]
            ge = float(np.abs(got["grad_edge"] - want["grad_edge"]).max())
            gd = float(np.abs(got["grad_dp"] - want["grad_dp"]).max())
            print("  atomic backward: grad_edge %.3e (bound %.3e) grad_dp %.3e (bound %.3e)" % (ge, FACTOR * b_ge, gd, FACTOR * b_gd))
            assert ge <= FACTOR * b_ge and gd <= FACTOR * b_gd
    # the labels above 20 take part: the default call on the wide map ignores them and counts fewer pairs
    default = _run(edge, dp, wide, radius, True)
    assert (default["counts"] <= want["counts"]).all() and default["counts"].sum() < want["counts"].sum()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d_b%d_%dx%d" % s)
def test_labels_above_the_class_count_are_void(shape):
    edge, dp, idx = _inputs(shape)
    radius = shape[0]
    a = np.uint8([0, 7, 81, 50, 200, 255])[idx]
    b = np.uint8([0, 7, 255, 50, 255, 255])[idx]
    for ordered in (True, False):
        got, want = _run(edge, dp, a, radius, ordered, n_classes=80), _run(edge, dp, b, radius, ordered, n_classes=80)
        assert np.array_equal(got["counts"], want["counts"]) and got["sums"].tobytes() == want["sums"].tobytes()
        if ordered:
            assert got["grad_edge"].tobytes() == want["grad_edge"].tobytes() and got["grad_dp"].tobytes() == want["grad_dp"].tobytes()
    # one class: only the labels 0 and 1 take part, 7 and 50 are void
    one = _run(edge, dp, np.uint8([0, 1, 2, 7, 50, 255])[idx], radius, True, n_classes=1)
    ref = _run(edge, dp, np.uint8([0, 1, 255, 255, 255, 255])[idx], radius, True)
    assert np.array_equal(one["counts"], ref["counts"]) and one["sums"].tobytes() == ref["sums"].tobytes()


def test_a_class_count_out_of_range_is_refused():
    from irn_amd.misc import indexing
    edge, dp, idx = _inputs(SHAPES[0])
    args = [torch.from_numpy(a).to(_dev()) for a in (edge, dp, NARROW[idx])]
    for bad in (0, 81, 255):
        with pytest.raises(ValueError, match="n_classes"):
            indexing.affinity_displacement_sums(*args, SHAPES[0][0], n_classes=bad)
