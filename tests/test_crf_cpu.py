"""The dense-CRF restatement (tests/_densecrf_ref.py) on its own: unary table, softmax, lattice invariants, symmetry of the
filter, Q a distribution, the fg / bg combination rule — and the step / CLI wiring that needs no GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _densecrf_ref as R  # noqa: E402


@pytest.mark.parametrize("n_labels", [2, 4, 21])
def test_unary_table(n_labels):
    labels = np.array([[0, n_labels - 1], [1 % n_labels, 0]])
    u = R.unary_from_labels(labels, n_labels, gt_prob=0.7)
    assert u.dtype == np.float32 and u.shape == (n_labels, 4)
    n_e = np.float32(-np.log(0.3 / (n_labels - 1)))
    p_e = np.float32(-np.log(0.7))
    for p, l in enumerate(labels.reshape(-1)):
        want = np.full(n_labels, n_e, np.float32)
        want[l] = p_e
        assert np.array_equal(u[:, p], want)


def test_softmax_hand_values():
    x = np.array([[0.0, 1000.0], [np.log(3.0), 1000.0]])
    q = R.softmax(x)
    assert np.allclose(q[:, 0], [0.25, 0.75], atol=1e-15)
    assert np.allclose(q[:, 1], [0.5, 0.5], atol=1e-15)            # the maximum is subtracted: no overflow


@pytest.mark.parametrize("d", [2, 5])
def test_lattice_invariants(d):
    rng = np.random.RandomState(d)
    f = (rng.rand(400, d) * 30).astype(np.float32)
    lat = R.Lattice(f)
    assert (lat.bary >= -1e-6).all()
    assert np.allclose(lat.bary.sum(1), 1.0, atol=1e-5)
    assert (lat.full_keys.sum(axis=2) == 0).all()                   # on the plane sum(x) = 0
    for r in range(d + 1):
        assert ((lat.full_keys[:, r, :] - r) % (d + 1) == 0).all()  # vertex r has colour r
    # the vertex keys are distinct, sorted, and every (pixel, remainder) maps to its own key
    assert lat.m == len({tuple(k) for k in lat.keys.tolist()})
    assert np.array_equal(lat.keys[lat.offset.reshape(-1)], lat.full_keys[:, :, :d].reshape(-1, d))
    # neighbour relation: n1 along axis j of v has v as its n2 along j
    for j in range(d + 1):
        n1 = lat.nbr[j, :, 0]
        ok = n1 >= 0
        assert np.array_equal(lat.nbr[j, n1[ok], 1], np.nonzero(ok)[0])


@pytest.mark.parametrize("d", [2, 5])
def test_compute_adjoint_is_the_reversed_blur(d):
    """<a, K b> = <K' a, b> with K' the same filter blurring the axes in reverse order (densecrf's transpose).  K itself
    is symmetric only up to the truncation of the lattice (the blur of one axis and of the next do not commute where
    vertices are missing): 1e-4 .. 5e-3 relative on these sets, so the exact identity is the one pinned here."""
    rng = np.random.RandomState(10 + d)
    f = (rng.rand(300, d) * 8).astype(np.float32)
    lat = R.Lattice(f)
    a, b = rng.randn(300, 2), rng.randn(300, 2)
    lhs = float((a * lat.compute(b)).sum())
    rhs = float((lat.compute(a, reverse=True) * b).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(np.abs(a * lat.compute(b)).sum())
    # ... and with a single blur axis (d + 1 = 2 passes that commute on a full lattice) the forward filter is symmetric
    g = R.Lattice(np.arange(40, dtype=np.float32)[:, None] / np.float32(3))
    x, y = rng.randn(40, 1), rng.randn(40, 1)
    assert abs(float((x * g.compute(y)).sum() - (g.compute(x) * y).sum())) <= 1e-12 * float(np.abs(x * g.compute(y)).sum())


def test_q_is_a_distribution_after_t_iterations():
    from irn_amd import synth
    img = synth.photo(20, 24, seed=3)
    labels = np.random.RandomState(0).randint(0, 4, (20, 24))
    for t in (0, 1, 5):
        q = R.inference(img, labels, t=t, n_labels=4)
        assert (q >= 0).all() and np.allclose(q.sum(0), 1.0, atol=1e-12)
    q32 = R.inference(img, labels, t=3, n_labels=4, dtype=np.float32)
    assert q32.dtype == np.float32 and np.allclose(q32.sum(0), 1.0, atol=1e-5)


def test_combine_rule_hand_maps():
    fg = np.array([[0, 3, 0], [7, 0, 3]])
    bg = np.array([[0, 3, 5], [0, 5, 0]])
    want = np.array([[0, 3, 255], [7, 255, 3]], np.uint8)
    assert np.array_equal(R.combine(fg, bg), want)


def test_seed_labels_first_maximum_wins():
    cams = np.array([[[0.5, 0.2, 0.3]], [[0.5, 0.4, 0.3]]], np.float32)        # [2,1,3]
    assert R.seed_labels(cams, 0.3).tolist() == [[1, 2, 0]]                    # a tie with thr keeps the earlier entry


def test_no_keys_gives_zeros():
    img = np.zeros((5, 6, 3), np.uint8)
    assert np.array_equal(R.ir_label(img, np.zeros((0, 5, 6), np.float32), np.zeros(0, np.int64)), np.zeros((5, 6), np.uint8))


def test_run_sample_accepts_the_pass_and_keeps_its_default():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_sample
    assert "cam_to_ir_label_pass" not in run_sample.OUT_OF_SCOPE
    args = run_sample.build_parser().parse_args(["--voc12_root", "x"])
    assert args.cam_to_ir_label_pass is False
    assert (args.conf_fg_thres, args.conf_bg_thres) == (0.30, 0.05)


def test_step_module_exists():
    from irn_amd.step import cam_to_ir_label
    assert callable(cam_to_ir_label.run)
