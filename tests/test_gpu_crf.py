"""Dense CRF on the GPU (irn_amd/csrc/crf.hip) against the numpy restatement tests/_densecrf_ref.py, and the
cam_to_ir_label step end to end (reference step/cam_to_ir_label.py, misc/imutils.py:156-170).

Lattice: the vertex set and the neighbour relation equal the restatement's exactly (both build the geometry in float32
op for op); the filter is within 1e-5 of the float64 restatement relative to max |value|.  Inference: Q within 1e-4
max-abs of the float64 restatement; a label may differ only at a pixel whose two best Q entries are a < 1e-4 tie
(tests/_parity.py), with no allowance on the count.  Reproducibility is bitwise."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _densecrf_ref as R  # noqa: E402
from _parity import TIE_TOL, label_mismatches  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 37), (29, 1), (7, 5), (64, 48), (500, 375), (375, 500)]


def _image(kind, h, w, seed=0):
    from irn_amd import synth
    if kind == "uniform":
        return np.broadcast_to(np.array([90, 140, 200], np.uint8), (h, w, 3)).copy()
    if kind == "noise":
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    return synth.photo(h, w, seed=seed)


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("kind", ["uniform", "noise", "photo"])
@pytest.mark.parametrize("h,w", SIZES)
def test_lattice_and_filter_vs_restatement(h, w, kind):
    from irn_amd import ops
    img = _image(kind, h, w, seed=h * 1000 + w)
    rng = np.random.RandomState(h + w)
    for feat in (R.gaussian_features(h, w), R.bilateral_features(img)):
        d = feat.shape[1]
        lat = R.Lattice(feat)
        vals = rng.randn(h * w, 3)
        out, keys, nbr = ops.crf_filter(torch.from_numpy(feat).to(_dev()), torch.from_numpy(vals.astype(np.float32)).to(_dev()),
                                        return_lattice=True)
        assert keys.shape[0] == lat.m, (kind, h, w, d, keys.shape[0], lat.m)
        assert np.array_equal(keys.cpu().numpy(), lat.keys), (kind, h, w, d)
        assert np.array_equal(nbr.cpu().numpy(), lat.nbr), (kind, h, w, d)
        want = lat.compute(vals.astype(np.float32).astype(np.float64))
        err = float(np.abs(out.cpu().numpy() - want).max()) / max(float(np.abs(want).max()), 1e-30)
        assert err <= 1e-5, (kind, h, w, d, err)


def _seed_labels(h, w, n_labels, seed):
    from irn_amd import synth
    cams = synth.cam_blobs(max(n_labels - 1, 1), h, w, seed=seed)
    return R.seed_labels(cams[:n_labels - 1], 0.3) if n_labels > 1 else np.zeros((h, w), np.int64)


def _assert_label_parity(got, want, q, what):
    """got / want [H,W] label maps; q the restatement's Q [L, H*W]."""
    h, w = want.shape
    label_mismatches(got + 1, want + 1, q.reshape(-1, h, w), -1.0, what=what)


@pytest.mark.parametrize("n_labels", [2, 4, 21])
@pytest.mark.parametrize("t", [0, 1, 10])
def test_inference_vs_restatement(t, n_labels):
    from irn_amd import ops, synth
    h, w = 48, 64
    img = synth.photo(h, w, seed=5)
    labels = _seed_labels(h, w, n_labels, seed=n_labels)
    lab, q = ops.crf_inference_label(torch.from_numpy(img).to(_dev()), torch.from_numpy(labels).to(_dev()), t=t,
                                     n_labels=n_labels, want_q=True)
    q_want = R.inference(img, labels, t=t, n_labels=n_labels)
    err = float(np.abs(q.cpu().numpy().reshape(n_labels, -1) - q_want).max())
    assert err <= 1e-4, (t, n_labels, err)
    want = np.argmax(q_want.reshape(n_labels, h, w), axis=0)
    _assert_label_parity(lab.cpu().numpy(), want, q_want, "t=%d L=%d" % (t, n_labels))


def test_inference_voc_size_and_imutils_mirror():
    from irn_amd import synth
    from irn_amd.misc import imutils
    h, w = 375, 500
    img = synth.photo(h, w, seed=11)
    labels = _seed_labels(h, w, 3, seed=4)
    got = imutils.crf_inference_label(img, labels, n_labels=3)
    assert got.dtype == np.int64 and got.shape == (h, w)
    q = R.inference(img, labels, t=10, n_labels=3)
    _assert_label_parity(got, np.argmax(q.reshape(3, h, w), axis=0), q, "voc")


def _conf_ties(conf_got, conf_want, qs, what):
    """Pixels of the ir-label map that differ must be ties of the fg or the bg CRF's Q."""
    diff = conf_got != conf_want
    if not diff.any():
        return 0
    h, w = conf_want.shape
    gaps = []
    for q in qs:
        s = np.sort(q.reshape(q.shape[0], h, w)[:, diff], axis=0)
        gaps.append(s[-1] - s[-2])
    gap = np.minimum(gaps[0], gaps[1])
    assert float(gap.max()) < TIE_TOL, "%s: %d pixels differ, one is not a tie (gap %.3g)" % (what, int(diff.sum()), float(gap.max()))
    return int(diff.sum())


def _cam(h, w, k, seed):
    from irn_amd import synth
    return synth.cam_blobs(k, h, w, seed=seed), np.sort(np.random.RandomState(seed).choice(20, k, replace=False))


def test_ir_label_fused_equals_two_single_crfs_and_is_reproducible():
    from irn_amd import ops, synth
    h, w = 375, 500
    img = synth.photo(h, w, seed=21)
    cams, keys = _cam(h, w, 3, seed=21)
    dev = _dev()
    run = lambda: ops.crf_ir_label(torch.from_numpy(img).to(dev), torch.from_numpy(cams).to(dev), keys, 0.30, 0.05).cpu().numpy()  # noqa: E731
    a, b = run(), run()
    assert np.array_equal(a, b)
    singles = []
    for thr in (0.30, 0.05):
        seed = R.seed_labels(cams, thr)
        lab = ops.crf_inference_label(torch.from_numpy(img).to(dev), torch.from_numpy(seed).to(dev), n_labels=4).cpu().numpy()
        singles.append(np.pad(keys + 1, (1, 0))[lab])
    assert np.array_equal(a, R.combine(singles[0], singles[1]))
    assert set(np.unique(a).tolist()) <= {0, 255} | set((keys + 1).tolist())


def test_ir_label_independent_of_image_order():
    from irn_amd import ops, synth
    dev = _dev()
    items = []
    for i, (h, w, k) in enumerate([(375, 500, 2), (97, 131, 5), (500, 375, 1)]):
        cams, keys = _cam(h, w, k, seed=40 + i)
        items.append((synth.photo(h, w, seed=40 + i), cams, keys))

    def go(order):
        return {i: ops.crf_ir_label(torch.from_numpy(items[i][0]).to(dev), torch.from_numpy(items[i][1]).to(dev), items[i][2],
                                    0.30, 0.05).cpu().numpy() for i in order}
    x, y = go([0, 1, 2]), go([2, 1, 0])
    for i in range(3):
        assert np.array_equal(x[i], y[i]), i


def test_ir_label_vs_restatement():
    from irn_amd import ops, synth
    h, w = 120, 160
    img = synth.photo(h, w, seed=8)
    cams, keys = _cam(h, w, 2, seed=8)
    got = ops.crf_ir_label(torch.from_numpy(img).to(_dev()), torch.from_numpy(cams).to(_dev()), keys, 0.30, 0.05).cpu().numpy()
    want, qs = R.ir_label(img, cams, keys, 0.30, 0.05, return_q=True)
    _conf_ties(got, want, qs, "ir_label")
    empty = ops.crf_ir_label(torch.from_numpy(img).to(_dev()), torch.zeros((0, h, w), device=_dev()), np.zeros(0, np.int64), 0.3, 0.05)
    assert not empty.any()


def _threshold_cams(h, w, k, fg, bg, seed):
    """CAMs on a floor of 0.01 whose interesting entries sit exactly on, one ulp below and one ulp above each threshold (and
    at 0.7); pixel p takes scenario p mod 14: one class at the value, or (second half, k > 1) two classes at the same value."""
    f32 = np.float32
    vals = [f32(bg), np.nextafter(f32(bg), f32(-1)), np.nextafter(f32(bg), f32(1)),
            f32(fg), np.nextafter(f32(fg), f32(-1)), np.nextafter(f32(fg), f32(1)), f32(0.7)]
    rng = np.random.RandomState(seed)
    cams = np.full((k, h * w), 0.01, f32)
    for p in range(h * w):
        s = p % (2 * len(vals))
        c1 = int(rng.randint(k))
        cams[c1, p] = vals[s % len(vals)]
        if s >= len(vals) and k > 1:
            cams[(c1 + 1 + int(rng.randint(k - 1))) % k, p] = vals[s % len(vals)]
    return cams.reshape(k, h, w)


@pytest.mark.parametrize("k", [1, 3, 20])
@pytest.mark.parametrize("h,w", [(7, 5), (64, 48)])
def test_ir_label_seed_and_finish_rules_exact_without_iterations(h, w, k):
    """With t = 0 the map is a pure function of k_prologue (seeds: strict >, so a CAM equal to the threshold leaves the
    background and the first of two equal classes wins), the unary softmax and k_finish (argmax, keys, combination): it
    equals the restatement exactly, no tie allowance."""
    from irn_amd import ops, synth
    fg, bg = 0.30, 0.05
    img = synth.photo(h, w, seed=3)
    cams = _threshold_cams(h, w, k, fg, bg, seed=h + k)
    keys = np.sort(np.random.RandomState(k).choice(20, k, replace=False))
    got = ops.crf_ir_label(torch.from_numpy(img).to(_dev()), torch.from_numpy(cams).to(_dev()), keys, fg, bg, t=0).cpu().numpy()
    want = R.ir_label(img, cams, keys, fg, bg, t=0)
    assert np.array_equal(got, want), (h, w, k, int((got != want).sum()))
    # the rules, spelt out on the scenarios (pixel p: scenario p mod 14)
    flat, scen = want.reshape(-1), np.arange(h * w) % 14
    assert (flat[np.isin(scen, (0, 1, 7, 8))] == 0).all()                    # <= bg threshold: background in both seeds
    assert (flat[np.isin(scen, (2, 3, 4, 9, 10, 11))] == 255).all()          # above bg, not above fg: unsure
    seed_fg = R.seed_labels(cams, fg).reshape(-1)
    sure = np.isin(scen, (5, 6, 12, 13))
    assert (seed_fg[sure] > 0).all() and np.array_equal(flat[sure], (keys + 1)[seed_fg[sure] - 1])
    assert np.array_equal(seed_fg[sure], np.argmax(cams.reshape(k, -1)[:, sure] > np.float32(fg), axis=0) + 1)   # the first class wins


@pytest.mark.parametrize("n", [1, 37, 3072])
@pytest.mark.parametrize("d", [1, 3, 4])
def test_lattice_dimensions_1_3_4_vs_restatement(d, n):
    from irn_amd import ops
    feat = R.random_features(n, d)
    lat = R.Lattice(feat)
    vals = np.random.RandomState(d + n).randn(n, 3)
    out, keys, nbr = ops.crf_filter(torch.from_numpy(feat).to(_dev()), torch.from_numpy(vals.astype(np.float32)).to(_dev()),
                                    return_lattice=True)
    assert keys.shape[0] == lat.m, (d, n, keys.shape[0], lat.m)
    assert np.array_equal(keys.cpu().numpy(), lat.keys), (d, n)
    assert np.array_equal(nbr.cpu().numpy(), lat.nbr), (d, n)
    want = lat.compute(vals.astype(np.float32).astype(np.float64))
    err = float(np.abs(out.cpu().numpy() - want).max()) / max(float(np.abs(want).max()), 1e-30)
    assert err <= 1e-5, (d, n, err)


@pytest.mark.parametrize("d,spread", [(1, 1.5e6), (4, 1.5e5)])
def test_lattice_key_outside_the_packed_range_is_refused(d, spread):
    """21 (d = 1) and 16 (d = 4) bits per key component: features this wide leave the range, and the call must say so rather
    than return a lattice of aliased keys."""
    from irn_amd import ops
    from irn_amd._lib import IrnHipError
    feat = R.random_features(37, d, spread=spread)
    assert np.abs(R.Lattice(feat).keys).max() >= 1 << ((21 if d == 1 else 16) - 1)
    with pytest.raises(IrnHipError, match=r"exceeds \d+ bits per component"):
        ops.crf_filter(torch.from_numpy(feat).to(_dev()), torch.ones((37, 1), device=_dev()), return_lattice=True)


# ---------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------

def _make_voc_with_cams(tmp, n=5):
    from irn_amd import synth
    root = tmp / "voc"
    (root / "JPEGImages").mkdir(parents=True)
    cam_dir = tmp / "cam"
    cam_dir.mkdir()
    names = []
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        h, w = ((96, 128), (113, 150), (75, 60))[i % 3]
        synth_img = synth.photo(h, w, seed=100 + i)
        Image.fromarray(synth_img).save(root / "JPEGImages" / (name + ".jpg"), quality=95)
        k = 0 if i == 2 else 1 + i % 3                     # image 3 has no class keys
        keys = np.sort(np.random.RandomState(i).choice(20, k, replace=False)).astype(np.int64)
        high_res = synth.cam_blobs(k, h, w, seed=100 + i) if k else np.zeros((0, h, w), np.float32)
        np.save(cam_dir / (name + ".npy"), {"keys": keys, "high_res": high_res})
        names.append(name)
    (tmp / "lists").mkdir()
    (tmp / "lists" / "train.txt").write_text("\n".join(names) + "\n")
    return root, names, cam_dir


def _step_args(tmp, root, cam_dir, tag, **kw):
    return argparse.Namespace(num_workers=2, voc12_root=str(root), train_list=str(tmp / "lists" / "train.txt"),
                              infer_list=str(tmp / "lists" / "train.txt"), cam_out_dir=str(cam_dir),
                              ir_label_out_dir=str(tmp / tag), conf_fg_thres=0.30, conf_bg_thres=0.05, **kw)


def _check_step_outputs(out_dir, root, names, cam_dir):
    for name in names:
        got = np.asarray(Image.open(os.path.join(out_dir, name + ".png")))
        img = np.asarray(Image.open(root / "JPEGImages" / (name + ".jpg")).convert("RGB"))
        cam = np.load(cam_dir / (name + ".npy"), allow_pickle=True).item()
        want, qs = R.ir_label(img, cam["high_res"], cam["keys"], 0.30, 0.05, return_q=True)
        assert got.dtype == np.uint8 and got.shape == want.shape, name
        if qs is None:
            assert not got.any(), name
        else:
            _conf_ties(got, want, qs, name)


def test_step_end_to_end_and_worker_layouts(tmp_path):
    from irn_amd.step import _common, cam_to_ir_label
    root, names, cam_dir = _make_voc_with_cams(tmp_path)
    one = _step_args(tmp_path, root, cam_dir, "one")
    cam_to_ir_label.run(one)
    _check_step_outputs(one.ir_label_out_dir, root, names, cam_dir)
    two = _step_args(tmp_path, root, cam_dir, "two", worker_devices="0,0")
    try:
        cam_to_ir_label.run(two)
    finally:
        _common.shutdown_workers()
    for name in names:
        a = np.asarray(Image.open(os.path.join(one.ir_label_out_dir, name + ".png")))
        b = np.asarray(Image.open(os.path.join(two.ir_label_out_dir, name + ".png")))
        assert np.array_equal(a, b), name


def test_run_sample_cam_to_ir_label_pass(tmp_path):
    import run_sample
    from irn_amd.step import _common
    root, names, cam_dir = _make_voc_with_cams(tmp_path, n=3)
    out = tmp_path / "ir"
    try:
        run_sample.main(["--voc12_root", str(root), "--train_list", str(tmp_path / "lists" / "train.txt"),
                         "--num_workers", "2", "--cam_out_dir", str(cam_dir), "--ir_label_out_dir", str(out),
                         "--make_cam_pass", "False", "--make_ins_seg_pass", "False", "--make_sem_seg_pass", "False",
                         "--cam_to_ir_label_pass", "True", "--sem_seg_out_dir", str(tmp_path / "sem"),
                         "--ins_seg_out_dir", str(tmp_path / "ins"), "--log_name", str(tmp_path / "log")])
    finally:
        _common.shutdown_workers()
    _check_step_outputs(str(out), root, names, cam_dir)
