"""Host side of the IRNet training step: the fp64 restatement of the fused loss against the recorded reference, argument
refusal of the three C entries, the optimiser, the augmentations, the affinity dataset and the run_train.py parser.
None of it needs a GPU."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _aff_loss_ref as R  # noqa: E402

from irn_amd import _lib  # noqa: E402
from irn_amd.misc import imutils, torchutils  # noqa: E402
from irn_amd.voc12 import dataloader  # noqa: E402


def test_restatement_reproduces_the_recorded_reference(golden):
    g = golden("aff_loss")
    ref = R.reference(g["edge"], g["dp"], g["label"], int(g["radius"]))
    assert np.array_equal(ref["counts"], g["counts"]) and (g["counts"] > 0).all()
    # the recording is the reference's fp32 arithmetic over <= 2 * 1540 terms per sum: 1e-6 relative is ~10 fp32 ulps
    assert np.allclose(ref["losses"], g["losses"], rtol=1e-6, atol=0)
    assert ref["grad_edge"].shape == g["edge"].shape and ref["grad_dp"].shape == g["dp"].shape
    assert np.abs(ref["grad_edge"]).max() > 0 and np.abs(ref["grad_dp"]).max() > 0


def test_restatement_pair_classes():
    from irn_amd.misc import indexing
    pi = indexing.PathIndex(5, (7, 11))                     # 3x3 sources
    lab = np.full((7, 11), 255, np.uint8)
    assert not any(m.any() for m in R.pair_labels(lab, pi))
    lab[:] = 0
    bg, fg, neg = R.pair_labels(lab, pi)
    assert bg.all() and not fg.any() and not neg.any()
    lab[:] = 4
    bg, fg, neg = R.pair_labels(lab, pi)
    assert fg.all() and not bg.any() and not neg.any()
    lab[:, 6:] = 9
    bg, fg, neg = R.pair_labels(lab, pi)
    assert neg.any() and fg.any() and not bg.any() and not (neg & fg).any()
    # the ignore threshold: 1..20 are classes, 21..255 take no part.  20 | 21 side by side: 20 pairs with 20 as fg, 21 with nothing
    lab[:] = 20
    lab[:, 6:] = 21
    bg, fg, neg = R.pair_labels(lab, pi)
    flat = lab.reshape(-1)
    a, b = np.broadcast_to(flat[pi.src_indices][None], bg.shape), flat[pi.dst_indices]
    assert not bg.any() and not neg.any() and fg.any()
    assert np.array_equal(fg, (a == 20) & (b == 20)) and (a == 21).any() and ((a == 20) & (b == 21)).any()
    # 254 behaves as 255: beside background and a class, both maps give the same three masks
    lab[:] = 0
    lab[2:, 3:9] = 20
    lab[:, 5:7] = 254
    with_254 = R.pair_labels(lab, pi)
    lab[lab == 254] = 255
    with_255 = R.pair_labels(lab, pi)
    assert all(np.array_equal(p, q) for p, q in zip(with_254, with_255))
    assert all(m.any() for m in with_254) and not (with_254[0] | with_254[1] | with_254[2]).all()
    # and the first class is a class: 0 | 1 is a negative pair, 1 | 1 a foreground pair
    lab[:] = 0
    lab[:, 6:] = 1
    bg, fg, neg = R.pair_labels(lab, pi)
    assert bg.any() and fg.any() and neg.any()


@pytest.mark.parametrize("shape", tuple(R.DEGENERATE_SEED), ids=lambda s: "r%d_b%d_%dx%d" % s)
def test_degenerate_inputs_provoke_what_they_are_for(shape):
    """The second input family at every shape of DEGENERATE_SEED with its seed: all three pair classes, tied path maxima,
    both edge saturations, residuals of exactly 0 for fg and bg pairs; and the helpers the GPU tests build their per-cell
    bounds from agree with each other on it."""
    radius, batch, hp, wp = shape
    edge, dp, label = R.make_degenerate_inputs(radius, batch, hp, wp, R.DEGENERATE_SEED[shape])
    assert edge.dtype == np.float32 and dp.dtype == np.float32 and label.dtype == np.uint8
    assert set(np.unique(edge)) == {0.0, 0.25, 0.5, 0.75, 1.0}
    assert set(np.unique(dp)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(np.unique(label)) <= {0, 1, 20, 21, 254, 255}
    ref = R.reference(edge, dp, label, radius, fp32_constants=True)
    tied, fg_zero, bg_zero = R.degeneracy(edge, dp, label, radius)
    assert (ref["counts"] > 0).all() and (ref["sums"] > 0).all()
    assert tied > 0 and fg_zero > 0 and bg_zero > 0
    # the gradient of the total loss is the gradient under its coefficients (fp64 on both sides: 1e-12 is ~4000 ulps of
    # slack for the different order of the products), and no cell's exceeds the sum of its |addends|
    coef = R.total_loss_coefficients(ref["counts"])
    by_coef = R.reference(edge, dp, label, radius, fp32_constants=True, coef=coef)
    assert np.allclose(by_coef["grad_edge"], ref["grad_edge"], rtol=1e-12, atol=0)
    assert np.allclose(by_coef["grad_dp"], ref["grad_dp"], rtol=1e-12, atol=0)
    mag_e, mag_d = R.addend_magnitudes(edge, dp, label, radius, coef, fp32_constants=True)
    assert (np.abs(ref["grad_edge"]) <= mag_e * (1 + 1e-12)).all() and (np.abs(ref["grad_dp"]) <= mag_d * (1 + 1e-12)).all()
    assert (mag_e > 0).any() and (mag_e == 0).any() and (mag_d > 0).any()
    # the fp32 constants touch the logarithms only: counts and displacement sums are the same numbers
    exact = R.reference(edge, dp, label, radius)
    assert np.array_equal(exact["sums"][[3, 4]], ref["sums"][[3, 4]]) and np.array_equal(exact["counts"], ref["counts"])


def test_restatement_constants_at_their_fp32_values():
    """One unequal pair over a path of zeros: -log(1 + 1e-5 - 1) with the constant exact and at its fp32 value."""
    edge = np.zeros((1, 2, 3), np.float32)
    label = np.asarray([[[255, 1, 2], [255, 255, 255]]], np.uint8)       # radius 2: one 1x1 source rectangle, the cell (0, 1)
    dp = np.zeros((1, 2, 2, 3), np.float32)
    exact, fp32 = R.reference(edge, dp, label, 2), R.reference(edge, dp, label, 2, fp32_constants=True)
    assert exact["counts"].tolist() == [0, 0, 1] and fp32["counts"].tolist() == [0, 0, 1]
    assert exact["sums"][2] == pytest.approx(-np.log(1e-5), rel=1e-9)
    assert fp32["sums"][2] == -np.log(float(np.float32(1.00001) - np.float32(1.0)))
    assert abs(fp32["sums"][2] - exact["sums"][2]) > 1e-3                # log(1.00136e-5 / 1e-5) = 1.36e-3


def test_c_entries_refuse_bad_arguments_before_any_device():
    L = _lib.lib
    one = C.c_void_p(64)                                     # never dereferenced on these paths
    need = L.irn_aff_loss_workspace_bytes(2, 33, 47, 5)
    assert need == 2 * 4 * 2 * 8 * 8                         # 29x39 sources in 8x32 tiles: 4 x 2 per image, 8 words each
    assert L.irn_aff_loss_workspace_bytes(32, 128, 128, 10) == 32 * 60 * 64
    for bad in ((0, 33, 47, 5), (2, 4, 47, 5), (2, 33, 8, 5), (2, 33, 47, 1), (2, 33, 47, 17)):
        assert L.irn_aff_loss_workspace_bytes(*bad) == 0

    def fwd(edge=one, dp=one, label=one, batch=2, hp=33, wp=47, radius=5, sums=one, counts=one, ws=one, ws_bytes=need):
        return L.irn_aff_loss_forward(edge, dp, label, batch, hp, wp, radius, 21, sums, counts, ws, ws_bytes, None)

    def bwd(edge=one, dp=one, label=one, batch=2, hp=33, wp=47, radius=5, coef=one, ge=one, gd=one, ws=one, ws_bytes=need):
        return L.irn_aff_loss_backward(edge, dp, label, batch, hp, wp, radius, 21, coef, ge, gd, ws, ws_bytes, None)

    for call, pointers in ((fwd, ("edge", "dp", "label", "sums", "counts", "ws")),
                           (bwd, ("edge", "dp", "label", "coef", "ge", "gd", "ws"))):
        for name in pointers:
            assert call(**{name: None}) == 1, name
        assert b"irn_aff_loss" in L.irn_last_error()
        assert call(batch=0) == 1
        assert call(hp=4) == 1 and b"too small" in L.irn_last_error()      # hp <= rf
        assert call(wp=8) == 1                                              # wp <= 2 rf
        assert call(radius=1) == 1 and call(radius=17) == 1
        assert call(ws_bytes=need - 1) == 3 and b"workspace" in L.irn_last_error()   # IRN_ERR_STATE


def test_operator_refuses_cpu_tensors():
    from irn_amd.misc import indexing
    e, d, lab = torch.rand(1, 7, 11), torch.randn(1, 2, 7, 11), torch.zeros(1, 7, 11, dtype=torch.uint8)
    with pytest.raises(ValueError):
        indexing.affinity_displacement_sums(e, d, lab, 5)


def test_poly_optimizer_follows_the_closed_form_and_stops():
    w1, w2 = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))
    opt = torchutils.PolyOptimizer([{"params": [w1], "lr": 0.1, "weight_decay": 0.0},
                                    {"params": [w2], "lr": 1.0, "weight_decay": 0.0}], lr=0.1, weight_decay=0.0, max_step=4)
    expect1, expect2 = 1.0, 1.0
    for step in range(6):
        opt.zero_grad()
        (w1.sum() + w2.sum()).backward()                                  # gradient 1 everywhere
        opt.step()
        assert opt.global_step == step + 1
        if step < 4:
            mult = (1 - step / 4) ** 0.9
            assert opt.param_groups[0]["lr"] == pytest.approx(0.1 * mult, rel=1e-12)
            assert opt.param_groups[1]["lr"] == pytest.approx(1.0 * mult, rel=1e-12)
            expect1 -= 0.1 * mult
            expect2 -= 1.0 * mult
        assert torch.allclose(w1, torch.full((3,), expect1), atol=1e-6)   # unchanged at and beyond max_step
        assert torch.allclose(w2, torch.full((2,), expect2), atol=1e-6)
    # weight decay is SGD's: w <- w - lr * (g + wd * w)
    w = torch.nn.Parameter(torch.full((1,), 2.0))
    opt = torchutils.PolyOptimizer([{"params": [w], "lr": 0.5, "weight_decay": 0.1}], lr=0.5, weight_decay=0.1, max_step=10)
    w.sum().backward()
    opt.step()
    assert float(w.detach()) == pytest.approx(2.0 - 0.5 * (1.0 + 0.1 * 2.0), rel=1e-6)


def _coded_pair(h, w):
    """An image whose red / green bytes spell the pixel's coordinates and a label that depends on them: alignment of the two
    is checkable after any flip or crop."""
    yy, xx = np.mgrid[:h, :w]
    img = np.stack([yy, xx, np.full_like(yy, 7)], -1).astype(np.uint8)
    label = ((yy // 5 + xx // 5) % 3).astype(np.uint8)
    return img, label


@pytest.mark.parametrize("make_rng", [lambda s: np.random.default_rng(s), lambda s: random.Random(s)], ids=["numpy", "random"])
def test_augmentations_same_seed_alignment_and_fill(make_rng):
    img, label = _coded_pair(40, 60)
    # crop larger than the image in one axis and smaller in the other: fill values and a window at once
    for seed in range(6):
        a = imutils.random_crop(imutils.random_lr_flip((img, label), make_rng(seed)), 48, (0, 255), make_rng(seed + 100))
        b = imutils.random_crop(imutils.random_lr_flip((img, label), make_rng(seed)), 48, (0, 255), make_rng(seed + 100))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        ci, cl = a
        assert ci.shape == (48, 48, 3) and cl.shape == (48, 48) and ci.dtype == np.uint8 and cl.dtype == np.uint8
        inside = ci[..., 2] == 7
        assert inside.sum() == 40 * 48                                     # all 40 rows, a 48-column window
        assert (ci[~inside] == 0).all() and (cl[~inside] == 255).all()
        yy, xx = ci[..., 0].astype(int), ci[..., 1].astype(int)
        assert np.array_equal(cl[inside], ((yy // 5 + xx // 5) % 3)[inside])     # label still belongs to its pixel
    flips = {bool(imutils.random_lr_flip((img, label), make_rng(s))[0][0, 0, 1]) for s in range(16)}
    assert flips == {True, False}                                           # both outcomes occur
    boxes = {tuple(np.argwhere(imutils.random_crop((img, label), 48, (0, 255), make_rng(s))[0][..., 2] == 7)[0]) for s in range(16)}
    assert len(boxes) > 1


def test_random_scale_and_top_left_crop():
    img, label = _coded_pair(40, 60)
    for seed in range(4):
        si, sl = imutils.random_scale((img, label), (0.5, 1.5), (3, 0), np.random.default_rng(seed))
        s2, _ = imutils.random_scale((img, label), (0.5, 1.5), (3, 0), np.random.default_rng(seed))
        assert np.array_equal(si, s2)
        assert si.shape[:2] == sl.shape and 20 <= sl.shape[0] <= 60 and 30 <= sl.shape[1] <= 90
        assert set(np.unique(sl)) <= {0, 1, 2}                              # order 0: no label is invented
    t = imutils.top_left_crop(label, 48, 255)
    assert np.array_equal(t[:40, :48], label[:, :48]) and (t[40:] == 255).all()
    t = imutils.top_left_crop(img.astype(np.float32), 64, 0)
    assert t.dtype == np.float32 and np.array_equal(t[:40, :60], img) and (t[40:] == 0).all() and (t[:, 60:] == 0).all()


def test_affinity_dataset_reduced_label(tmp_path):
    lst, label_dir = R.write_voc(str(tmp_path), 3)
    ds = dataloader.VOC12AffinityDataset(lst, label_dir=label_dir, crop_size=96, voc12_root=str(tmp_path), hor_flip=True,
                                         crop_method="random", rescale=(0.5, 1.5), seed=5)
    assert len(ds) == 3
    for idx in range(3):
        item = ds[idx]
        assert set(item) == {"name", "img", "label"}                      # no [|S|, N] tensors
        assert item["img"].shape == (3, 96, 96) and item["img"].dtype == np.float32
        assert item["label"].shape == (24, 24) and item["label"].dtype == np.uint8
        assert set(np.unique(item["label"])) <= {0, 3, 7, 255}
        again = ds[idx]
        assert np.array_equal(item["img"], again["img"]) and np.array_equal(item["label"], again["label"])
    ds.set_epoch(1)
    assert any(not np.array_equal(ds[i]["img"], item["img"]) for i in range(3))
    # without augmentation the reduced map is the nearest-neighbour quarter of the top-left crop of the file, and the image its
    # normalised top-left crop
    plain = dataloader.VOC12AffinityDataset(lst, label_dir=label_dir, crop_size=96, voc12_root=str(tmp_path), crop_method="top_left")
    item = plain[1]
    lab = np.asarray(Image.open(os.path.join(label_dir, "2007_000002.png")))
    assert np.array_equal(item["label"], imutils.pil_rescale(np.ascontiguousarray(lab[:96, :96]), 0.25, 0))
    img = np.asarray(Image.open(os.path.join(str(tmp_path), "JPEGImages", "2007_000002.jpg")).convert("RGB"))
    expect = dataloader.TorchvisionNormalize()(img)[:96, :96].transpose(2, 0, 1)
    assert np.array_equal(item["img"], expect)
    infer = dataloader.VOC12ImageDataset(lst, voc12_root=str(tmp_path), crop_size=128)
    item = infer[1]
    assert item["img"].shape == (3, 128, 128) and np.array_equal(item["img"][:, :120, :128], dataloader.TorchvisionNormalize()(img)[:, :128].transpose(2, 0, 1))
    assert (item["img"][:, 120:] == 0).all()


def test_run_train_parser_and_refusals(tmp_path):
    import run_sample
    import run_train
    a = run_train.build_parser().parse_args(["--voc12_root", "x"])
    assert a.seed == 0 and a.irn_init_weights is None and a.train_irn_pass is False
    assert (a.irn_crop_size, a.irn_batch_size, a.irn_num_epoches, a.irn_learning_rate, a.irn_weight_decay) == (512, 32, 3, 0.1, 1e-4)
    a = run_train.build_parser().parse_args(["--voc12_root", "x", "--seed", "3", "--irn_init_weights", "w.pth", "--train_irn_pass", "True"])
    assert a.seed == 3 and a.irn_init_weights == "w.pth" and a.train_irn_pass is True
    with pytest.raises(SystemExit):
        run_train.main(["--voc12_root", str(tmp_path), "--train_cam_pass", "True", "--log_name", str(tmp_path / "log")])
    assert not os.path.exists(str(tmp_path / "log.log"))                   # refused before anything is opened
    assert run_sample.OUT_OF_SCOPE == ("train_cam_pass", "train_irn_pass")
    with pytest.raises(SystemExit) as e:
        run_sample.main(["--voc12_root", str(tmp_path), "--train_irn_pass", "True", "--log_name", str(tmp_path / "log")])
    assert "run_train.py" in str(e.value)
