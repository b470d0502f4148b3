"""Host-side mirrors: backbones reproduce the reference's forward on the same seeded weights,
sharding partitions the dataset, small helpers match."""
import os

import numpy as np
import pytest
import torch

from irn_amd.misc import imutils, pyutils, torchutils


def test_cam_forward_matches_reference(golden):
    from irn_amd.net import resnet50_cam, weights
    g = golden("nets")
    net = resnet50_cam.CAM()
    net.load_state_dict(weights.random_cam_state(seed=1), strict=True)
    net.eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g["cam_in"]))
    assert y.shape == g["cam_out"].shape
    assert np.abs(y.numpy() - g["cam_out"]).max() <= 1e-4 * max(1.0, np.abs(g["cam_out"]).max())


def test_edge_displacement_forward_matches_reference(golden):
    from irn_amd.net import resnet50_irn, weights
    g = golden("nets")
    net = resnet50_irn.EdgeDisplacement(crop_size=128)
    net.load_state_dict(weights.random_irn_state(seed=2), strict=False)
    net.eval()
    with torch.no_grad():
        edge, dp = net(torch.from_numpy(g["irn_in"]))
    assert edge.shape == g["irn_edge"].shape and dp.shape == g["irn_dp"].shape
    assert np.abs(edge.numpy() - g["irn_edge"]).max() <= 1e-4
    assert np.abs(dp.numpy() - g["irn_dp"]).max() <= 1e-4 * max(1.0, np.abs(g["irn_dp"]).max())


def test_state_dict_keys_cover_reference_aliases():
    from irn_amd.net import resnet50_cam, resnet50_irn
    cam_keys = set(resnet50_cam.CAM().state_dict())
    for k in ("resnet50.conv1.weight", "stage1.0.weight", "stage1.4.0.conv1.weight", "backbone.3.0.2.bn3.running_var",
              "classifier.weight", "newly_added.0.weight", "resnet50.layer4.0.downsample.1.running_mean"):
        assert k in cam_keys, k
    irn_keys = set(resnet50_irn.EdgeDisplacement().state_dict())
    for k in ("fc_edge3.0.weight", "fc_edge6.bias", "fc_dp7.3.weight", "fc_dp7.4.running_mean",
              "mean_shift.running_mean", "edge_layers.5.weight", "dp_layers.6.1.bias", "stage5.0.2.conv3.weight"):
        assert k in irn_keys, k


@pytest.mark.parametrize("n_items,n", [(10, 1), (11, 2), (1449, 4), (10582, 8), (5, 8)])
def test_split_dataset_partitions(n_items, n):
    shards = torchutils.split_dataset(list(range(n_items)), n)
    seen = np.concatenate([np.asarray(s.indices) for s in shards])
    assert len(shards) == n and sorted(seen.tolist()) == list(range(n_items))
    for r in range(n):
        assert np.array_equal(shards[r].indices, torchutils.shard_indices(n_items, r, n))


def test_small_helpers():
    assert imutils.get_strided_size((375, 500), 4) == (94, 125)
    assert imutils.get_strided_up_size((375, 500), 16) == (384, 512)
    a = np.array([[5, 5, 9], [2, 9, 2]])
    assert np.array_equal(imutils.compress_range(a), [[1, 1, 2], [0, 2, 0]])
    oh = pyutils.to_one_hot(np.array([[0, 2], [1, 1]]))
    assert oh.shape == (3, 2, 2) and oh.dtype == np.bool_ and oh[2, 0, 1] and oh.sum() == 4
    assert pyutils.to_one_hot(np.array([0, 1]), maximum_val=4).shape == (4, 2)


def test_dataset_msf(tmp_path):
    from PIL import Image
    from irn_amd.voc12 import dataloader
    root = tmp_path / "voc"
    (root / "JPEGImages").mkdir(parents=True)
    rng = np.random.RandomState(0)
    Image.fromarray(rng.randint(0, 255, (37, 50, 3), dtype=np.uint8)).save(root / "JPEGImages" / "2007_000032.jpg")
    lst = tmp_path / "list.txt"
    lst.write_text("2007_000032\n")
    lab = np.zeros(20, np.float32)
    lab[[3, 7]] = 1
    ds = dataloader.VOC12ClassificationDatasetMSF(str(lst), str(root), scales=(1.0, 0.5, 2.0),
                                                  cls_labels={2007000032: lab})
    item = ds[0]
    assert item["name"] == "2007_000032" and item["size"] == (37, 50)
    assert [tuple(x.shape) for x in item["img"]] == [(2, 3, 37, 50), (2, 3, 18, 25), (2, 3, 74, 100)]
    assert np.array_equal(item["img"][0][1], item["img"][0][0][..., ::-1])
    assert dataloader.decode_int_filename(2007000032) == "2007_000032"


def test_cam_merge_matches_reference_golden(golden):
    """step/make_cam.py:32-52 through the torch-op mirror of the merge (CPU here) against the reference's
    outputs; the HIP kernel the step uses is checked against the same fixture in test_gpu_steps.py."""
    from oracle import torch_mirrors
    cm = golden("cam_merge")
    for name in "ab":
        outs = [torch.from_numpy(cm["%s_out%d" % (name, i)]) for i in range(4)]
        keys, cam, hi = torch_mirrors.merge_scales_torch(outs, tuple(int(v) for v in cm[name + "_size"]),
                                              torch.from_numpy(cm[name + "_label"]))
        assert np.array_equal(keys.numpy(), cm[name + "_keys"])
        assert np.abs(cam.numpy() - cm[name + "_cam"]).max() <= 1e-6
        assert np.abs(hi.numpy() - cm[name + "_high_res"]).max() <= 1e-6


def test_bicubic_plan_host_table_equals_oracle():
    """irn_bicubic_plan is host-only (no GPU): the fixed-point tap tables the kernels consume are Pillow's."""
    from irn_amd import ops
    from oracle import msf_oracle as M
    for n_in, n_out in [(500, 250), (375, 188), (375, 562), (500, 1000), (7, 3), (333, 334), (281, 1), (3, 40)]:
        lo, cnt, k = ops.bicubic_plan(n_in, n_out)
        a, b, c = M.bicubic_coeffs(n_in, n_out)
        assert np.array_equal(lo, a) and np.array_equal(cnt, b) and np.array_equal(k, c), (n_in, n_out)
    lo, cnt, k = ops.bicubic_plan(64, 64)                    # identity plan = "pass skipped"
    assert np.array_equal(lo, np.arange(64)) and (cnt == 1).all() and (k == 1 << 22).all()


def test_normalize_lut_equals_reference_normalisation():
    from irn_amd import ops
    from irn_amd.voc12.dataloader import TorchvisionNormalize
    img = np.random.RandomState(1).randint(0, 256, (9, 11, 3)).astype(np.uint8)
    lut = ops.normalize_lut()
    assert np.array_equal(TorchvisionNormalize()(img), np.stack([lut[c][img[..., c]] for c in range(3)], -1))


def test_msf_pack_refuses_cpu_tensors():
    from irn_amd import ops
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.msf_pack(torch.zeros((4, 4, 3), dtype=torch.uint8), (1.0,))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.bicubic_resize(torch.zeros((4, 4, 3), dtype=torch.uint8), (2, 2))


def test_dataset_raw_mode_hands_over_the_decoded_image(tmp_path):
    """raw=True: the item carries the decoded uint8 image (the steps build the scales on the GPU); name, size and
    label are those of the reference-format item."""
    from PIL import Image
    from irn_amd import synth
    from irn_amd.voc12 import dataloader
    root = tmp_path / "voc"
    (root / "JPEGImages").mkdir(parents=True)
    img = synth.photo(37, 52, seed=3)
    Image.fromarray(img).save(root / "JPEGImages" / "2008_000001.jpg", quality=95)
    (tmp_path / "train.txt").write_text("2008_000001\n")
    lab = np.zeros(20, np.float32)
    lab[[2, 7]] = 1
    kw = dict(voc12_root=str(root), scales=(1.0, 0.5), cls_labels={2008000001: lab})
    raw = dataloader.VOC12ClassificationDatasetMSF(str(tmp_path / "train.txt"), raw=True, **kw)[0]
    ref = dataloader.VOC12ClassificationDatasetMSF(str(tmp_path / "train.txt"), **kw)[0]
    decoded = np.asarray(Image.open(root / "JPEGImages" / "2008_000001.jpg").convert("RGB"))
    assert raw["img"].dtype == torch.uint8 and np.array_equal(raw["img"].numpy(), decoded)
    assert raw["name"] == ref["name"] and raw["size"] == ref["size"] == (37, 52)
    assert torch.equal(raw["label"], ref["label"])
    # the host loop over the same decoded image is what the oracle restates
    from oracle import msf_oracle as M
    for a, b in zip(ref["img"], M.msf_item(decoded, (1.0, 0.5))):
        assert np.array_equal(a, b)


def test_dense_operator_mirrors_match_reference(golden):
    """irn_amd.misc.indexing.affinity_sparse2dense / to_transition_matrix (API-completeness mirrors of reference
    misc/indexing.py:112-139; the walk itself never densifies) against the oracle's restatement and, chained the way
    misc/indexing.py:141-165 chains them, against the reference's own propagate_to_edge output."""
    import torch.nn.functional as F
    from irn_amd.misc import indexing
    from oracle import irn_oracle as O
    af = golden("affinity")
    for r in (3, 5):
        edge = af["r%d_edge" % r]
        h, w = edge.shape
        pi = indexing.PathIndex(r, (h + r, w + 2 * r))
        aff = torch.from_numpy(af["r%d_aff" % r])
        dense = indexing.affinity_sparse2dense(aff, pi.src_indices, pi.dst_indices, (h + r) * (w + 2 * r))
        want = O.affinity_dense(af["r%d_aff" % r], pi.src_indices, pi.dst_indices, (h + r) * (w + 2 * r))
        assert np.array_equal(dense.numpy(), want)
        assert torch.equal(dense, dense.t()) and float(dense.diagonal().min()) == 1.0
        t = indexing.to_transition_matrix(dense[:64, :64].contiguous() + 0.01, 10, 2)
        want_t = O.to_transition_matrix(want[:64, :64] + np.float32(0.01), 10, 2)
        assert np.abs(t.numpy() - want_t).max() <= 1e-6
    wk = golden("walk")
    name = "r5_b10_e4"
    h, w, c, r, beta, e = (int(v) for v in wk[name + "_params"])
    edge = torch.from_numpy(wk[name + "_edge"])[None]
    pi = indexing.PathIndex(r, (h + r, w + 2 * r))
    ep = F.pad(edge, (r, r, 0, r), value=1.0).reshape(-1).numpy()
    aff = torch.from_numpy(O.edge_to_affinity(ep, pi.path_indices))
    dense = indexing.affinity_sparse2dense(aff, pi.src_indices, pi.dst_indices, (h + r) * (w + 2 * r))
    dense = dense.view(h + r, w + 2 * r, h + r, w + 2 * r)[:-r, r:-r, :-r, r:-r].reshape(h * w, h * w)
    t = indexing.to_transition_matrix(dense, beta, e)
    x = torch.from_numpy(wk[name + "_cam"]).view(-1, h, w) * (1 - edge)
    rw = torch.matmul(x.view(-1, h * w), t).view(-1, 1, h, w)
    assert np.abs(rw.numpy() - wk[name + "_rw"]).max() <= 1e-6


def test_logger_and_timer(tmp_path, capsys):
    import sys
    import time
    log = pyutils.Logger(str(tmp_path / "run.log"))
    try:
        t = pyutils.Timer("step.make_cam:")
        print("hello")
        time.sleep(0.01)
        assert t.lapse() >= 0.01 and t.elapsed() >= 0.01
    finally:
        log.close()
    assert sys.stdout is not log
    text = (tmp_path / "run.log").read_text()
    assert "step.make_cam:" in text and "hello" in text
    assert "hello" in capsys.readouterr().out


def test_backbones_at_512_match_reference(golden):
    """CAM.forward on [2,3,512,512] and EdgeDisplacement.forward on a ragged VOC-size item vs the reference's CPU forwards
    (tests/golden/nets512.npz); the GPU forms of these checks live in tests/test_gpu_parity_r2.py."""
    from irn_amd import synth
    from irn_amd.net import resnet50_cam, resnet50_irn, weights
    g = golden("nets512")
    cam = resnet50_cam.CAM()
    cam.load_state_dict(weights.random_cam_state(seed=1), strict=True)
    cam.eval()
    irn = resnet50_irn.EdgeDisplacement()
    irn.load_state_dict(weights.random_irn_state(seed=2), strict=False)
    irn.eval()
    with torch.no_grad():
        h, w, seed = (int(v) for v in g["cam512_seed"])
        y = cam(torch.from_numpy(synth.image_pair(h, w, seed))).numpy()
        assert np.abs(y - g["cam512_out"]).max() <= 1e-4 * np.abs(g["cam512_out"]).max()
        h, w, seed = (int(v) for v in g["irn_seed"])
        edge, dp = irn(torch.from_numpy(synth.image_pair(h, w, seed)))
        assert np.abs(edge.numpy() - g["irn_edge"]).max() <= 1e-4
        assert np.abs(dp.numpy() - g["irn_dp"]).max() <= 1e-4 * max(1.0, np.abs(g["irn_dp"]).max())


def test_frozen_batch_norm_folding_and_composed_path():
    """FrozenBatchNorm.folded() is the batch norm as one multiply-add (the constants irn_bn_act consumes), and apply_ on
    the CPU (or with autograd on) is the reference's composed tail: FixedBatchNorm -> += residual -> ReLU
    (net/resnet50.py:11-14, :34-54), leaving its input untouched."""
    import torch.nn.functional as F
    from irn_amd.net import resnet50 as R
    g = torch.Generator().manual_seed(9)
    bn = R.FrozenBatchNorm(6)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(6, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(6, generator=g))
        bn.running_mean.copy_(torch.randn(6, generator=g))
        bn.running_var.copy_(torch.rand(6, generator=g) + 0.05)
    x = torch.randn(2, 6, 5, 7, generator=g)
    skip = torch.randn(2, 6, 5, 7, generator=g)
    scale, shift = bn.folded()
    with torch.no_grad():
        want = bn(x)
    assert float((x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) - want).abs().max()) < 2e-6
    x0 = x.clone()
    with torch.no_grad():
        y = bn.apply_(x, residual=skip, relu=True)
    assert torch.equal(x, x0) and torch.equal(y, F.relu(want + skip))
    bn.train()                                                   # statistics stay frozen (FixedBatchNorm)
    with torch.no_grad():
        assert torch.equal(bn(x), want)
    key = bn.folded()[0]
    assert bn.folded()[0] is key
    with torch.no_grad():
        bn.weight.mul_(2.0)
    assert float((bn.folded()[0] - 2 * key).abs().max()) < 1e-6


def test_apply_with_a_batch_norm_on_the_residual_composed_path():
    """apply_(x, residual, residual_bn=...) off the device = bn(x) + bn_r(residual) -> ReLU: the projection shortcut of
    net/resnet50.py:48-52."""
    import torch.nn.functional as F
    from irn_amd.net import resnet50 as R
    torch.manual_seed(2)
    bn, bn_r = R.FrozenBatchNorm(4), R.FrozenBatchNorm(4)
    with torch.no_grad():
        for m in (bn, bn_r):
            m.running_mean.normal_()
            m.running_var.uniform_(0.2, 2.0)
            m.weight.normal_()
            m.bias.normal_()
        x, r = torch.randn(2, 4, 3, 5), torch.randn(2, 4, 3, 5)
        assert torch.equal(bn.apply_(x, residual=r, relu=True, residual_bn=bn_r), F.relu(bn(x) + bn_r(r)))
        unit = R.Bottleneck(8, 4, stride=2, project=True).eval()
        y = unit(torch.randn(1, 8, 9, 9))
        assert y.shape == (1, 16, 5, 5) and float(y.min()) >= 0.0


def test_folding_under_inference_mode():
    """Tensors made under torch.inference_mode() have no version counter; the folded constants are then cached by
    storage only."""
    from irn_amd.net import resnet50 as R
    with torch.inference_mode():
        bn = R.FrozenBatchNorm(3)
        scale, shift = bn.folded()
        assert bn.folded()[0] is scale
        x = torch.randn(2, 3, 4, 4)
        assert float((bn.apply_(x, relu=False) - (x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))).abs().max()) < 1e-6


def test_load_checkpoint_skips_only_what_the_checkpoint_overwrites(tmp_path):
    """net/weights.load_checkpoint (the start of every step's run(args), reference step/make_cam.py:63-65): the random
    initialisers are skipped, the loaded network equals the regularly built one, a partial checkpoint keeps a regular
    initialisation for the rest, and torch.nn.init is left as it was."""
    import torch.nn.init as init
    from irn_amd.net import resnet50_cam, weights
    before = init.kaiming_uniform_
    path = str(tmp_path / "cam.pth")
    torch.save(weights.random_cam_state(1), path)
    fast = weights.load_checkpoint(resnet50_cam.CAM, path, strict=True)
    ref = resnet50_cam.CAM()
    ref.load_state_dict(torch.load(path), strict=True)
    ref.eval()
    x = torch.randn(2, 3, 48, 64, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert torch.equal(fast(x), ref(x)) and not fast.training
    sd = torch.load(path)
    dropped = "classifier.weight"
    sd.pop(dropped)
    torch.save(sd, str(tmp_path / "part.pth"))
    part = weights.load_checkpoint(resnet50_cam.CAM, str(tmp_path / "part.pth"), strict=False)
    w = part.state_dict()[dropped]
    assert bool(torch.isfinite(w).all()) and float(w.abs().max()) < 1.0 and float(w.std()) > 1e-4     # a real initialisation
    assert init.kaiming_uniform_ is before


def test_trunk_layout_is_chosen_per_input_shape(monkeypatch):
    """auto: channels-last only for the network-input shapes the shipped find database was tuned for; 1 / 0 force it."""
    from irn_amd.net import resnet50 as r50

    class _T:                    # a tensor stand-in: only the attributes channels_last_for reads
        def __init__(self, shape, cuda=True):
            self.shape, self.is_cuda = shape, cuda

        def dim(self):
            return len(self.shape)

    from irn_amd.step import _common
    monkeypatch.setattr(r50, "_TUNED_SHAPES", {_common.miopen_cache_key(): {(16, 512, 512)}, _common.miopen_cache_key() + "-det": {(16, 512, 512)}})
    monkeypatch.setattr(r50, "DETERMINISTIC", None)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    with torch.no_grad():
        monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "auto")
        monkeypatch.delenv("IRN_MIOPEN_DB_SET", raising=False)
        assert not r50.channels_last_for(_T((16, 3, 512, 512)))       # no miopen_setup in this process: the NHWC entries may be missing
        monkeypatch.setenv("IRN_MIOPEN_DB_SET", "/somewhere")
        assert r50.channels_last_for(_T((16, 3, 512, 512))) and not r50.channels_last_for(_T((16, 3, 375, 500)))
        assert not r50.channels_last_for(_T((2, 3, 512, 512))) and not r50.channels_last_for(_T((16, 3, 512, 512), cuda=False))
        monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "1")
        assert r50.channels_last_for(_T((2, 3, 375, 500)))
        monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "0")
        assert not r50.channels_last_for(_T((16, 3, 512, 512)))
        # a caller's own deterministic flag, not managed by the steps: MIOpen's attribute leaves no fast NHWC solver -> NCHW
        monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "auto")
        torch.backends.cudnn.deterministic = True
        assert not r50.channels_last_for(_T((16, 3, 512, 512)))
        # the reproducible mode of the steps (managed): tuned shapes channels-last WITHOUT the attribute (their database has no
        # order-dependent solver), everything else NCHW WITH it; the end of a pass puts the attribute back on
        monkeypatch.setattr(r50, "DETERMINISTIC", True)
        assert r50.channels_last_for(_T((16, 3, 512, 512))) and torch.backends.cudnn.deterministic is False
        r50.end_trunk_pass()
        assert torch.backends.cudnn.deterministic is True
        assert not r50.channels_last_for(_T((16, 3, 333, 500))) and torch.backends.cudnn.deterministic is True
        monkeypatch.setattr(r50, "DETERMINISTIC", False)
        torch.backends.cudnn.deterministic = False
        assert r50.channels_last_for(_T((16, 3, 512, 512))) and torch.backends.cudnn.deterministic is False
    monkeypatch.setattr(r50, "DETERMINISTIC", None)
    monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "1")
    with torch.enable_grad():
        assert not r50.channels_last_for(_T((16, 3, 512, 512)))       # the training seam keeps the composed NCHW path


def test_reproducible_mode_runs_the_trunk_in_passes_of_a_fixed_size(monkeypatch):
    """which kernels an image meets must not depend on the batch it travels in (shard split, tail of a
    shard, early flush).  Reproducible mode: rows go through in passes of 16 (sizes the shipped database is tuned for: a short
    pass is filled with zero images) or 2 (every other size: the reference's own batch); forced channels-last on an unknown
    shape keeps MIOpen's deterministic attribute on."""
    from irn_amd.net import resnet50 as r50
    from irn_amd.step import _common

    class _T:
        def __init__(self, shape, cuda=True):
            self.shape, self.is_cuda = shape, cuda

        def dim(self):
            return len(self.shape)

    monkeypatch.setattr(r50, "_TUNED_SHAPES", {_common.miopen_cache_key() + "-det": {(16, 512, 512), (16, 375, 500)}})
    monkeypatch.delenv("IRN_DETERMINISTIC", raising=False)
    monkeypatch.setenv("IRN_MIOPEN_DB_SET", "/somewhere")
    monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "auto")
    with torch.no_grad():
        monkeypatch.setattr(r50, "DETERMINISTIC", True)
        assert r50.pass_rows(_T((6, 3, 512, 512))) == 16 and r50.pass_rows(_T((16, 3, 375, 500))) == 16
        assert r50.pass_rows(_T((16, 3, 333, 500))) == 2 and r50.pass_rows(_T((2, 3, 64, 64))) == 2
        monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "0")
        assert r50.pass_rows(_T((16, 3, 512, 512))) == 2                      # no channels-last trunk: every size is "untuned"
        monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "1")
        prev = torch.backends.cudnn.deterministic
        assert r50.channels_last_for(_T((4, 3, 100, 100))) and torch.backends.cudnn.deterministic is True     # forced layout, unknown shape
        assert r50.channels_last_for(_T((16, 3, 512, 512))) and torch.backends.cudnn.deterministic is False
        torch.backends.cudnn.deterministic = prev
        monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "auto")
        for mode in (None, False):
            monkeypatch.setattr(r50, "DETERMINISTIC", mode)
            assert r50.pass_rows(_T((6, 3, 512, 512))) is None                # outside the mode the caller's batch is the pass
        assert r50.pass_rows(_T((6, 3, 512, 512), cuda=False)) is None
    # the chunking itself (CPU tensors, the plan injected): every pass has exactly `rows` rows, pads are dropped, tuples work
    seen = []

    def fn(c):
        seen.append(int(c.shape[0]))
        return c.sum(dim=(1, 2, 3)), c * 2.0

    x = torch.arange(6 * 3 * 2 * 2, dtype=torch.float32).reshape(6, 3, 2, 2)
    monkeypatch.setattr(r50, "pass_rows", lambda t: 4)
    pads0 = r50.PASS_STATS["pad_rows"]
    a, b = r50.run_rows(fn, x)
    assert seen == [4, 4] and r50.PASS_STATS["pad_rows"] - pads0 == 2
    assert torch.equal(a, x.sum(dim=(1, 2, 3))) and torch.equal(b, x * 2.0)
    seen.clear()
    assert torch.equal(r50.run_rows(lambda c: c + 1.0, x[:4]), x[:4] + 1.0)      # a full pass is handed over as it is
    monkeypatch.setattr(r50, "pass_rows", lambda t: None)
    assert torch.equal(r50.run_rows(lambda c: c + 1.0, x), x + 1.0)


def test_gemm_params_fold_is_the_composed_definition_and_follows_bn2_and_the_switches(monkeypatch):
    """Bottleneck.gemm_params (reference net/resnet50.py:34-54 with FixedBatchNorm folded in): w * (gamma / sqrt(var + eps)) in
    float64, rounded to fp32 once; b3 = shift3 + shift_d for a projection unit; bn2's constants are read where they are used, so
    writing bn2 alone changes them; the SPLIT_* switches are part of the cache key."""
    from irn_amd.net import resnet50 as r50
    torch.manual_seed(5)
    for project in (False, True):
        unit = r50.Bottleneck(64 if project else 128, 32, stride=1, project=project).eval()
        bns = [m for m in unit.modules() if isinstance(m, r50.FrozenBatchNorm)]
        with torch.no_grad():
            for m in bns:
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 2.0)

        def fold(conv, bn):
            scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
            return conv.weight.detach().double() * scale.view(-1, 1, 1, 1), bn.bias.detach().double() - bn.running_mean.detach().double() * scale
        p = unit.gemm_params()
        w1, t1 = fold(unit.conv1, unit.bn1)
        w3, t3 = fold(unit.conv3, unit.bn3)
        assert torch.equal(p["w1"], w1.float().flatten(1)) and torch.equal(p["b1"], t1.float())
        assert torch.equal(p["w3"], w3.float().flatten(1)) and p["w1"].dtype == torch.float32 and p["b3"].dtype == torch.float32
        if project:
            wd, td = fold(unit.downsample[0], unit.downsample[1])
            assert torch.equal(p["wd"], wd.float()) and torch.equal(p["b3"], (t3 + td).float())
        else:
            assert "wd" not in p and torch.equal(p["b3"], t3.float())
        assert "s2" not in p and "t2" not in p and unit.gemm_params() is p                    # cached; bn2 is not in it
        scale2 = lambda: (unit.bn2.weight.detach().double() / torch.sqrt(unit.bn2.running_var.detach().double() + unit.bn2.eps)).float()
        s2, t2 = (t.clone() for t in unit.bn2.folded())
        assert torch.equal(s2, scale2())
        with torch.no_grad():
            unit.bn2.running_var.mul_(4.0)                                                      # bn2 ALONE, in place
        s2b, t2b = unit.bn2.folded()                                                            # what _forward_gemm hands to the split pass
        assert not torch.equal(s2b, s2) and torch.equal(s2b, scale2())
        assert not torch.equal(t2b, t2) and unit.gemm_params() is p                             # ... and nothing else was rebuilt
        key = unit._gemm[0]
        monkeypatch.setattr(r50, "SPLIT_GEMM", not r50.SPLIT_GEMM)
        p2 = unit.gemm_params()
        assert unit._gemm[0] != key and p2 is not p and torch.equal(p2["w1"], p["w1"])
        monkeypatch.setattr(r50, "SPLIT_GEMM", not r50.SPLIT_GEMM)
        for name in ("SPLIT_MIN_PLANES", "SPLIT_MIN_PLANES_3X3", "SPLIT_MIN_INPUT"):
            before = unit.gemm_params() and unit._gemm[0]
            monkeypatch.setattr(r50, name, getattr(r50, name) + 8)
            assert unit.gemm_params() is not None and unit._gemm[0] != before, name


def test_bottleneck_gemm_params_fold_batch_norm_into_weight_and_bias():
    """Bottleneck.gemm_params: conv -> FrozenBatchNorm == conv with (weight * scale) + shift, shortcut shift merged into conv3's
    bias; checked on the CPU against the module's own composed forward (reference net/resnet50.py:11-14, :34-54)."""
    import torch
    import torch.nn.functional as F
    from irn_amd.net import resnet50 as r50
    torch.manual_seed(0)
    for project in (False, True):
        c_in = 64 if project else 128
        unit = r50.Bottleneck(c_in, 32, stride=1, project=project).eval()
        for m in unit.modules():
            if isinstance(m, r50.FrozenBatchNorm):
                m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(); m.running_mean.normal_(); m.running_var.uniform_(0.5, 2.0)
        x = torch.randn(2, c_in, 8, 8)
        with torch.no_grad():
            want = unit(x)
            p = unit.gemm_params()
            y = F.relu(F.conv2d(x, p["w1"].view(32, c_in, 1, 1), p["b1"]))
            y = unit.bn2.apply_(unit.conv2(y), relu=True)
            sc = F.conv2d(x, p["wd"]) if project else x
            got = F.relu(F.conv2d(y, p["w3"].view(128, 32, 1, 1), p["b3"]) + sc)
        assert float((got - want).abs().max()) <= 1e-5
        assert unit.gemm_params() is p                          # cached while the parameters stand
        with torch.no_grad():
            unit.bn3.bias.add_(1.0)
        assert unit.gemm_params() is not p and not torch.equal(unit.gemm_params()["b3"], p["b3"])


def test_dataset_skips_the_pixels_when_the_step_says_so(tmp_path):
    """VOC12ClassificationDatasetMSF(raw=True, skip_image=...): an image the step will not need (its edge maps are on the device)
    comes as an empty uint8 tensor with the size from the file header; `device_images` maps it to None; `EdgeStore.peek` does not
    count.  (The reference decodes every image in both label steps, step/make_sem_seg_labels.py:24-34.)"""
    import numpy as np
    import torch
    from PIL import Image
    from torch.utils.data import default_collate
    from irn_amd.step import _common
    from irn_amd.voc12 import dataloader
    root = tmp_path / "voc" / "JPEGImages"
    root.mkdir(parents=True)
    for name, (h, w) in (("2008_000001", (30, 44)), ("2008_000002", (37, 21))):
        Image.fromarray((np.random.RandomState(0).rand(h, w, 3) * 255).astype(np.uint8)).save(root / (name + ".jpg"))
    (tmp_path / "train.txt").write_text("2008_000001\n2008_000002\n")
    np.save(tmp_path / "cls_labels.npy", {2008000001: np.eye(20, dtype=np.float32)[3], 2008000002: np.eye(20, dtype=np.float32)[5]})
    ds = dataloader.VOC12ClassificationDatasetMSF(str(tmp_path / "train.txt"), voc12_root=str(tmp_path / "voc"), raw=True,
                                                  skip_image=lambda name: name.endswith("2"))
    a, b = default_collate([ds[0]]), default_collate([ds[1]])
    assert a["img"].shape == (1, 30, 44, 3) and b["img"].numel() == 0
    assert (int(b["size"][0]), int(b["size"][1])) == (37, 21) and b["name"][0] == "2008_000002"
    assert _common.device_images(b, (1.0,)) is None
    _common.set_skip_image(torch.utils.data.Subset(ds, [0, 1]), None)
    assert ds.skip_image is None and ds[1]["img"].shape == (37, 21, 3)
    store = _common.EdgeStore()
    store.put("k", torch.zeros(1, 2, 2), torch.zeros(2, 2, 2))
    h0, m0 = store.hits, store.misses
    assert store.peek("k", torch.device("cpu")) and not store.peek("other", torch.device("cpu"))
    assert (store.hits, store.misses) == (h0, m0)


def test_run_sample_help_renders_and_deterministic_flag_reaches_the_environment(monkeypatch, tmp_path):
    """`run_sample.py --help` formats (a bare % in a help string used to crash argparse) and `--deterministic` sets the variable
    every process that sets MIOpen up reads (workers inherit it)."""
    import run_sample
    text = run_sample.build_parser().format_help()
    assert "--deterministic {0,1}" in text and "--edge_out_dir" in text and "--walk_accel {0,1}" in text
    a = run_sample.build_parser().parse_args(["--voc12_root", "x", "--deterministic", "0"])
    assert a.deterministic == 0 and run_sample.build_parser().parse_args(["--voc12_root", "x"]).deterministic is None


def test_instance_step_pipeline_order(monkeypatch):
    """make_ins_seg_labels._flush: per turn (1) the batch whose front half is enqueued gets its back half, (2) the new batch's IRNet
    forward + front half are enqueued, (3) the batch before is collected and written — every batch passes the three stages once
    and in order, the back half of batch k never queues behind the forward of batch k+1, three closing turns drain the pipe.
    (Reference loop: step/make_ins_seg_labels.py:119-152, one image at a time.)"""
    import argparse
    from irn_amd.step import _labels, make_ins_seg_labels as mis
    log = []
    monkeypatch.setattr(_labels, "edges_for", lambda model, pend, irn_batch, **kw: log.append(("irnet", tuple(p["name"] for p in pend))))
    monkeypatch.setattr(_labels, "edge_store_kw", lambda model, args: {})
    monkeypatch.setattr(mis, "instance_front", lambda items: log.append(("front", tuple(it["name"] for it in items))) or ("cmaps", "k_dev"))
    monkeypatch.setattr(mis, "instance_back", lambda walker, items, front, beta, exp_times, bg, deferred=False:
                        log.append(("back", tuple(it["name"] for it in items))) or "pending-%s" % items[0]["name"])
    monkeypatch.setattr(mis, "_write", lambda names, pending, args, writer: log.append(("write", tuple(names), pending)))
    args = argparse.Namespace(beta=10, exp_times=8, ins_seg_bg_thres=0.25, irn_batch=8)
    state = {}
    batches = [["a1", "a2"], ["b1", "b2"], ["c1"]]
    for b in batches:
        pend = [{"name": n} for n in b]
        mis._flush(None, None, pend, args, None, state)
        assert pend == []
    for _ in range(3):
        mis._flush(None, None, [], args, None, state)
    assert state == {"front": None, "emit": None}
    stages = [(kind, names[0][0]) for kind, names, *rest in log]
    # per batch: irnet -> front -> back -> write, once each
    for tag in "abc":
        assert [k for k, t in stages if t == tag] == ["irnet", "front", "back", "write"], (tag, stages)
    # the back half of a batch is enqueued BEFORE the next batch's forward (its small read-backs must not wait behind it)
    assert stages.index(("back", "a")) < stages.index(("irnet", "b")) < stages.index(("write", "a")) or \
        stages.index(("back", "a")) < stages.index(("irnet", "b"))
    assert stages.index(("back", "b")) < stages.index(("irnet", "c"))
    # a batch is collected one turn after its back half: its detections cross PCIe under the next batch's kernels
    assert stages.index(("write", "a")) > stages.index(("front", "b")) and stages.index(("write", "b")) > stages.index(("front", "c"))
    assert [w[2] for w in log if w[0] == "write"] == ["pending-a1", "pending-b1", "pending-c1"]


def test_label_step_batch_defaults():
    """step/_labels.irn_batch / walk_batch: 8 images per IRNet pass and the step's own walk batch (64 semantic, 32 instance)
    when the argument is absent or 0, the given value otherwise."""
    import argparse
    from irn_amd.step import _labels
    for args in (argparse.Namespace(), argparse.Namespace(irn_batch=0, walk_batch=0), argparse.Namespace(irn_batch=None, walk_batch=None)):
        assert _labels.irn_batch(args) == 8
        assert _labels.walk_batch(args, 64) == 64 and _labels.walk_batch(args, 32) == 32
    args = argparse.Namespace(irn_batch=3, walk_batch=5)
    assert _labels.irn_batch(args) == 3 and _labels.walk_batch(args, 64) == 5 and _labels.walk_batch(args, 32) == 5


def test_split_weight_operands_reconstruct_the_weight_to_22_bits_and_the_split_product_is_fp32_grade():
    """The host half of the split-precision convolutions (irn_amd/gemm.py split_weight[_3x3]; reference net/resnet50.py:34-54 with
    FixedBatchNorm folded in): [w_hi | w_lo | w_hi 2^-11] of w 2^p reconstructs w to 2^-22 of the layer's largest weight, every
    entry stays inside fp16's range, the taps of a 3x3 weight share one exponent in both operand layouts — and the product the GPU
    forms with them, emulated here in numpy (fp16 operands, exact products, wide accumulation), is as close to the exact one as a
    correctly rounded fp32 dot product."""
    from irn_amd import gemm, ops
    g = torch.Generator().manual_seed(4)
    for cout, cin, spread in ((64, 256, 1.0), (512, 128, 1e-3), (8, 16, 30.0)):
        w = torch.randn(cout, cin, generator=g).double() * spread * torch.rand(cout, 1, generator=g).double()
        b16, alpha = ops.split_weight(w)
        assert b16.dtype == torch.float16 and b16.shape == (cout, 3 * cin) and float(b16.float().abs().max()) < 2.0 ** 14
        hi, lo, his = b16[:, :cin].double(), b16[:, cin:2 * cin].double(), b16[:, 2 * cin:].double()
        # the scaled copy is exact for every weight above 2^-17 of the largest, and off by at most half a subnormal step below
        assert float((his - hi * 2.0 ** -11).abs().max()) <= 2.0 ** -25 and torch.equal(his[hi.abs() >= 0.125], (hi * 2.0 ** -11)[hi.abs() >= 0.125])
        rec = (hi + lo) * alpha
        assert float((rec - w).abs().max()) <= 2.0 ** -22 * float(w.abs().max())
        # the activation side as irn_split16 forms it, and the three-term product
        x = torch.relu(torch.randn(40, cin, generator=g)).float() * 5.0
        xh = x.to(torch.float16)
        xl = ((x - xh.float()) * 2048.0).to(torch.float16)
        a16 = torch.cat([xh, xh, xl], dim=1).double()
        got = alpha * (a16 @ b16.double().t())
        want = x.double() @ w.t()
        f32 = (x @ w.float().t()).double()
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 4e-7 * scale and float((got - want).abs().max()) <= 2.0 * float((f32 - want).abs().max()) + 1e-7 * scale
    w3 = torch.randn(16, 8, 3, 3, generator=g).double() * 0.1
    for fused, shape in ((False, (9, 16, 24)), (True, (3, 16, 72))):
        gemm.CONV3X3_ROW_FUSED, saved = fused, gemm.CONV3X3_ROW_FUSED
        try:
            t16, a3 = ops.split_weight_3x3(w3)
        finally:
            gemm.CONV3X3_ROW_FUSED = saved
        assert tuple(t16.shape) == shape
        taps = t16.view(3, 16, 3, 24).permute(0, 2, 1, 3).reshape(9, 16, 24) if fused else t16
        for t in range(9):
            rec = (taps[t][:, :8].double() + taps[t][:, 8:16].double()) * a3
            assert float((rec - w3[:, :, t // 3, t % 3]).abs().max()) <= 2.0 ** -22 * float(w3.abs().max())


def test_warmup_tool_picks_the_untuned_sizes_of_a_dataset(tmp_path):
    """tools/miopen_warmup.py --from-list: the (H, W) histogram of a list's images from their JPEG headers, most frequent first,
    minus what the shipped channels-last database covers, until the requested share of the images has a tuned size."""
    import argparse
    import importlib.util
    from PIL import Image
    root = tmp_path / "voc"
    (root / "JPEGImages").mkdir(parents=True)
    sizes = [(375, 500)] * 5 + [(300, 420)] * 3 + [(123, 77)] * 2 + [(64, 64)]
    names = []
    for i, (h, w) in enumerate(sizes):
        names.append("2011_%06d" % i)
        Image.new("RGB", (w, h)).save(root / "JPEGImages" / (names[-1] + ".jpg"))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    spec = importlib.util.spec_from_file_location("miopen_warmup", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "miopen_warmup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    shipped = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "irn_amd", "data", "miopen")
    a = argparse.Namespace(from_list=str(tmp_path / "list.txt"), voc12_root=str(root), coverage=0.9, max_sizes=40, out=shipped)
    assert mod.sizes_of_list(a) == "300x420,123x77"          # 375x500 is shipped; 8 + 2 of 11 images >= 90 %; 64x64 not needed
    a.coverage, a.max_sizes = 1.0, 1
    assert mod.sizes_of_list(a) == "300x420"
