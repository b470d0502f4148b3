"""ops.crf_label_sweep / ops.ir_label_confusion (irn_amd/csrc/crf.hip, eval.hip) and step/tune_ir_label.py on the GPU.

The sweep's planes equal single CRF calls BIT FOR BIT (a CRF's result does not depend on what shares its filter pass, so
neither the chunking nor the shared lattices may show); the counting kernel equals a numpy count of the combined maps cell for
cell; the step's scores at a grid point are exactly those of the PNGs cam_to_ir_label writes there.  Only the one comparison
with the float64 restatement uses the tie rule of tests/test_gpu_crf.py (restated here)."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _densecrf_ref as R  # noqa: E402
import _eval_ref as E  # noqa: E402
import _steps as S  # noqa: E402

pytestmark = pytest.mark.gpu

TIE_TOL = 1e-4          # tests/_parity.py: Q within 1e-4 max-abs of the restatement => only ties at that level can flip an argmax


def _dev():
    return torch.device("cuda", 0)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _case(h, w, k, seed):
    from irn_amd import synth
    keys = np.sort(np.random.RandomState(seed).choice(20, k, replace=False)) if k <= 20 else np.arange(k)
    return synth.photo(h, w, seed=seed), synth.cam_blobs(k, h, w, seed=seed), keys.astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,n_t", [(1, 16), (3, 5), (20, 4), (31, 3)])      # chunks of 16 | 5 | 3 + 1 | 2 + 1 CRFs
@pytest.mark.parametrize("h,w", [(64, 48), (97, 131)])
def test_sweep_equals_single_calls_bit_for_bit(h, w, k, n_t):
    from irn_amd import ops
    img, cams, keys = _case(h, w, k, seed=h + k)
    thres = np.linspace(0.05, 0.8, n_t).astype(np.float32)
    planes = ops.crf_label_sweep(_gpu(img), _gpu(cams), keys, thres)
    assert planes.dtype == torch.uint8 and tuple(planes.shape) == (n_t, h, w) and planes.is_cuda
    again = ops.crf_label_sweep(_gpu(img), _gpu(cams), keys, thres).cpu().numpy()
    planes = planes.cpu().numpy()
    assert np.array_equal(planes, again)
    pad = np.pad(keys + 1, (1, 0))
    for i, thr in enumerate(thres):
        lab = ops.crf_inference_label(_gpu(img), _gpu(R.seed_labels(cams, thr)), n_labels=k + 1).cpu().numpy()
        assert np.array_equal(planes[i], pad[lab]), (h, w, k, i)
    for i in range(n_t):
        for j in range(n_t):
            want = ops.crf_ir_label(_gpu(img), _gpu(cams), keys, thres[i], thres[j]).cpu().numpy()
            assert np.array_equal(R.combine(planes[i], planes[j]), want), (h, w, k, i, j)
    assert len(np.unique(planes)) >= 2 and (planes != planes[0]).any()        # not vacuous: the planes differ


@pytest.mark.parametrize("h,w", [(1, 1), (7, 5)])
def test_sweep_small_images_one_threshold_and_no_keys(h, w):
    from irn_amd import ops
    img, cams, keys = _case(h, w, 2, seed=3)
    planes = ops.crf_label_sweep(_gpu(img), _gpu(cams), keys, [0.05, 0.3]).cpu().numpy()
    one = ops.crf_label_sweep(_gpu(img), _gpu(cams), keys, [0.3]).cpu().numpy()            # T = 1
    assert one.shape == (1, h, w) and np.array_equal(one[0], planes[1])
    assert np.array_equal(R.combine(planes[1], planes[0]), ops.crf_ir_label(_gpu(img), _gpu(cams), keys, 0.3, 0.05).cpu().numpy())
    out = torch.full((3, h, w), 9, dtype=torch.uint8, device=_dev())
    got = ops.crf_label_sweep(_gpu(img), torch.zeros((0, h, w), device=_dev()), np.zeros(0, np.int64), [0.1, 0.2, 0.3], out=out)
    assert got is out and not out.any()                                                   # k = 0: zeros, no workspace


def test_sweep_without_keys_needs_no_workspace():
    import ctypes as C
    from irn_amd import _lib
    h, w = 5, 6
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device=_dev())
    planes = torch.full((2, h, w), 7, dtype=torch.uint8, device=_dev())
    th = (C.c_float * 2)(0.1, 0.2)
    rc = _lib.lib.irn_crf_label_sweep(rgb.data_ptr(), None, None, 0, h, w, th, 2, 10, 0.7, planes.data_ptr(), None, 0,
                                      _lib._stream())
    assert rc == 0 and not planes.any()
    cams = torch.zeros((1, h, w), device=_dev())
    keys = torch.zeros(1, dtype=torch.int64, device=_dev())
    ws = torch.empty(1024, dtype=torch.uint8, device=_dev())
    rc = _lib.lib.irn_crf_label_sweep(rgb.data_ptr(), cams.data_ptr(), keys.data_ptr(), 1, h, w, th, 2, 10, 0.7,
                                      planes.data_ptr(), ws.data_ptr(), ws.numel(), _lib._stream())
    assert rc == 3 and b"workspace" in _lib.lib.irn_last_error()                          # IRN_ERR_STATE


def _threshold_cams(h, w, k, thres, seed):
    """The construction of tests/test_gpu_crf.py's _threshold_cams for any number of thresholds: CAMs on a floor of 0.01
    whose interesting entries sit exactly on, one ulp below and one ulp above each threshold (and at 0.7); pixel p takes
    scenario p mod 2V: one class at the value, or (second half, k > 1) two classes tied at it."""
    f32 = np.float32
    vals = [v for t in thres for v in (f32(t), np.nextafter(f32(t), f32(-1)), np.nextafter(f32(t), f32(1)))] + [f32(0.7)]
    rng = np.random.RandomState(seed)
    cams = np.full((k, h * w), 0.01, f32)
    for p in range(h * w):
        s = p % (2 * len(vals))
        c1 = int(rng.randint(k))
        cams[c1, p] = vals[s % len(vals)]
        if s >= len(vals) and k > 1:
            cams[(c1 + 1 + int(rng.randint(k - 1))) % k, p] = vals[s % len(vals)]
    return cams.reshape(k, h, w), len(vals)


@pytest.mark.parametrize("k", [1, 3, 20])
@pytest.mark.parametrize("h,w", [(7, 5), (64, 48)])
def test_sweep_seed_rules_exact_without_iterations(h, w, k):
    """t = 0: a plane is a pure function of the seeds (strict >, the first of two tied classes wins), the unary softmax and
    the argmax through the keys."""
    from irn_amd import ops, synth
    thres = np.float32([0.05, 0.2, 0.3, 0.5])
    cams, n_vals = _threshold_cams(h, w, k, thres, seed=h + k)
    keys = np.sort(np.random.RandomState(k).choice(20, k, replace=False)).astype(np.int64)
    planes = ops.crf_label_sweep(_gpu(synth.photo(h, w, seed=3)), _gpu(cams), keys, thres, t=0).cpu().numpy()
    pad = np.pad(keys + 1, (1, 0))
    scen = (np.arange(h * w) % (2 * n_vals)) % n_vals
    for i, thr in enumerate(thres):
        seed = R.seed_labels(cams, thr)
        assert np.array_equal(planes[i], pad[seed]), (h, w, k, i)
        flat = planes[i].reshape(-1)
        assert (flat[np.isin(scen, (3 * i, 3 * i + 1))] == 0).all()               # on the threshold or below it: background
        assert (flat[scen == 3 * i + 2] > 0).all()                                # one ulp above: a class
        fg = seed.reshape(-1) > 0
        assert np.array_equal(seed.reshape(-1)[fg], np.argmax(cams.reshape(k, -1)[:, fg] > thr, axis=0) + 1)   # the first class wins


def _conf_ties(got, want, qs, what):
    """tests/test_gpu_crf.py's rule: pixels of the ir-label map that differ must be ties of the fg or the bg CRF's Q."""
    diff = got != want
    if not diff.any():
        return
    h, w = want.shape
    gaps = []
    for q in qs:
        s = np.sort(q.reshape(q.shape[0], h, w)[:, diff], axis=0)
        gaps.append(s[-1] - s[-2])
    gap = np.minimum(gaps[0], gaps[1])
    assert float(gap.max()) < TIE_TOL, "%s: %d pixels differ, one is not a tie (gap %.3g)" % (what, int(diff.sum()), float(gap.max()))


def test_sweep_vs_restatement():
    from irn_amd import ops
    h, w, k = 120, 160, 2
    img, cams, keys = _case(h, w, k, seed=8)
    thres = (0.05, 0.2, 0.3)
    planes = ops.crf_label_sweep(_gpu(img), _gpu(cams), keys, thres).cpu().numpy()
    kern = R.Kernels(img)                             # R.ir_label with the kernels and the shared CRFs built once
    pad = np.pad(keys + 1, (1, 0))
    qs = [R.inference(img, R.seed_labels(cams, t), 10, k + 1, 0.7, np.float64, kern) for t in thres]
    maps = [pad[np.argmax(q, axis=0).reshape(h, w)] for q in qs]
    for i, j in ((2, 0), (1, 0)):
        _conf_ties(R.combine(planes[i], planes[j]), R.combine(maps[i], maps[j]), (qs[i], qs[j]), "fg %g bg %g" % (thres[i], thres[j]))


# ---------------------------------------------------------------------------------------------------------------------
# the counting kernel
# ---------------------------------------------------------------------------------------------------------------------

def _hist22(gt, label):
    """One image's [22,22] count: row = GT (21 = 255), column = label (21 = 255)."""
    r = np.where(gt == 255, 21, gt).astype(np.int64).reshape(-1)
    c = np.where(label == 255, 21, label).astype(np.int64).reshape(-1)
    return np.bincount(r * 22 + c, minlength=484).reshape(22, 22)


def _grid_hist(planes, fg_idx, bg_idx, gt, keep=None):
    out = np.zeros((len(fg_idx), len(bg_idx), 22, 22), np.int64)
    keep = np.ones(gt.shape, bool) if keep is None else keep
    for i, a in enumerate(fg_idx):
        for j, b in enumerate(bg_idx):
            out[i, j] = _hist22(gt[keep], R.combine(planes[a], planes[b])[keep])
    return out


def _random_planes(n_t, h, w, seed):
    rng = np.random.RandomState(seed)
    keys = np.sort(rng.choice(20, 4, replace=False))
    planes = np.where(rng.rand(n_t, h, w) < 0.5, 0, (keys + 1)[rng.randint(4, size=(n_t, h, w))]).astype(np.uint8)
    gt = rng.randint(0, 21, size=(h, w)).astype(np.uint8)
    gt[h // 3:h // 3 + max(h // 8, 1) if h > 2 else 0] = 255            # a void band (none in the 1x1 image)
    return planes, gt


GRIDS = {"1x1": (6, [4], [1]), "3x4": (6, [5, 0, 5], [1, 2, 0, 3]), "16x16": (16, list(range(16)), list(range(15, -1, -1)))}


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("h,w", [(1, 1), (7, 5), (64, 48), (375, 500)])
def test_confusion_equals_numpy_and_accumulates(h, w, grid):
    from irn_amd import ops
    n_t, fg_idx, bg_idx = GRIDS[grid]
    planes, gt = _random_planes(n_t, h, w, seed=h + n_t)
    want = _grid_hist(planes, fg_idx, bg_idx, gt)
    hist, bad = ops.ir_label_confusion(_gpu(planes), fg_idx, bg_idx, _gpu(gt))
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (len(fg_idx), len(bg_idx), 22, 22)
    assert np.array_equal(hist.cpu().numpy(), want) and int(bad.item()) == 0
    assert int(want[0, 0].sum()) == h * w
    h2, b2 = ops.ir_label_confusion(_gpu(planes), fg_idx, bg_idx, _gpu(gt), hist, bad)
    assert h2 is hist and b2 is bad and np.array_equal(hist.cpu().numpy(), 2 * want) and int(bad.item()) == 0
    if h * w >= 64 * 48:                                   # not vacuous: unsure pixels, several labels, the void row
        cols = want.sum(axis=(0, 1, 2))
        assert cols[21] > 0 and (cols[1:21] > 0).sum() >= 3 and cols[0] > 0 and want[:, :, 21].sum() > 0
        assert len({want[i, j].tobytes() for i in range(len(fg_idx)) for j in range(len(bg_idx))}) >= min(2, len(fg_idx) * len(bg_idx))


def test_confusion_skips_out_of_range_pixels_for_every_pair():
    from irn_amd import ops
    h, w = 64, 48
    planes, gt = _random_planes(6, h, w, seed=5)
    gt[10, 11] = 37
    planes[3, 40, 7] = 21
    keep = np.ones((h, w), bool)
    keep[10, 11] = keep[40, 7] = False
    fg_idx, bg_idx = [5, 0, 3], [1, 2]
    hist, bad = ops.ir_label_confusion(_gpu(planes), fg_idx, bg_idx, _gpu(gt))
    assert int(bad.item()) == 2
    clean = planes.copy()
    clean[3, 40, 7] = 0
    assert np.array_equal(hist.cpu().numpy(), _grid_hist(clean, fg_idx, bg_idx, gt, keep))
    assert (hist.cpu().numpy().sum(axis=(2, 3)) == h * w - 2).all()


def test_confusion_of_an_all_void_ground_truth_fills_only_row_21():
    from irn_amd import ops
    planes, _ = _random_planes(6, 64, 48, seed=6)
    hist, bad = ops.ir_label_confusion(_gpu(planes), [0, 1], [2], _gpu(np.full((64, 48), 255, np.uint8)))
    hist = hist.cpu().numpy()
    assert int(bad.item()) == 0 and not hist[:, :, :21].any() and (hist[:, :, 21].sum(axis=2) == 64 * 48).all()


# ---------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------

def _make_voc(tmp, n, no_keys=()):
    """JPEGs, CAM files (`high_res` at image size) and ground truth of n images, built like _make_voc of
    tests/test_gpu_tune_sem_seg.py: CAMs and GT come from the same Gaussian blobs (2-3 classes per image, a void band where the
    blobs fade).  Images listed in `no_keys` get a CAM file without class keys."""
    from irn_amd import synth
    rng = np.random.RandomState(0)
    specs = []
    for i in range(n):
        h, w = ((96, 128), (113, 150))[i % 2]
        k = 2 + i % 2
        keys = np.sort(rng.choice(20, k, replace=False)).astype(np.int64)
        cam = synth.cam_blobs(k, h, w, seed=40 + i)
        gt = synth.blob_ground_truth(cam, keys, 0.4, 0.32)[0]
        if i in no_keys:
            keys, cam = keys[:0], cam[:0]
        specs.append({"name": "2008_%06d" % (i + 1), "photo": synth.photo(h, w, seed=60 + i), "quality": 95, "keys": keys, "cls": gt,
                      "cam": {"keys": keys, "high_res": cam}})
    return tmp / "voc", synth.write_voc_tree(tmp / "voc", specs, tmp / "lists" / "train.txt", cam_dir=tmp / "cam")


def _run(tmp_path, root, ir_dir, extra):
    lst = str(tmp_path / "lists" / "train.txt")
    return S.run_sample_main(["--voc12_root", str(root), "--train_list", lst, "--infer_list", lst, "--num_workers", "2",
                              "--worker_devices", "0", "--cam_out_dir", str(tmp_path / "cam"), "--ir_label_out_dir", str(ir_dir),
                              "--sem_seg_out_dir", str(tmp_path / "sem"), "--ins_seg_out_dir", str(tmp_path / "ins"),
                              "--log_name", str(tmp_path / "log"), "--make_cam_pass", "False", "--make_ins_seg_pass", "False",
                              "--make_sem_seg_pass", "False"] + extra)


def _read_gt(root, name):
    return np.asarray(Image.open(os.path.join(root, "SegmentationClass", name + ".png")))


def _count_pngs(root, names, ir_dir):
    total = np.zeros((22, 22), np.int64)
    for n in names:
        total += _hist22(_read_gt(root, n), np.asarray(Image.open(os.path.join(ir_dir, n + ".png"))))
    return total


def _files(tmp):
    return sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs if not f.endswith(".log"))


def test_step_grid_points_equal_the_counted_pngs(tmp_path, capsys):
    from irn_amd.misc import evaluation
    root, names = _make_voc(tmp_path, 6, no_keys=(4,))
    first, second = (0.30, 0.05), (0.45, 0.15)
    want = {}
    for tag, (fg, bg) in (("a", first), ("b", second)):
        out = tmp_path / ("ir_" + tag)
        _run(tmp_path, root, out, ["--cam_to_ir_label_pass", "True", "--conf_fg_thres", str(fg), "--conf_bg_thres", str(bg)])
        assert sorted(os.listdir(out)) == [n + ".png" for n in names]
        want[tag] = _count_pngs(root, names, out)
    assert not np.asarray(Image.open(tmp_path / "ir_a" / (names[4] + ".png"))).any()           # no keys: all background
    assert want["a"][:, 21].sum() > 0 and (want["a"][:21, 1:21].sum(axis=0) > 0).sum() >= 3 and want["a"][21].sum() > 0
    before = _files(tmp_path)
    capsys.readouterr()
    got = _run(tmp_path, root, tmp_path / "ir_tune", ["--tune_ir_label_pass", "True", "--tune_conf_fg_thres", "0.45",
                                                      "--tune_conf_bg_thres", "0.15"])
    printed = capsys.readouterr().out
    assert set(got) == {"tune_ir_label"}
    got = got["tune_ir_label"]
    assert _files(tmp_path) == before and not (tmp_path / "ir_tune").exists()                  # it writes nothing
    points = [(f, b) for f in (0.3, 0.45) for b in (0.05, 0.15)]
    assert list(got["grid"]) == points and list(got["scores"]) == points and got["hist"].shape == (2, 2, 22, 22)
    assert np.array_equal(got["hist"][0, 0], want["a"]) and np.array_equal(got["hist"][1, 1], want["b"])
    for point, h22 in ((first, want["a"]), (second, want["b"])):
        s, ref = got["scores"][point], evaluation.ir_label_scores(h22)
        conf = h22[:21, :21]
        iou = E.iou_of(conf[:len(ref["iou"]), :len(ref["iou"])])
        assert np.array_equal(s["iou"], iou, equal_nan=True)
        assert s["coverage"] == conf.sum() / h22[:21].sum() and 0 < s["coverage"] < 1
        d = np.diag(conf)
        with np.errstate(invalid="ignore"):
            assert s["miou_all"] == np.nanmean(d / (h22[:21].sum(axis=1) + conf.sum(axis=0) - d)) == got["grid"][point]
    assert np.array_equal(got["iou"], got["scores"][first]["iou"], equal_nan=True) and got["miou_all"] == got["grid"][first]
    assert len({got["hist"][i, j].tobytes() for i in range(2) for j in range(2)}) == 4         # the points do not score alike
    assert len({(s["miou"], s["coverage"], s["miou_all"]) for s in got["scores"].values()}) >= 2
    lines = [ln for ln in printed.splitlines() if ln.startswith(("fg ", "best "))]
    assert len(lines) == 5 and lines[-1].startswith("best fg %g bg %g " % got["best"])
    assert [ln.startswith("fg %g bg %g miou " % p) for ln, p in zip(lines, points)] == [True] * 4
    assert got["grid"][got["best"]] == max(got["grid"].values())
    assert lines[-1] == "best " + lines[points.index(got["best"])]


def test_step_counts_an_image_without_class_keys_as_background(tmp_path):
    import argparse
    from irn_amd.step import tune_ir_label
    root, names = _make_voc(tmp_path, 2, no_keys=(1,))
    args = argparse.Namespace(voc12_root=str(root), chainer_eval_set="train", cam_out_dir=str(tmp_path / "cam"), num_workers=0,
                              conf_fg_thres=0.3, conf_bg_thres=0.05, tune_conf_fg_thres=[], tune_conf_bg_thres=[0.05])
    (root / "ImageSets" / "Segmentation" / "first.txt").write_text(names[0] + "\n")
    got = tune_ir_label.run(args)
    with_keys = tune_ir_label.run(argparse.Namespace(**dict(vars(args), chainer_eval_set="first")))
    gt = _read_gt(root, names[1])
    assert got["hist"].shape == (1, 1, 22, 22)
    assert np.array_equal(got["hist"][0, 0] - with_keys["hist"][0, 0], _hist22(gt, np.zeros_like(gt)))
    assert with_keys["hist"][0, 0][:, 1:].sum() > 0
