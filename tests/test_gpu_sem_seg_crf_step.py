"""`--sem_seg_crf_iters` through make_sem_seg_labels and tune_sem_seg, on a 4-image VOC tree of two sizes with
random IRNet weights: with 0 nothing changes and the CRF is never called; with 10 every PNG is the composition
`label_epilogue(want_rw_up)` -> `crf_score_sweep` on the step's own walk outputs and decoded pixels, whatever the worker
layout and on the `--split_gemm auto` redo path; tune_sem_seg's grid points score what eval_sem_seg scores on those files."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _steps as S  # noqa: E402

pytestmark = pytest.mark.gpu

os.environ.setdefault("MIOPEN_FIND_MODE", "2")     # fast find: the backbone is plumbing here, not the subject

N_IMAGES = 4
THRES = 0.25


def _make_voc(tmp):
    """As tests/test_gpu_tune_sem_seg.py builds its tree: CAMs and ground truth from the same Gaussian blobs."""
    from irn_amd import synth
    rng = np.random.RandomState(0)
    specs = []
    for i in range(N_IMAGES):
        h, w = ((96, 128), (113, 150))[i % 2]
        k = 2 + i % 2
        keys = np.sort(rng.choice(20, k, replace=False)).astype(np.int64)
        cam = synth.cam_blobs(k, *synth.grid_of((h, w)), seed=40 + i)
        specs.append({"name": "2008_%06d" % (i + 1), "photo": synth.photo(h, w, seed=60 + i), "quality": 95, "keys": keys,
                      "cls": synth.blob_ground_truth(synth.upsample4(cam, (h, w)), keys, 0.45, 0.35)[0],
                      "cam": {"keys": torch.from_numpy(keys), "cam": torch.from_numpy(cam)}})
    return tmp / "voc", synth.write_voc_tree(tmp / "voc", specs, tmp / "lists" / "train.txt", cam_dir=tmp / "cam", cls_labels=20)


class _World:
    def __init__(self, tmp):
        from irn_amd.net import weights
        self.tmp = tmp
        self.root, self.names = _make_voc(tmp)
        torch.save(weights.random_irn_state(2), tmp / "res50_irn.pth")
        self.runs = {}

    def run(self, tag, extra, workers="0", shutdown=True):
        tmp = self.tmp
        sem = tmp / ("sem_" + tag)
        out = S.run_sample_main(["--voc12_root", str(self.root), "--infer_list", str(tmp / "lists" / "train.txt"), "--num_workers", "2",
                                 "--worker_devices", workers, "--irn_weights_name", str(tmp / "res50_irn.pth"),
                                 "--cam_out_dir", str(tmp / "cam"), "--sem_seg_out_dir", str(sem), "--ins_seg_out_dir", str(tmp / "ins"),
                                 "--log_name", str(tmp / "log"), "--make_cam_pass", "False", "--make_ins_seg_pass", "False"] + extra,
                                shutdown=shutdown)
        return sem, out

    def labels(self, tag, extra, **kw):
        """The label files of a configuration, written once per module."""
        if tag not in self.runs:
            self.runs[tag] = self.run(tag, extra, **kw)[0]
            assert sorted(os.listdir(self.runs[tag])) == [n + ".png" for n in self.names]
        return self.runs[tag]

    def png(self, sem, name):
        return np.asarray(Image.open(os.path.join(sem, name + ".png")))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from irn_amd.step import _common
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    try:
        yield _World(tmp_path_factory.mktemp("sem_seg_crf"))
    finally:
        _common.shutdown_workers()
        _common.EDGE_STORE.clear()
        _common.CAM_STORE.clear()


def _bytes(sem, name):
    with open(os.path.join(sem, name + ".png"), "rb") as f:
        return f.read()


def test_flag_at_zero_changes_no_byte_and_never_calls_the_crf(world, monkeypatch):
    from irn_amd import ops

    def boom(*a, **k):
        raise AssertionError("crf_score_sweep called with --sem_seg_crf_iters 0")

    monkeypatch.setattr(ops, "crf_score_sweep", boom)
    plain = world.labels("plain", [])
    zero = world.labels("zero", ["--sem_seg_crf_iters", "0"])
    for n in world.names:
        assert _bytes(plain, n) == _bytes(zero, n), n


def test_every_png_is_the_composition_on_the_steps_own_walk(world, monkeypatch):
    from irn_amd import ops
    from irn_amd.step import make_sem_seg_labels as M
    seen = {}
    real = M._start_copy

    def spy(batch, args):
        for i, n in enumerate(batch["names"]):       # (a fall-back re-run comes through here again and replaces the entry)
            seen[n] = (batch["rws"][i].clone(), batch["sizes"][i], batch["keys"][i].clone(), batch["rgbs"][i].clone())
        return real(batch, args)

    monkeypatch.setattr(M, "_start_copy", spy)
    world.runs.pop("on", None)                       # this run must come through the spy, whichever test ran first
    on = world.labels("on", ["--sem_seg_crf_iters", "10"])
    assert sorted(seen) == sorted(world.names)
    plain = world.labels("plain", [])
    changed = 0
    for n in world.names:
        rw, size, keys, rgb = seen[n]
        jpeg = np.asarray(Image.open(world.root / "JPEGImages" / (n + ".jpg")).convert("RGB"))
        assert np.array_equal(rgb.cpu().numpy(), jpeg), n                     # the CRF sees the pixels the IRNet saw
        up = ops.label_epilogue([rw], [size], THRES, want_labels=False, want_rw_up=True)["rw_up"][0]
        want = ops.crf_score_sweep(rgb, up, keys, [THRES], t=10)[0].cpu().numpy()
        got = world.png(on, n)
        assert got.dtype == np.uint8 and np.array_equal(got, want), n
        assert set(np.unique(got).tolist()) <= {0} | set((keys + 1).tolist())
        changed += int((got != world.png(plain, n)).sum())
    assert changed > 0, "the CRF changed no pixel of any image"


def test_one_and_two_workers_write_identical_files(world):
    one = world.labels("on", ["--sem_seg_crf_iters", "10"])
    two = world.labels("two", ["--sem_seg_crf_iters", "10"], workers="0,0")
    for n in world.names:
        assert _bytes(one, n) == _bytes(two, n), n


def test_tune_grid_points_equal_the_label_and_eval_steps(world):
    first, second = (10.0, 8, THRES), (6.0, 8, 0.4)
    want = {}
    for tag, (beta, exp_times, thres) in (("a", first), ("b", second)):
        want[tag] = world.run("tune_" + tag, ["--eval_sem_seg_pass", "True", "--beta", str(beta), "--exp_times", str(exp_times),
                                              "--sem_seg_bg_thres", str(thres), "--sem_seg_crf_iters", "10"])[1]["eval_sem_seg"]
    assert not np.array_equal(want["a"]["iou"], want["b"]["iou"], equal_nan=True)
    sem, got = world.run("tune", ["--make_sem_seg_pass", "False", "--tune_sem_seg_pass", "True", "--tune_beta", "6",
                                  "--tune_bg_thres", "0.4", "0.1", "--sem_seg_crf_iters", "10"])
    got = got["tune_sem_seg"]
    assert os.listdir(sem) == []
    assert set(got["grid"]) == {(b, 8, t) for b in (6.0, 10.0) for t in (0.1, THRES, 0.4)}
    assert np.array_equal(got["iou"], want["a"]["iou"], equal_nan=True) and got["miou"] == want["a"]["miou"]
    assert np.array_equal(got["ious"][first], want["a"]["iou"], equal_nan=True) and got["grid"][first] == want["a"]["miou"]
    assert np.array_equal(got["ious"][second], want["b"]["iou"], equal_nan=True) and got["grid"][second] == want["b"]["miou"]
    assert got["grid"][got["best"]] == max(got["grid"].values())
    # with the flag at 0 the grid is today's: the run without the flag, whose points are the T = 0 files' scores
    grid = ["--make_sem_seg_pass", "False", "--tune_sem_seg_pass", "True", "--tune_beta", "6", "--tune_bg_thres", "0.4", "0.1"]
    plain = world.run("tune_plain", grid)[1]["tune_sem_seg"]
    zero = world.run("tune_zero", grid + ["--sem_seg_crf_iters", "0"])[1]["tune_sem_seg"]
    assert plain["grid"] == zero["grid"] and plain["best"] == zero["best"]
    for point in plain["ious"]:
        assert np.array_equal(plain["ious"][point], zero["ious"][point], equal_nan=True), point
    off = world.run("tune_off", ["--eval_sem_seg_pass", "True"])[1]["eval_sem_seg"]
    assert np.array_equal(zero["ious"][first], off["iou"], equal_nan=True)
    assert not np.array_equal(zero["ious"][first], got["ious"][first], equal_nan=True)      # the CRF moves the scores


def test_split_gemm_auto_redoes_the_flagged_image_with_the_crf(tmp_path, monkeypatch):
    """One image forced over fp16's range the way tests/test_gpu_split_auto.py forces it (its tree, its raised IRNet checkpoint,
    its switches): under `--split_gemm auto` the image is redone on the fp32 GEMMs, and its file is the one a `--split_gemm 0` run
    writes — with the CRF on in both."""
    import test_gpu_split_auto as A
    from irn_amd import ops, synth
    from irn_amd.net import resnet50 as r50
    from irn_amd.step import _common, _report, make_sem_seg_labels
    for k in ("SPLIT_GEMM", "SPLIT_AUTO"):
        monkeypatch.setattr(r50, k, getattr(r50, k))
    monkeypatch.setenv("IRN_SPLIT_GEMM", os.environ.get("IRN_SPLIT_GEMM", "1"))
    monkeypatch.delenv("IRN_DETERMINISTIC", raising=False)
    monkeypatch.setattr(r50, "CHANNELS_LAST_MODE", "1")
    monkeypatch.setattr(r50, "SPLIT_MIN_PLANES", 64)
    monkeypatch.setattr(r50, "SPLIT_MIN_INPUT", 1 << 20)
    monkeypatch.setattr(r50, "SPLIT_MIN_ROWS_3X3", 1)
    monkeypatch.setattr(_report, "say", lambda s: None)
    root, all_list, _ = A._make_tree(tmp_path)
    A._checkpoint("irn", root, all_list, str(tmp_path / "res50_irn.pth"))
    os.makedirs(tmp_path / "cam")
    for i, name in enumerate(A.NAMES):
        np.save(tmp_path / "cam" / (name + ".npy"),
                {"keys": torch.tensor([2 + i, 11]), "cam": torch.from_numpy(synth.cam_blobs(2, *synth.grid_of((A.H, A.W)), seed=i))})

    def run(mode, tag):
        r50.set_split_mode(mode)
        _common.EDGE_STORE.clear()
        _common.CAM_STORE.clear()
        a = argparse.Namespace(num_workers=0, voc12_root=str(root), infer_list=all_list, irn_network="net.resnet50_irn",
                               irn_weights_name=str(tmp_path / "res50_irn.pth"), beta=10, exp_times=8, sem_seg_bg_thres=THRES,
                               sem_seg_crf_iters=10, cam_out_dir=str(tmp_path / "cam"), sem_seg_out_dir=str(tmp_path / tag))
        n0 = _report.worker_stats()["split_fallback_images"]
        make_sem_seg_labels.run(a)
        return a.sem_seg_out_dir, _report.worker_stats()["split_fallback_images"] - n0

    try:
        ops.split_overflowed()
        fp32, n_fp32 = run("0", "fp32")
        auto, n_auto = run("auto", "auto")
        assert n_fp32 == 0 and n_auto == 1
        assert sorted(os.listdir(auto)) == [n + ".png" for n in A.NAMES]
        assert A._same_png(auto, fp32, A.NOISE)
        assert np.unique(np.asarray(Image.open(os.path.join(auto, A.NOISE + ".png")))).size >= 2
    finally:
        _common.EDGE_STORE.clear()
        _common.CAM_STORE.clear()
        ops.split_overflowed()
