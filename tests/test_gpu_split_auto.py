"""`--split_gemm auto` through the steps (irn_amd/step/make_cam.py, make_sem_seg_labels.py, make_ins_seg_labels.py, _split_auto.py),
in-process step path, reproducible mode: an image's files depend on that image alone.

Tree: one high-contrast noise image and two flat grey ones, 96 x 80.  CAM and IRNet networks carry seeded random weights in
which ONE unit (layer1.1 of the trunk, 64 planes: its conv3 operand is bn2 + ReLU + split in one pass) has bn2's scale and shift
raised by a factor f and bn3 compensated (running mean times f, scale over f), so the network is the same function and only
what that unit's split pass is handed grows by f.  f comes from a CPU forward of the composed modules, image by image: the noise
image is handed at least 2 x 65504, every flat image (and, for the IRNet, whose tuned passes carry zero fill rows, the zero image)
at most 65504 / 2 — asserted before anything runs on the GPU.

  make_cam auto                the noise image's file is the `--split_gemm 0` run's, bit for bit; the flat images' files are those of a
                               `--split_gemm 1` run on the flat images alone; no raise; one fallback image, named in the report line
  make_sem_seg / make_ins_seg  same process (device CAMs and edge maps live), IRNet treated the same way: the flagged image's PNG and
                               instance file are the 0 chain's, the others the 1 chain's
  lag                          make_cam auto with the device kept busy in front of every flush: the flags are read behind their copy
  baseline                     `--split_gemm 1` on the whole tree still raises at the end of the step, naming IRN_SPLIT_GEMM=0"""
import argparse
import math
import os
import sys
import time

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lag  # noqa: E402

pytestmark = pytest.mark.gpu

os.environ.setdefault("MIOPEN_FIND_MODE", "2")     # fast find: the backbones are plumbing here, not the subject

FP16_MAX = 65504.0
H, W = 80, 96
SCALES = (1.0, 0.5)
NOISE, FLAT = "2008_000001", ["2008_000002", "2008_000003"]
NAMES = [NOISE] + FLAT
CAM_SEED, IRN_SEED = 1, 2


class _Stop(Exception):
    pass


def _make_tree(tmp):
    """-> (voc root, list of all three images, list of the flat ones)."""
    root = tmp / "voc"
    (root / "JPEGImages").mkdir(parents=True)
    rng = np.random.RandomState(0)
    pixels = {NOISE: (rng.rand(H, W, 3) > 0.5).astype(np.uint8) * 255, FLAT[0]: np.full((H, W, 3), 120, np.uint8),
              FLAT[1]: np.full((H, W, 3), 136, np.uint8)}
    labels = {}
    for i, name in enumerate(NAMES):
        Image.fromarray(pixels[name]).save(root / "JPEGImages" / (name + ".jpg"), quality=95)
        lab = np.zeros(20, np.float32)
        lab[[2 + i, 11]] = 1
        labels[int(name.replace("_", ""))] = lab
    (tmp / "lists").mkdir()
    (tmp / "lists" / "all.txt").write_text("\n".join(NAMES) + "\n")
    (tmp / "lists" / "flat.txt").write_text("\n".join(FLAT) + "\n")
    np.save(tmp / "lists" / "cls_labels.npy", labels)
    return root, str(tmp / "lists" / "all.txt"), str(tmp / "lists" / "flat.txt")


def _handed(net, unit, x):
    """Largest magnitude the split pass of `unit` is handed — conv3's input = relu(bn2(conv2(.))) — when `net` sees `x`; the
    forward (CPU, fp32, composed modules) ends there."""
    top = []

    def hook(module, inputs):
        top.append(float(inputs[0].abs().max()))
        raise _Stop()

    h = unit.conv3.register_forward_pre_hook(hook)
    try:
        with torch.no_grad():
            net(x)
    except _Stop:
        pass
    finally:
        h.remove()
    assert len(top) == 1 and math.isfinite(top[0])
    return top[0]


def _maxima(net, unit, root, list_path, scales, with_zero):
    """name -> the largest value handed over all scales (image and flip travel together); "zero": the fill row of a tuned pass."""
    from irn_amd.voc12 import dataloader
    ds = dataloader.VOC12ClassificationDatasetMSF(list_path, voc12_root=str(root), scales=scales, raw=False)
    out = {}
    for i in range(len(ds)):
        item = ds[i]
        name = item["name"] if isinstance(item["name"], str) else dataloader.decode_int_filename(item["name"])
        imgs = item["img"] if isinstance(item["img"], list) else [item["img"]]          # one scale: the pair itself
        out[name] = max(_handed(net, unit, torch.from_numpy(np.ascontiguousarray(t))) for t in imgs)
    if with_zero:
        out["zero"] = _handed(net, unit, torch.zeros(2, 3, H, W))
    return out


def _checkpoint(kind, root, list_path, path):
    """The seeded network of `kind` with its layer1.1 raised as the module docstring says, saved at `path`; the maxima before and after."""
    from irn_amd.net import resnet50_cam, resnet50_irn, weights
    net = weights._fill(resnet50_cam.CAM() if kind == "cam" else resnet50_irn.EdgeDisplacement(), CAM_SEED if kind == "cam" else IRN_SEED).eval()
    unit = net.resnet50.layer1[1]
    scales = SCALES if kind == "cam" else (1.0,)
    before = _maxima(net, unit, root, list_path, scales, kind == "irn")
    quiet = max(v for k, v in before.items() if k != NOISE)
    assert before[NOISE] >= 4.0 * quiet > 0, ("the seeded weights do not separate the images by a factor of 4", kind, before)
    # f: the geometric mean of the smallest factor that lifts the noise image to 2 x 65504 and the largest that keeps the others at 65504 / 2
    f = math.sqrt((2 * FP16_MAX / before[NOISE]) * (FP16_MAX / 2 / quiet))
    with torch.no_grad():
        unit.bn2.weight.mul_(f), unit.bn2.bias.mul_(f)
        unit.bn3.running_mean.mul_(f), unit.bn3.weight.div_(f)
    after = _maxima(net, unit, root, list_path, scales, kind == "irn")
    print("split auto (%s): handed to layer1.1's split pass before %s, factor %.4g, after %s" % (kind, before, f, after))
    assert after[NOISE] >= 2 * FP16_MAX, (kind, after)
    assert all(v <= FP16_MAX / 2 for k, v in after.items() if k != NOISE), (kind, after)
    torch.save(net.state_dict(), path)


def _load_cam(d, name):
    x = np.load(os.path.join(d, name + ".npy"), allow_pickle=True).item()
    return x["keys"], x["cam"], torch.from_numpy(x["high_res"])


def _same_cam(a, b, name):
    (ka, ca, ha), (kb, cb, hb) = _load_cam(a, name), _load_cam(b, name)
    return torch.equal(ka, kb) and torch.equal(ca.view(torch.int32), cb.view(torch.int32)) and torch.equal(ha.view(torch.int32), hb.view(torch.int32))


def _same_png(a, b, name):
    return np.array_equal(np.asarray(Image.open(os.path.join(a, name + ".png"))), np.asarray(Image.open(os.path.join(b, name + ".png"))))


def _same_ins(a, b, name):
    pa, pb = (os.path.join(d, name + ".npy") for d in (a, b))
    if not os.path.exists(pa) or not os.path.exists(pb):
        return os.path.exists(pa) == os.path.exists(pb)              # an image without a detection has no file, in either chain
    x, y = (np.load(p, allow_pickle=True).item() for p in (pa, pb))
    return (set(x) == set(y) == {"score", "mask", "class"} and np.array_equal(x["class"], y["class"]) and np.array_equal(x["mask"], y["mask"])
            and np.array_equal(np.asarray(x["score"], np.float32).view(np.int32), np.asarray(y["score"], np.float32).view(np.int32)))


class _World:
    """The tree, the two checkpoints and the switches of every run in this module; `run(mode, ...)` is one chain of steps."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.root, self.all_list, self.flat_list = _make_tree(tmp)
        _checkpoint("cam", self.root, self.all_list, str(tmp / "res50_cam.pth"))
        _checkpoint("irn", self.root, self.all_list, str(tmp / "res50_irn.pth"))
        self.said = []

    def args(self, tag, list_path):
        tmp = self.tmp
        a = argparse.Namespace(
            num_workers=0, voc12_root=str(self.root), train_list=list_path, infer_list=list_path, cam_network="net.resnet50_cam",
            cam_weights_name=str(tmp / "res50_cam"), cam_scales=SCALES, irn_network="net.resnet50_irn",
            irn_weights_name=str(tmp / "res50_irn.pth"), beta=10, exp_times=8, sem_seg_bg_thres=0.25, ins_seg_bg_thres=0.25,
            cam_out_dir=str(tmp / tag / "cam"), sem_seg_out_dir=str(tmp / tag / "sem"), ins_seg_out_dir=str(tmp / tag / "ins"))
        for d in (a.cam_out_dir, a.sem_seg_out_dir, a.ins_seg_out_dir):
            os.makedirs(d, exist_ok=True)
        return a

    def run(self, mode, tag, list_path, steps=("cam", "sem", "ins")):
        """One chain with IRN_SPLIT_GEMM = mode, every hand-off store of an earlier chain forgotten -> (args, fallback images per step)."""
        from irn_amd.net import resnet50 as r50
        from irn_amd.step import _common, _report, make_cam, make_ins_seg_labels, make_sem_seg_labels
        r50.set_split_mode(mode)
        _common.EDGE_STORE.clear()
        _common.CAM_STORE.clear()
        a = self.args(tag, list_path)
        counts = {}
        for s in steps:
            n0 = _report.worker_stats()["split_fallback_images"]
            {"cam": make_cam, "sem": make_sem_seg_labels, "ins": make_ins_seg_labels}[s].run(a)
            counts[s] = _report.worker_stats()["split_fallback_images"] - n0
        return a, counts


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Switches of the existing range test so that these sizes take the split path, channels-last forced; everything put back."""
    from irn_amd import ops
    from irn_amd.net import resnet50 as r50
    from irn_amd.step import _common, _report
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mp = pytest.MonkeyPatch()
    try:
        for k in ("SPLIT_GEMM", "SPLIT_AUTO"):
            mp.setattr(r50, k, getattr(r50, k))
        mp.setenv("IRN_SPLIT_GEMM", os.environ.get("IRN_SPLIT_GEMM", "1"))
        mp.delenv("IRN_DETERMINISTIC", raising=False)          # the reproducible mode is the default
        mp.setattr(r50, "CHANNELS_LAST_MODE", "1")
        mp.setattr(r50, "SPLIT_MIN_PLANES", 64)
        mp.setattr(r50, "SPLIT_MIN_INPUT", 1 << 20)
        mp.setattr(r50, "SPLIT_MIN_ROWS_3X3", 1)
        w = _World(tmp_path_factory.mktemp("split_auto"))
        mp.setattr(_report, "say", w.said.append)
        ops.split_overflowed()
        w.fp32 = w.run("0", "fp32", w.all_list)
        w.split = w.run("1", "split_flat", w.flat_list)
        w.said.clear()
        w.auto = w.run("auto", "auto", w.all_list)
        w.auto_said = list(w.said)
        yield w
    finally:
        _common.EDGE_STORE.clear()
        _common.CAM_STORE.clear()
        ops.split_overflowed()
        mp.undo()


def test_make_cam_auto_writes_fp32_files_for_the_flagged_image_only(world):
    (fp32, c0), (split, c1), (auto, ca) = world.fp32, world.split, world.auto
    assert c0["cam"] == 0 and c1["cam"] == 0 and ca["cam"] == 1
    assert _same_cam(auto.cam_out_dir, fp32.cam_out_dir, NOISE), "the flagged image is the --split_gemm 0 run's, bit for bit"
    for name in FLAT:
        assert _same_cam(auto.cam_out_dir, split.cam_out_dir, name), (name, "is the --split_gemm 1 run's, bit for bit")
    k, cam, hi = _load_cam(auto.cam_out_dir, NOISE)
    assert bool(torch.isfinite(cam).all()) and bool(torch.isfinite(hi).all())
    lines = [s for s in world.auto_said if "split_gemm auto" in s]
    # make_cam and the semantic step each recomputed it; the instance step found the fp32 maps in the store and says nothing
    assert len(lines) == 2 and all(s.startswith("[worker 0] ") and "1 image(s)" in s and s.endswith(": " + NOISE) for s in lines), lines


def test_the_label_steps_auto_follow_the_same_rule(world):
    (fp32, _), (split, _), (auto, ca) = world.fp32, world.split, world.auto
    assert ca["sem"] == 1 and ca["ins"] == 0, "the semantic step recomputed the image; the instance step took its fp32 maps from the store"
    assert _same_png(auto.sem_seg_out_dir, fp32.sem_seg_out_dir, NOISE) and _same_ins(auto.ins_seg_out_dir, fp32.ins_seg_out_dir, NOISE)
    for name in FLAT:
        assert _same_png(auto.sem_seg_out_dir, split.sem_seg_out_dir, name), name
        assert _same_ins(auto.ins_seg_out_dir, split.ins_seg_out_dir, name), name


def test_the_instance_step_auto_recomputes_on_its_own(world):
    """make_ins_seg_labels as the FIRST label step of a run (no edge map handed over): it flags, drops and recomputes itself."""
    from irn_amd.step import _common, make_ins_seg_labels
    from irn_amd.step import _report
    from irn_amd.net import resnet50 as r50
    r50.set_split_mode("auto")
    _common.EDGE_STORE.clear()
    a = argparse.Namespace(**{**vars(world.auto[0]), "ins_seg_out_dir": str(world.tmp / "auto" / "ins_first")})
    os.makedirs(a.ins_seg_out_dir)
    n0 = _report.worker_stats()["split_fallback_images"]
    make_ins_seg_labels.run(a)
    assert _report.worker_stats()["split_fallback_images"] - n0 == 1
    assert _same_ins(a.ins_seg_out_dir, world.fp32[0].ins_seg_out_dir, NOISE)
    for name in FLAT:
        assert _same_ins(a.ins_seg_out_dir, world.split[0].ins_seg_out_dir, name), name


def test_make_cam_auto_reads_the_flags_behind_their_copy(world, monkeypatch):
    """The device is kept busy in front of every flush, for ten times the host time a warm flush takes: the writer threads run
    ahead of the flags' copy, and a read that did not wait for it would see zeros and write the split pass's file."""
    from irn_amd.step import make_cam
    real = make_cam._flush_group
    host = []

    def timed(*a, **k):
        t0 = time.perf_counter()
        real(*a, **k)
        host.append((time.perf_counter() - t0) * 1e3)

    monkeypatch.setattr(make_cam, "_flush_group", timed)
    world.run("auto", "auto_warm", world.all_list, steps=("cam",))
    ms = _lag.stall_ms_for(max(host))
    seen = []

    def stalled(*a, **k):
        ev = _lag.stall(ms)
        t0 = time.perf_counter()
        real(*a, **k)
        seen.append(((time.perf_counter() - t0) * 1e3, _lag.lagging(ev)))

    monkeypatch.setattr(make_cam, "_flush_group", stalled)
    auto, counts = world.run("auto", "auto_lag", world.all_list, steps=("cam",))
    print("split auto lag: warm flushes took %s ms of host time, stall %.0f ms; (host ms, still lagging on return) per flush: %s" % (
        ["%.1f" % v for v in host], ms, seen))
    assert len(seen) == 2 and all(lag for host_ms, lag in seen), "a flush waited for the device"
    assert counts["cam"] == 1
    assert _same_cam(auto.cam_out_dir, world.fp32[0].cam_out_dir, NOISE)
    for name in FLAT:
        assert _same_cam(auto.cam_out_dir, world.split[0].cam_out_dir, name), name


def test_split_gemm_1_still_raises_at_the_end_of_the_step(world):
    """Existing behaviour: the default mode on the same tree writes its files and raises when the step ends."""
    from irn_amd import ops
    ops.split_overflowed()
    with pytest.raises(RuntimeError, match="IRN_SPLIT_GEMM=0"):
        world.run("1", "split_all", world.all_list, steps=("cam",))
    assert not ops.split_overflowed()                    # reported once
