"""The (image, label) input pipeline of the IRNet step without a GPU: `ops.nearest_plan` is Pillow's NEAREST index row;
the host tables of `ops.augment_label_tables` drive a numpy emulation of the label kernel to exactly the host pipeline; the
raw items of the two IRNet datasets carry the draws of the non-raw items, and the host functions applied with those draws
give the non-raw item; the bicubic plan of equal sizes is the identity; the C entry refuses bad descriptors before any
device work; the new flag parses.  Two tests here do not test new code and pass without it: the identity of the equal-size
bicubic plan is a precondition of the top-left mode, and `test_the_cases_cover_what_they_claim` checks the case generator."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _aff_loss_ref as R  # noqa: E402
import _augment_pair_ref as P  # noqa: E402

from irn_amd import _lib, ops  # noqa: E402
from irn_amd.misc import imutils  # noqa: E402
from irn_amd.voc12 import dataloader  # noqa: E402


def _pillow_row(w, out):
    """The source index Pillow's NEAREST reads per output cell: an index ramp resized (mode I: 32-bit, any width)."""
    ramp = Image.fromarray(np.arange(w, dtype=np.int32)[None, :])
    return np.asarray(ramp.resize((out, 1), Image.NEAREST))[0]


def test_nearest_plan_is_pillows_index_row_for_every_small_pair():
    for w in range(1, 41):
        for out in range(1, 61):
            got = ops.nearest_plan(w, out)
            assert got.dtype == np.int32 and got.shape == (out,)
            assert np.array_equal(got, _pillow_row(w, out)), (w, out)


def test_nearest_plan_is_pillows_index_row_for_seeded_scales():
    rng = np.random.default_rng(2024)
    textbook_differs = 0
    for _ in range(2000):
        w = int(rng.integers(1, 600))
        out = max(1, int(np.round(w * (0.5 + rng.random()))))
        want = _pillow_row(w, out)
        assert np.array_equal(ops.nearest_plan(w, out), want), (w, out)
        textbook_differs += not np.array_equal(np.floor((np.arange(out) + 0.5) * w / out).astype(np.int64), want)
    assert textbook_differs > 0            # the running sum is not the closed form: the restatement has to be Pillow's
    # the same walk along the other axis, and crop -> crop / 4 is [2::4]
    col = Image.fromarray(np.arange(37, dtype=np.int32)[:, None]).resize((1, 23), Image.NEAREST)
    assert np.array_equal(np.asarray(col)[:, 0], ops.nearest_plan(37, 23))
    for crop in (8, 96, 512):
        assert np.array_equal(ops.nearest_plan(crop, crop // 4), np.arange(crop)[2::4])
    assert np.array_equal(ops.nearest_plan(45, 45), np.arange(45))
    assert not ops.nearest_plan(45, 45).flags.writeable
    with pytest.raises(ValueError):
        ops.nearest_plan(0, 4)


@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "%dx%d_crop%d" % s)
@pytest.mark.parametrize("reduce", [1, 4])
def test_label_tables_drive_the_gather_to_the_host_pipeline(shape, reduce):
    cases = P.cases([shape])
    assert len(cases) >= 3 * 2 * 2
    lab = P.label(shape[0], shape[1], 0)
    for h, w, crop, params in cases:
        t = ops.augment_label_tables([(h, w)], [params], crop, reduce)
        got = P.emulate_label(t, [lab], crop, reduce)[0]
        assert np.array_equal(got, P.label_ref(lab, params, crop, reduce)), "params %s" % (params,)


def test_the_cases_cover_what_they_claim():
    seen_fit, seen_edges = set(), set()
    for h, w, crop, (hs, ws, flip, (c_top, c_left, i_top, i_left, rows, cols)) in P.cases():
        seen_fit.add((np.sign(hs - crop) > 0, np.sign(ws - crop) > 0))
        seen_edges |= {("c_top", c_top == 0), ("c_left", c_left == 0), ("c_bottom", c_top + rows == crop), ("c_right", c_left + cols == crop),
                       ("i_top", i_top == 0), ("i_left", i_left == 0), ("i_bottom", i_top + rows == hs), ("i_right", i_left + cols == ws)}
        assert crop in (8, 96)
    assert seen_fit == {(False, False), (False, True), (True, False), (True, True)}
    assert len(seen_edges) == 16           # every edge of the image and of the container both touched and not


def test_label_tables_of_a_batch_are_the_tables_of_its_images():
    crop = 96
    cases = [c for c in P.cases() if c[2] == crop][5::7]
    assert len(cases) >= 4
    labs = [P.label(h, w, i) for i, (h, w, _, _) in enumerate(cases)]
    params = [c[3] for c in cases]
    for reduce in (1, 4):
        t = ops.augment_label_tables([lb.shape for lb in labs], params, crop, reduce)
        assert t.meta.dtype == np.int32 and t.labels_bytes == sum(lb.size for lb in labs)
        got = P.emulate_label(t, labs, crop, reduce)
        for i, (lb, p) in enumerate(zip(labs, params)):
            assert np.array_equal(got[i], P.label_ref(lb, p, crop, reduce)), i
    with pytest.raises(ValueError):
        ops.augment_label_tables([(20, 27)], [(20, 27, 0, (0, 0, 0, 0, 21, 27))], 32, 4)       # a box taller than the image
    with pytest.raises(ValueError):
        ops.augment_label_tables([(20, 27)], [(20, 27, 0, (0, 0, 0, 0, 20, 27))], 32, 3)       # 32 % 3 != 0


def test_bicubic_plan_of_equal_sizes_is_the_identity():
    """The host path skips the resize at equal sizes (`pil_resize` returns its input); the device path resamples with the
    plan, which must then copy: one tap per cell, on the cell itself, of weight 1.0 in Pillow's fixed point."""
    for n in (1, 2, 5, 96, 375, 500):
        lo, cnt, k = ops.bicubic_plan(n, n)
        assert np.array_equal(lo + np.argmax(k, axis=1), np.arange(n))
        assert np.array_equal(k.max(axis=1), np.full(n, 1 << 22)) and np.array_equal(np.abs(k).sum(axis=1), np.full(n, 1 << 22))
        assert np.all(lo >= 0) and np.all(lo + cnt <= n)


@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("voc_aff"))
    lst, label_dir = R.write_voc(root, 4)
    return root, lst, label_dir


def _affinity(voc, raw, **kw):
    root, lst, label_dir = voc
    args = dict(hor_flip=True, crop_size=96, crop_method="random", rescale=(0.5, 1.5), seed=3)
    args.update(kw)
    return dataloader.VOC12AffinityDataset(lst, label_dir=label_dir, voc12_root=root, raw=raw, **args)


def test_raw_affinity_item_carries_the_draws_of_the_host_item(voc):
    host, raw = _affinity(voc, False), _affinity(voc, True)
    seen = set()
    for epoch in range(4):
        host.set_epoch(epoch), raw.set_epoch(epoch)
        for idx in range(len(host)):
            a, b = host[idx], raw[idx]
            assert sorted(b) == ["aug", "img", "label_map", "name", "size"] and sorted(a) == ["img", "label", "name"]
            assert a["name"] == b["name"] and b["size"] == (120, 140)
            assert b["img"].dtype == torch.uint8 and tuple(b["img"].shape) == (120, 140, 3)
            assert b["label_map"].dtype == torch.uint8 and tuple(b["label_map"].shape) == (120, 140)
            assert a["img"].dtype == np.float32 and a["img"].shape == (3, 96, 96)
            assert a["label"].dtype == np.uint8 and a["label"].shape == (24, 24)
            assert b["aug"] == raw.draw(idx, b["size"])
            hs, ws = b["aug"][:2]
            assert 60 <= hs <= 180 and 70 <= ws <= 210
            # the host functions with the raw item's draws give the host item
            assert np.array_equal(a["img"], P.augment_ref(b["img"].numpy(), b["aug"], 96))
            assert np.array_equal(a["label"], P.label_ref(b["label_map"].numpy(), b["aug"], 96, 4))
            # and so do the tables the device will read
            t = ops.augment_label_tables([b["size"]], [b["aug"]], 96, 4)
            assert np.array_equal(P.emulate_label(t, [b["label_map"].numpy()], 96, 4)[0], a["label"])
            seen.add((b["aug"][2], hs > 96))
    assert len(seen) == 4                                      # mirrored and not, padded and windowed
    # the top-left form without rescale and mirror
    host, raw = _affinity(voc, False, rescale=None, hor_flip=False, crop_method="top_left"), \
        _affinity(voc, True, rescale=None, hor_flip=False, crop_method="top_left")
    assert raw[1]["aug"] == (120, 140, 0, (0, 0, 0, 0, 96, 96))
    assert np.array_equal(host[1]["img"], P.augment_ref(raw[1]["img"].numpy(), raw[1]["aug"], 96))
    assert np.array_equal(host[1]["label"], P.label_ref(raw[1]["label_map"].numpy(), raw[1]["aug"], 96, 4))


def test_draw_consumes_the_generator_in_the_order_of_getitem(voc):
    ds = _affinity(voc, True)
    ds.set_epoch(2)
    rng = np.random.default_rng([3, 2, 1])
    scale = 0.5 + float(rng.random()) * (1.5 - 0.5)
    hs, ws = int(np.round(120 * scale)), int(np.round(140 * scale))
    flip = int(rng.integers(2))
    left = int(rng.integers(abs(ws - 96) + 1))
    top = int(rng.integers(abs(hs - 96) + 1))
    assert ds.draw(1, (120, 140)) == (hs, ws, flip, P.box_for(hs, ws, 96, left, top))
    # np.round: half to even, as pil_rescale rounds
    fixed = _affinity(voc, True, rescale=(0.5, 0.5), hor_flip=False)
    assert fixed.draw(0, (5, 7))[:2] == (2, 4)


def test_raw_image_item_is_the_top_left_form(voc):
    root, lst, _ = voc
    for crop in (96, 160):                                     # the image larger than the crop, and smaller
        host = dataloader.VOC12ImageDataset(lst, voc12_root=root, crop_size=crop)
        raw = dataloader.VOC12ImageDataset(lst, voc12_root=root, crop_size=crop, raw=True)
        a, b = host[2], raw[2]
        assert sorted(b) == ["aug", "img", "name", "size"] and a["name"] == b["name"]
        assert b["aug"] == (120, 140, 0, (0, 0, 0, 0, min(crop, 120), min(crop, 140)))
        assert np.array_equal(a["img"], P.augment_ref(b["img"].numpy(), b["aug"], crop))
        # the device path resamples with the identity plan where the host path copies
        t = ops.augment_tables([b["size"]], [b["aug"]], crop)
        import _augment_ref as A
        assert np.array_equal(A.emulate(t, [b["img"].numpy()], crop, ops.normalize_lut())[0], a["img"])


def test_collate_and_loader_forms(voc):
    import argparse
    from irn_amd.step import _train, train_irn
    raw, host = _affinity(voc, True), _affinity(voc, False)
    pack = dataloader.affinity_collate([raw[0], raw[1]])
    assert isinstance(pack["img"], list) and isinstance(pack["label_map"], list) and len(pack["aug"]) == 2 and len(pack["size"]) == 2
    pack = dataloader.affinity_collate([host[0], host[1]])
    assert tuple(pack["img"].shape) == (2, 3, 96, 96) and pack["label"].dtype == torch.uint8 and "aug" not in pack
    a = next(iter(_train.loader(host, 2, 0, True, 7, train_irn.collate(host))))
    b = next(iter(_train.loader(raw, 2, 0, True, 7, train_irn.collate(raw))))
    assert a["name"] == b["name"] and tuple(a["label"].shape) == (2, 24, 24) and len(b["label_map"]) == 2
    root, lst, _ = voc
    img_raw = dataloader.VOC12ImageDataset(lst, voc12_root=root, crop_size=96, raw=True)
    c = next(iter(_train.loader(img_raw, 2, 0, False, 7, train_irn.collate(img_raw))))
    assert "label_map" not in c and len(c["img"]) == 2 and c["aug"][0][2] == 0
    assert train_irn.device_augment(argparse.Namespace()) and not train_irn.device_augment(argparse.Namespace(irn_augment="host"))
    ns = argparse.Namespace(train_list=lst, infer_list=lst, ir_label_out_dir=voc[2], voc12_root=root, irn_crop_size=96, irn_augment="host")
    train, infer = train_irn.make_datasets(ns, 3)
    assert not train.raw and not infer.raw and train.rescale == (0.5, 1.5) and train.hor_flip and train.seed == 3
    ns.irn_augment = "device"
    train, infer = train_irn.make_datasets(ns, 3)
    assert train.raw and infer.raw


def test_pair_refuses_mismatched_inputs_before_touching_a_device():
    img = torch.zeros((20, 27, 3), dtype=torch.uint8)
    params = [(20, 27, 0, (0, 0, 0, 0, 20, 27))]
    with pytest.raises(ValueError, match="label map"):
        ops.augment_pair_batch([img], [torch.zeros((20, 26), dtype=torch.uint8)], params, 32)
    with pytest.raises(ValueError, match="divide"):
        ops.augment_pair_batch([img], [torch.zeros((20, 27), dtype=torch.uint8)], params, 32, reduce=3)
    with pytest.raises(ValueError):
        ops.augment_pair_batch([img], [torch.zeros((20, 27), dtype=torch.int32)], params, 32)
    with pytest.raises(ValueError):
        ops.augment_pair_batch([img], [], params, 32)


def _call(n, crop, reduce, meta, words, labels_bytes, out_elems=None, null=None):
    """Fake device pointers: never dereferenced before the checks pass."""
    one = C.c_void_p(64)
    ptrs = {k: one for k in ("labels", "out", "meta_dev")}
    if null:
        ptrs[null] = None
    m = None if null == "meta" else meta.ctypes.data_as(C.POINTER(C.c_int32))
    g = crop // reduce if reduce > 0 else 0
    return _lib.lib.irn_augment_label_batch(n, crop, reduce, m, words, ptrs["labels"], labels_bytes, ptrs["out"],
                                            n * g * g if out_elems is None else out_elems, ptrs["meta_dev"], words, None)


def test_label_entry_refuses_bad_descriptors_before_any_device_work():
    params = [(10, 14, 1, P.box_for(10, 14, 32, 18, 22)), (105, 135, 0, P.box_for(105, 135, 32, 103, 73))]
    t = ops.augment_label_tables([(20, 27), (70, 90)], params, 32, 4)
    meta, words, lb = t.meta.copy(), t.meta.size, t.labels_bytes
    err = _lib.lib.irn_last_error
    assert _call(0, 32, 4, meta, words, lb) == 0                                 # empty batch: nothing to do
    assert _call(-1, 32, 4, meta, words, lb) == 1
    for null in ("meta", "labels", "out", "meta_dev"):
        assert _call(2, 32, 4, meta, words, lb, null=null) == 1 and b"null" in err()
    assert _call(2, 0, 4, meta, words, lb) == 1 and b"crop" in err()
    assert _call(2, 32, 3, meta, words, lb) == 1 and b"reduce" in err()
    assert _call(2, 32, 0, meta, words, lb) == 1 and b"reduce" in err()
    assert _call(0, 32, 3, meta, words, lb) == 1                                  # also refused for an empty batch

    def broken(edit, **kw):
        m = meta.copy()
        edit(m)
        args = dict(n=2, crop=32, reduce=4, meta=m, words=words, labels_bytes=lb)
        args.update(kw)
        return _call(**args), err()

    D = ops.AUGMENT_LABEL_DESC_WORDS
    h, w, c_top, c_left, rows, cols, src, rtab, ctab = (int(v) for v in meta[D:D + 9])       # image 1
    assert (h, w, rows, cols) == (70, 90, 32, 32) and rtab + rows == ctab and ctab + cols == words
    rc, msg = broken(lambda m: m.__setitem__(rtab + 5, h))                      # a row one past the source
    assert rc == 1 and b"row entry 5" in msg
    rc, msg = broken(lambda m: m.__setitem__(ctab + 31, w))
    assert rc == 1 and b"column entry 31" in msg
    rc, msg = broken(lambda m: m.__setitem__(ctab, -1))
    assert rc == 1 and b"column entry 0" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 3, 1))                         # the box one cell past the crop's right edge
    assert rc == 1 and b"crop" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 2, -1))
    assert rc == 1 and b"crop" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 4, 0))
    assert rc == 1 and b"crop" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 0, 0))
    assert rc == 1 and b"bad size" in msg
    rc, msg = broken(lambda m: None, labels_bytes=lb - 1)                        # the last map ends past the label buffer
    assert rc == 1 and b"labels at byte" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 6, -1))
    assert rc == 1 and b"labels at byte" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 8, words - cols + 1))          # a table that ends past the words passed
    assert rc == 1 and b"column table" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 7, 2 * D - 1))                 # a table inside the descriptors
    assert rc == 1 and b"row table" in msg
    rc, msg = broken(lambda m: None, out_elems=2 * 8 * 8 - 1)
    assert rc == 1 and b"output" in msg
    rc, msg = broken(lambda m: None, words=2 * D - 1)
    assert rc == 1 and b"descriptor" in msg


def test_parser_reads_the_new_flag():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import run_train
    a = run_train.build_parser().parse_args(["--voc12_root", "x"])
    assert a.irn_augment == "device"
    a = run_train.build_parser().parse_args(["--voc12_root", "x", "--irn_augment", "host"])
    assert a.irn_augment == "host"
    with pytest.raises(SystemExit):
        run_train.build_parser().parse_args(["--voc12_root", "x", "--irn_augment", "both"])
