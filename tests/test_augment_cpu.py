"""The batched training-input pipeline without a GPU: the host tables of `ops.augment_tables` drive a numpy emulation of
the two device passes to exactly the PIL / numpy pipeline; the CAM training dataset's two item forms agree; its draws are a
function of (seed, epoch, index); `irn_augment_batch` refuses bad descriptors before any device work; the new entry point
parses, and the old ones still refuse."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as A  # noqa: E402

from irn_amd import _lib, ops  # noqa: E402
from irn_amd.voc12 import dataloader  # noqa: E402

LUT = ops.normalize_lut()
ALL_SHAPES = A.SHAPES + A.TRAIN_SHAPES


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "%dx%d_crop%d" % s[:3])
def test_tables_drive_the_two_passes_to_the_reference(shape):
    cases = A.cases([shape])
    assert len(cases) >= 18
    img = A.image(shape[0], shape[1], 0)
    for h, w, crop, params in cases:
        t = ops.augment_tables([(h, w)], [params], crop)
        got = A.emulate(t, [img], crop, LUT)[0]
        assert np.array_equal(got, A.augment_ref(img, params, crop)), "params %s" % (params,)


def test_tables_of_a_batch_are_the_tables_of_its_images():
    imgs = [A.image(h, w, i) for i, (h, w, _, _) in enumerate(A.SHAPES)]
    crop = 48
    params = [A.params_for(h, w, crop, t, f, "drawn", np.random.default_rng(i))
              for i, ((h, w, _, _), t, f) in enumerate(zip(A.SHAPES, (30, 64, 100, 95, 310), (1, 0, 1, 0, 1)))]
    t = ops.augment_tables([im.shape[:2] for im in imgs], params, crop)
    assert t.meta.dtype == np.int32 and t.pixels_bytes == sum(im.size for im in imgs)
    got = A.emulate(t, imgs, crop, LUT)
    for i, (im, p) in enumerate(zip(imgs, params)):
        assert np.array_equal(got[i], A.augment_ref(im, p, crop)), i
    with pytest.raises(ValueError):
        ops.augment_tables([(20, 27)], [(20, 27, 0, (0, 0, 0, 0, 21, 27))], 32)          # a box taller than the image


@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("voc_cls"))
    return root, A.write_voc(root, 4)


def _dataset(voc, raw, **kw):
    root, lst = voc
    args = dict(resize_long=(48, 200), hor_flip=True, crop_size=96, crop_method="random", seed=3)
    args.update(kw)
    return dataloader.VOC12ClassificationDataset(lst, voc12_root=root, raw=raw, **args)


def test_dataset_item_is_the_reference_of_its_own_draws(voc):
    host, raw = _dataset(voc, False), _dataset(voc, True)
    seen = set()
    for epoch in range(3):
        host.set_epoch(epoch), raw.set_epoch(epoch)
        for idx in range(len(host)):
            a, b = host[idx], raw[idx]
            assert a["name"] == b["name"] and torch.equal(a["label"], b["label"]) and b["size"] == (120, 140)
            assert b["img"].dtype == torch.uint8 and tuple(b["img"].shape) == (120, 140, 3)
            assert a["img"].dtype == np.float32 and a["img"].shape == (3, 96, 96)
            assert np.array_equal(a["img"], A.augment_ref(b["img"].numpy(), b["aug"], 96))
            seen.add((b["aug"][2], b["aug"][0] > 96))
    assert len(seen) == 4                                      # mirrored and not, padded and windowed
    # the validation form: no resize, no mirror, the top-left box
    host, raw = _dataset(voc, False, resize_long=None, hor_flip=False, crop_method=None), \
        _dataset(voc, True, resize_long=None, hor_flip=False, crop_method=None)
    assert raw[1]["aug"] == (120, 140, 0, (0, 0, 0, 0, 96, 96))
    assert np.array_equal(host[1]["img"], A.augment_ref(raw[1]["img"].numpy(), raw[1]["aug"], 96))
    assert host[1]["label"].sum() >= 1 and host[1]["label"].shape == (20,)


def test_collate_keeps_ragged_images_as_a_list(voc):
    raw, host = _dataset(voc, True), _dataset(voc, False)
    pack = dataloader.classification_collate([raw[0], raw[1]])
    assert isinstance(pack["img"], list) and len(pack["aug"]) == 2 and tuple(pack["label"].shape) == (2, 20)
    pack = dataloader.classification_collate([host[0], host[1]])
    assert tuple(pack["img"].shape) == (2, 3, 96, 96) and pack["img"].dtype == torch.float32 and "aug" not in pack


def test_draws_depend_on_seed_epoch_and_index_only(voc):
    from torch.utils.data import DataLoader
    ds = _dataset(voc, True)

    def draws(workers):
        loader = DataLoader(ds, batch_size=2, shuffle=False, num_workers=workers, collate_fn=dataloader.classification_collate)
        return [a for pack in loader for a in pack["aug"]]

    ds.set_epoch(0)
    first = draws(0)
    assert first == draws(2) and len(first) == 4
    ds.set_epoch(1)
    assert draws(0) != first
    assert _dataset(voc, True, seed=4)[0]["aug"] != _dataset(voc, True, seed=3)[0]["aug"]
    # the long side: uniform over the range, both ends included (random.randint)
    ds = _dataset(voc, True, resize_long=(320, 640), crop_size=512)
    longs = [max(ds.draw(i, (375, 500))[:2]) for i in range(2000)]
    assert min(longs) == 320 and max(longs) == 640
    flips = [ds.draw(i, (375, 500))[2] for i in range(200)]
    assert 60 < sum(flips) < 140


def _valid_call():
    """A valid two-image call as ctypes arguments (fake device pointers: never dereferenced before the checks pass)."""
    params = [A.params_for(20, 27, 32, 40, 1, "max"), A.params_for(70, 90, 32, 60, 0, "max")]
    t = ops.augment_tables([(20, 27), (70, 90)], params, 32)
    return t, t.meta.copy()


def _call(n, crop, meta, words, pixels_bytes, scratch_bytes, out_elems=None, null=None):
    one = C.c_void_p(64)
    ptrs = {k: one for k in ("pixels", "lut", "out", "scratch", "meta_dev")}
    if null:
        ptrs[null] = None
    m = None if null == "meta" else meta.ctypes.data_as(C.POINTER(C.c_int32))
    return _lib.lib.irn_augment_batch(n, crop, m, words, ptrs["pixels"], pixels_bytes, ptrs["lut"], ptrs["out"],
                                      n * 3 * crop * crop if out_elems is None else out_elems, ptrs["scratch"], scratch_bytes,
                                      ptrs["meta_dev"], words, None)


def test_entry_refuses_bad_descriptors_before_any_device_work():
    t, meta = _valid_call()
    words, pb, sb = meta.size, t.pixels_bytes, t.scratch_bytes
    assert _call(0, 32, meta, words, pb, sb) == 0                                # empty batch: nothing to do
    assert _call(-1, 32, meta, words, pb, sb) == 1
    for null in ("meta", "pixels", "lut", "out", "scratch", "meta_dev"):
        assert _call(2, 32, meta, words, pb, sb, null=null) == 1 and b"null" in _lib.lib.irn_last_error()
    assert _call(2, 0, meta, words, pb, sb) == 1 and b"crop" in _lib.lib.irn_last_error()

    def broken(edit, **kw):
        m = meta.copy()
        edit(m)
        args = dict(n=2, crop=32, meta=m, words=words, pixels_bytes=pb, scratch_bytes=sb)
        args.update(kw)
        rc = _call(**args)
        return rc, _lib.lib.irn_last_error()

    D = ops.AUGMENT_DESC_WORDS
    h, w, c_top, c_left, rows, cols, r0, nrows, kx, ky, src, mid, xtab, ytab = (int(v) for v in meta[D:D + 14])      # image 1

    def x_tap_past_the_row(m):                  # the last tap of some column now ends one past the source row
        j = int(np.argmax(m[xtab:xtab + cols] + m[xtab + cols:xtab + 2 * cols]))
        m[xtab + j] += w - (m[xtab + j] + m[xtab + cols + j]) + 1
    rc, msg = broken(x_tap_past_the_row)
    assert rc == 1 and b"X tap" in msg

    def y_tap_past_the_rows(m):
        j = int(np.argmax(m[ytab:ytab + rows] + m[ytab + rows:ytab + 2 * rows]))
        m[ytab + rows + j] += 1                 # r1 is the largest lo + count: one more reads past the intermediate
    rc, msg = broken(y_tap_past_the_rows)
    assert rc == 1 and b"Y tap" in msg
    rc, msg = broken(lambda m: m.__setitem__(xtab, -1))
    assert rc == 1 and b"X tap" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 3, 32 - cols + 1))              # the box one pixel past the crop's right edge
    assert rc == 1 and b"crop" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 2, -1))
    assert rc == 1 and b"crop" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 7, h - r0 + 1))                 # one source row too many
    assert rc == 1 and b"source rows" in msg
    rc, msg = broken(lambda m: None, pixels_bytes=pb - 1)                        # the last image ends past the pixel buffer
    assert rc == 1 and b"pixels" in msg
    rc, msg = broken(lambda m: None, scratch_bytes=sb - 1)
    assert rc == 1 and b"intermediate" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 13, words - rows * (2 + ky) + 1))   # a table that ends past the words passed
    assert rc == 1 and b"Y table" in msg
    rc, msg = broken(lambda m: m.__setitem__(D + 12, 2 * D - 1))                 # a table inside the descriptors
    assert rc == 1 and b"X table" in msg
    rc, msg = broken(lambda m: None, out_elems=2 * 3 * 32 * 32 - 1)
    assert rc == 1 and b"output" in msg


def test_parser_of_the_new_entry_point_and_the_old_refusals(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import run_sample
    import run_train
    import run_train_cam
    a = run_train_cam.build_parser().parse_args(["--voc12_root", "x"])
    assert tuple(a.cam_resize_long) == (320, 640) and a.cam_augment == "device" and a.cam_init_weights is None
    assert (a.cam_crop_size, a.cam_batch_size, a.cam_num_epoches, a.cam_learning_rate, a.cam_weight_decay) == (512, 16, 5, 0.1, 1e-4)
    assert a.seed == 0 and a.cam_weights_name == "sess/res50_cam.pth" and a.val_list == "voc12/val.txt"
    a = run_train_cam.build_parser().parse_args(["--voc12_root", "x", "--cam_resize_long", "48", "96", "--cam_augment", "host",
                                                 "--cam_init_weights", "w.pth"])
    assert tuple(a.cam_resize_long) == (48, 96) and a.cam_augment == "host" and a.cam_init_weights == "w.pth"
    with pytest.raises(SystemExit):
        run_train_cam.build_parser().parse_args(["--voc12_root", "x", "--cam_augment", "both"])
    for mod in (run_train, run_sample):
        with pytest.raises(SystemExit) as e:
            mod.main(["--voc12_root", str(tmp_path), "--train_cam_pass", "True", "--log_name", str(tmp_path / "log")])
        assert "run_train_cam.py" in str(e.value)
        assert not os.path.exists(str(tmp_path / "log.log"))
    assert run_sample.OUT_OF_SCOPE == ("train_cam_pass", "train_irn_pass")
    from irn_amd.step import train_cam
    assert train_cam.MAX_LOADER_WORKERS == 8 and train_cam.PRINT_EVERY == 100
