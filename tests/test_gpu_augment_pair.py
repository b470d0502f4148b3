"""`ops.augment_pair_batch` (irn_amd/csrc/augment.hip) on the GPU against the host pipeline of `VOC12AffinityDataset`
(Pillow / numpy), bit for bit.  The image buffer is filled with NaN and the label buffer with 7 — a value no label map here
holds — before every call: a cell the kernels do not write fails the comparison."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _aff_loss_ref as R  # noqa: E402
import _augment_pair_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 7


def _dev():
    return torch.device("cuda", 0)


def _run(imgs, labs, params, crop, reduce, on_device=False):
    from irn_amd import ops
    ti, tl = [torch.from_numpy(im) for im in imgs], [torch.from_numpy(lb) for lb in labs]
    if on_device:
        ti, tl = [t.to(_dev()) for t in ti], [t.to(_dev()) for t in tl]
    g = crop // reduce
    out = torch.full((len(ti), 3, crop, crop), float("nan"), dtype=torch.float32, device=_dev())
    out_label = torch.full((len(ti), g, g), SENTINEL, dtype=torch.uint8, device=_dev())
    got = ops.augment_pair_batch(ti, tl, params, crop, reduce=reduce, device=_dev(), out=out, out_label=out_label)
    assert got[0] is out and got[1] is out_label
    return out.cpu(), out_label.cpu()


def _ref(imgs, labs, params, crop, reduce):
    return (torch.from_numpy(np.stack([P.augment_ref(im, p, crop) for im, p in zip(imgs, params)])),
            torch.from_numpy(np.stack([P.label_ref(lb, p, crop, reduce) for lb, p in zip(labs, params)])))


@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "%dx%d_crop%d" % s)
@pytest.mark.parametrize("reduce", [1, 4])
def test_every_case_of_a_shape_equals_the_host_pipeline(shape, reduce):
    """Scales 0.5, 1.5 and 1.0 x both mirror states x the box at every edge of the image and of the container."""
    img, lab = P.image(shape[0], shape[1], 0), P.label(shape[0], shape[1], 0)
    cases = P.cases([shape])
    assert len(cases) >= 12
    for h, w, crop, params in cases:
        got_img, got_lab = _run([img], [lab], [params], crop, reduce)
        want_img, want_lab = _ref([img], [lab], [params], crop, reduce)
        assert torch.equal(got_lab, want_lab), "label, params %s" % (params,)
        assert torch.equal(got_img, want_img), "image, params %s" % (params,)


def _mixed():
    crop = 96
    cases = [c for c in P.cases() if c[2] == crop][5::7]
    imgs = [P.image(h, w, i) for i, (h, w, _, _) in enumerate(cases)]
    labs = [P.label(h, w, i) for i, (h, w, _, _) in enumerate(cases)]
    return imgs, labs, [c[3] for c in cases], crop


@pytest.mark.parametrize("reduce", [1, 4])
def test_mixed_batch_equals_each_image_alone(reduce):
    from irn_amd import ops
    imgs, labs, params, crop = _mixed()
    assert len(imgs) >= 4 and len({im.shape for im in imgs}) >= 2
    b_img, b_lab = _run(imgs, labs, params, crop, reduce)
    want_img, want_lab = _ref(imgs, labs, params, crop, reduce)
    assert torch.equal(b_lab, want_lab) and torch.equal(b_img, want_img)
    for i in range(len(imgs)):
        a_img, a_lab = _run([imgs[i]], [labs[i]], [params[i]], crop, reduce)
        assert torch.equal(a_lab[0], b_lab[i]) and torch.equal(a_img[0], b_img[i]), i
    d_img, d_lab = _run(imgs, labs, params, crop, reduce, on_device=True)      # inputs already on the device
    assert torch.equal(d_lab, b_lab) and torch.equal(d_img, b_img)
    # the image half is `augment_batch`
    assert torch.equal(ops.augment_batch([torch.from_numpy(im) for im in imgs], params, crop, device=_dev()).cpu(), b_img)
    e_img, e_lab = ops.augment_pair_batch([], [], [], crop, reduce=reduce, device=_dev())
    assert tuple(e_img.shape) == (0, 3, crop, crop) and tuple(e_lab.shape) == (0, crop // reduce, crop // reduce)
    assert e_lab.dtype == torch.uint8


def test_five_calls_give_identical_bits():
    imgs, labs, params, crop = _mixed()
    first = _run(imgs, labs, params, crop, 4)
    for _ in range(4):
        again = _run(imgs, labs, params, crop, 4)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


def test_top_left_mode_equals_the_image_dataset_item(tmp_path):
    """The displacement-mean pass: raw `VOC12ImageDataset` items through `augment_batch` give the non-raw items (the bicubic
    plan of equal sizes copies), the image larger than the crop and smaller."""
    from irn_amd import ops
    from irn_amd.voc12 import dataloader
    root = str(tmp_path)
    lst, _ = R.write_voc(root, 2)
    for crop in (96, 160):
        host = dataloader.VOC12ImageDataset(lst, voc12_root=root, crop_size=crop)
        raw = dataloader.VOC12ImageDataset(lst, voc12_root=root, crop_size=crop, raw=True)
        pack = dataloader.affinity_collate([raw[0], raw[1]])
        out = torch.full((2, 3, crop, crop), float("nan"), dtype=torch.float32, device=_dev())
        ops.augment_batch(pack["img"], pack["aug"], crop, device=_dev(), out=out)
        want = torch.from_numpy(np.stack([host[0]["img"], host[1]["img"]]))
        assert torch.equal(out.cpu(), want), crop


def test_refusals_launch_nothing():
    """A size mismatch, a `reduce` that does not divide the crop and a table entry outside the source are each refused, and
    both output buffers come back as they went in."""
    from irn_amd import _lib, ops
    crop = 32
    img, lab = P.image(20, 27, 0), P.label(20, 27, 0)
    params = [(20, 27, 1, P.box_for(20, 27, crop, 3, 5))]
    out = torch.full((1, 3, crop, crop), 3.5, dtype=torch.float32, device=_dev())
    out_label = torch.full((1, 8, 8), SENTINEL, dtype=torch.uint8, device=_dev())

    def untouched():
        torch.cuda.synchronize()
        return bool((out == 3.5).all()) and bool((out_label == SENTINEL).all())

    ti, tl = torch.from_numpy(img), torch.from_numpy(lab)
    with pytest.raises(ValueError, match="label map"):
        ops.augment_pair_batch([ti], [tl[:, :26].contiguous()], params, crop, device=_dev(), out=out, out_label=out_label)
    assert untouched()
    with pytest.raises(ValueError, match="divide"):
        ops.augment_pair_batch([ti], [tl], params, crop, reduce=3, device=_dev(), out=out, out_label=out_label)
    assert untouched()
    # the C entry itself, on real device buffers: a column entry one past the source row
    t = ops.augment_label_tables([(20, 27)], params, crop, 4)
    meta = t.meta.copy()
    ctab = int(meta[8])
    meta[ctab + 4] = 27
    labels_dev = tl.to(_dev()).reshape(-1)
    meta_dev = torch.zeros(meta.size, dtype=torch.int32, device=_dev())

    def entry(m, reduce=4):
        return _lib.lib.irn_augment_label_batch(1, crop, reduce, m.ctypes.data_as(C.POINTER(C.c_int32)), m.size, labels_dev.data_ptr(),
                                                labels_dev.numel(), out_label.data_ptr(), out_label.numel(), meta_dev.data_ptr(),
                                                meta_dev.numel(), None)

    assert entry(meta) == 1 and b"column entry 4" in _lib.lib.irn_last_error()
    assert untouched() and bool((meta_dev == 0).all())
    assert entry(t.meta, reduce=3) == 1 and b"reduce" in _lib.lib.irn_last_error()
    assert untouched() and bool((meta_dev == 0).all())
    # and the same call with its table intact goes through
    assert entry(t.meta) == 0
    torch.cuda.synchronize()
    assert torch.equal(out_label.cpu()[0], torch.from_numpy(P.label_ref(lab, params[0], crop, 4)))
