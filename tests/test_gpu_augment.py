"""`ops.augment_batch` (irn_amd/csrc/augment.hip) on the GPU against the PIL / numpy pipeline, bit for bit.  The output
buffer is filled with NaN before every call: a cell the kernels do not write fails the comparison."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _run(imgs, params, crop, on_device=False):
    from irn_amd import ops
    ts = [torch.from_numpy(im) for im in imgs]
    if on_device:
        ts = [t.to(_dev()) for t in ts]
    out = torch.full((len(ts), 3, crop, crop), float("nan"), dtype=torch.float32, device=_dev())
    got = ops.augment_batch(ts, params, crop, device=_dev(), out=out)
    assert got is out
    return out.cpu()


def _ref(imgs, params, crop):
    return torch.from_numpy(np.stack([A.augment_ref(im, p, crop) for im, p in zip(imgs, params)]))


@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "%dx%d_crop%d" % s[:3])
def test_every_case_of_a_shape_equals_the_reference(shape):
    img = A.image(shape[0], shape[1], 0)
    cases = A.cases([shape])
    assert len(cases) >= 18
    for h, w, crop, params in cases:
        assert torch.equal(_run([img], [params], crop), _ref([img], [params], crop)), "params %s" % (params,)


def test_training_shape_as_a_batch_of_two():
    (h0, w0, crop, _), (h1, w1, _, _) = A.TRAIN_SHAPES
    imgs = [A.image(h0, w0, 1), A.image(h1, w1, 2)]
    rng = np.random.default_rng(5)
    params = [A.params_for(h0, w0, crop, 320, 1, "drawn", rng), A.params_for(h1, w1, crop, 640, 0, "drawn", rng)]
    assert params[0][1] < crop < params[1][0]                    # one padded, one windowed
    assert torch.equal(_run(imgs, params, crop), _ref(imgs, params, crop))


def _mixed():
    crop = 48
    imgs = [A.image(h, w, i) for i, (h, w, _, _) in enumerate(A.SHAPES)]
    params = [A.params_for(h, w, crop, t, f, "drawn", np.random.default_rng(i))
              for i, ((h, w, _, _), t, f) in enumerate(zip(A.SHAPES, (30, 64, 100, 95, 310), (1, 0, 1, 0, 1)))]
    return imgs, params, crop


def test_mixed_batch_equals_each_image_alone():
    imgs, params, crop = _mixed()
    batch = _run(imgs, params, crop)
    assert torch.equal(batch, _ref(imgs, params, crop))
    for i in range(len(imgs)):
        assert torch.equal(_run([imgs[i]], [params[i]], crop)[0], batch[i]), i
    assert torch.equal(_run(imgs, params, crop, on_device=True), batch)          # images already on the device
    from irn_amd import ops
    assert tuple(ops.augment_batch([], [], crop, device=_dev()).shape) == (0, 3, crop, crop)


def test_five_calls_give_identical_bits():
    imgs, params, crop = _mixed()
    first = _run(imgs, params, crop)
    for _ in range(4):
        assert torch.equal(_run(imgs, params, crop), first)


@pytest.mark.parametrize("flip", [0, 1])
def test_window_and_pad_at_every_edge(flip):
    crop = 32
    # 70x90 -> 47x60: a window on both axes (i_left 0 / 28, i_top 0 / 15); 20x27 -> 18x24: a pad on both (c_left 0 / 8, c_top 0 / 14)
    for (h, w), target in (((70, 90), 60), ((20, 27), 24)):
        img = A.image(h, w, 3)
        hs, ws = A.imutils.resize_long_size(h, w, target)
        max_left, max_top = abs(ws - crop), abs(hs - crop)
        assert max_left > 0 and max_top > 0
        for left in (0, max_left):
            for top in (0, max_top):
                params = (hs, ws, flip, A.box_for(hs, ws, crop, left, top))
                assert torch.equal(_run([img], [params], crop), _ref([img], [params], crop)), "params %s" % (params,)
