"""ops.detection_overlap_batch (irn_detect_instance_batch_overlap) and ops.argmax_rethreshold_batch on the GPU.

The overlap counts are integers and are compared with ==: against the existing dense path (ops.detect_instance_batch +
ops.mask_overlap per image) and against the numpy restatement tests/_detmap_overlap_ref.py.  The rethresholded argmax map is
compared bit for bit with the label epilogue's own map at that threshold."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _detmap_overlap_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (17, 1), (5, 7), (16, 64), (17, 65), (33, 65), (96, 128)]
CELLS = 4096                                     # kOvlCells of instance.hip: the LDS budget of the count table


def _dev():
    return torch.device("cuda", 0)


def _blocky(rng, h, w, hi, cell, zero=0.3):
    """int map of values 0..hi, constant on cell x cell blocks (several pixels per component), about `zero` of them 0."""
    gh, gw = -(-h // cell), -(-w // cell)
    coarse = rng.randint(1, hi + 1, (gh, gw)) * (rng.rand(gh, gw) >= zero) if hi else np.zeros((gh, gw), int)
    return np.repeat(np.repeat(coarse, cell, 0), cell, 1)[:h, :w]


def _image(seed, h, w, n_ch, g, cell=5):
    rng = np.random.RandomState(seed)
    am = _blocky(rng, h, w, n_ch, cell).astype(np.int32)
    rw = rng.rand(n_ch, h, w).astype(np.float32)
    inst = (_blocky(rng, h, w, g, 7) if g < 255 else rng.randint(0, 256, (h, w))).astype(np.uint8)
    return {"rw": rw, "am": am, "n_ch": n_ch, "inst": inst, "g": g, "min_area": h * w * 0.01,
            "class_ids": np.arange(n_ch, dtype=np.int64) * 3 + 1}


def _gpu(images):
    d = _dev()
    return ([torch.from_numpy(im["rw"]).to(d) for im in images], [torch.from_numpy(im["am"]).to(d) for im in images],
            [torch.from_numpy(im["inst"]).to(d) for im in images])


def _overlap(images, **kw):
    from irn_amd import ops
    rws, ams, insts = _gpu(images)
    bad = torch.zeros(1, dtype=torch.int64, device=_dev())
    recs = ops.detection_overlap_batch(rws, ams, [im["class_ids"] for im in images], [im["n_ch"] for im in images],
                                       [im["min_area"] for im in images], insts, [im["g"] for im in images], bad, **kw)
    return recs, bad


def _dense(images):
    """The existing path: dense masks per image, then mask_overlap on them."""
    from irn_amd import ops
    rws, ams, insts = _gpu(images)
    dets = ops.detect_instance_batch(rws, ams, [im["class_ids"] for im in images], [im["n_ch"] for im in images],
                                     [im["min_area"] for im in images])
    bad = torch.zeros(1, dtype=torch.int64, device=_dev())
    out = []
    for im, det, inst in zip(images, dets, insts):
        h, w = im["am"].shape
        if isinstance(det, Exception):
            det = {"score": np.zeros(0, np.float32), "class": np.zeros(0, np.int64), "mask": np.zeros((0, h, w), bool)}
        inter, ap, ag = ops.mask_overlap(torch.from_numpy(np.ascontiguousarray(det["mask"])).to(_dev()), inst, im["g"], bad)
        out.append({"pred_class": det["class"], "pred_score": det["score"], "inter": inter.cpu().numpy(),
                    "area_pred": ap.cpu().numpy(), "area_gt": ag.cpu().numpy()})
    return out, int(bad.item())


def _same(got, want, keys=("pred_class", "pred_score", "inter", "area_pred", "area_gt")):
    assert set(got) == {"pred_class", "pred_score", "inter", "area_pred", "area_gt"}
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), k


def _check(images, numpy_too=True):
    got, bad = _overlap(images)
    want, want_bad = _dense(images)
    assert len(got) == len(images)
    for im, a, b in zip(images, got, want):
        _same(a, b)
        if numpy_too:
            ref, _ = R.overlap(im["rw"], im["am"], im["n_ch"], im["min_area"], im["inst"], im["g"])
            ref["pred_class"] = im["class_ids"][ref.pop("channel")]
            _same(a, ref)
    assert int(bad.item()) == want_bad == sum(int((im["inst"] > im["g"]).sum()) for im in images)
    return got


@pytest.mark.parametrize("h,w", SHAPES)
def test_counts_equal_the_dense_path(h, w):
    for g in (0, 1, 3, 255):
        _check([_image(h * 131 + w + g, h, w, 3, g, cell=3 if h * w < 100 else 5)])


def test_mixed_batch_with_an_image_without_detections():
    images = [_image(1, 33, 65, 2, 3), _image(2, 17, 65, 2, 4), _image(3, 96, 128, 4, 2)]
    images[1]["am"][:] = 0                                  # n_det == 0 inside a batch of three
    got = _check(images)
    assert len(got[1]["pred_score"]) == 0 and got[1]["inter"].shape == (0, 4) and got[1]["area_gt"].sum() > 0
    assert len(got[0]["pred_score"]) > 1 and len(got[2]["pred_score"]) > 1


def test_all_sizes_in_one_batch_and_alone():
    images = [_image(50 + i, h, w, 3, (0, 1, 3, 255)[i % 4]) for i, (h, w) in enumerate(SHAPES)]
    together = _check(images, numpy_too=False)
    for im, rec in zip(images, together):
        alone, _ = _overlap([im])
        _same(alone[0], rec)


def test_gt_id_above_the_count_is_bad_and_belongs_to_nobody():
    im = _image(7, 33, 65, 3, 3)
    im["inst"][4:9, 10:30] = 9
    im["inst"][20, :] = 4
    got = _check([im])
    assert int((im["inst"] > 3).sum()) == 5 * 20 + 65 and got[0]["inter"].shape[1] == 3


def test_checkerboard_takes_the_global_path():
    h, w = 33, 65
    yy, xx = np.mgrid[:h, :w]
    im = _image(11, h, w, 2, 3)
    im["am"] = (1 + (yy + xx) % 2).astype(np.int32)          # every pixel is its own detection
    im["min_area"] = 0.0
    got = _check([im])
    assert len(got[0]["pred_score"]) == h * w == 2145 and (h * w + 1) * (3 + 1) > CELLS
    assert (got[0]["area_pred"] == 1).all() and (got[0]["pred_score"] > 0).all()


def test_small_table_and_one_detection_across_tiles_and_waves():
    im = _image(13, 96, 128, 2, 3, cell=24)
    im["am"][:] = 0
    im["am"][3:90, 2:126] = 1                                # one component over 6 x 2 labelling tiles
    im["am"][92:94, 5:6] = 2                                 # area 2 < min_area: score 0, place kept
    got = _check([im])[0]
    assert len(got["pred_score"]) == 2 and (2 + 1) * (3 + 1) <= CELLS
    assert got["area_pred"].tolist() == [87 * 124, 2] and got["pred_score"][1] == 0 and got["pred_score"][0] > 0
    assert (got["inter"][0] > 0).sum() >= 2                  # the detection meets several GT instances


def test_five_calls_give_identical_bytes():
    images = [_image(21, 96, 128, 4, 5), _image(22, 33, 65, 2, 255, cell=1)]
    runs = [_overlap(images)[0] for _ in range(5)]
    for recs in runs[1:]:
        for a, b in zip(recs, runs[0]):
            _same(a, b)
    deferred = _overlap(images, deferred=True)[0].result()
    for a, b in zip(deferred, runs[0]):
        _same(a, b)


def test_argument_refusals_leave_the_outputs_untouched():
    from irn_amd import _lib, ops
    im = _image(31, 17, 65, 2, 3)
    rws, ams, insts = _gpu([im])
    dc = ops.detect_batch_count(rws, ams, [2])
    nd = dc.nds[0]
    assert nd > 0
    outs = [torch.full((n,), 0x55, dtype=torch.uint8, device=_dev()) for n in (4 * nd, 4 * nd, 8 * nd, 8 * nd * 3, 8 * 3, 8)]

    def call(n_det=nd, g=3, inst=insts[0].data_ptr(), h=dc.hs_a, w=dc.ws_a, min_area=(C.c_double * 1)(1.0), n=1, bad=outs[5].data_ptr()):
        return _lib.lib.irn_detect_instance_batch_overlap(
            n, dc.sc_p, dc.am_p, dc.cs_a, h, w, _lib.i32_array([n_det]), min_area, _lib.ptr_array([inst]), _lib.i32_array([g]),
            outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), bad,
            dc.scratch.data_ptr(), None)

    big = _lib.i32_array([40000])
    for kw in (dict(inst=None), dict(g=256), dict(g=-1), dict(n_det=-1), dict(n_det=17 * 65 + 1), dict(h=big, w=big),
               dict(min_area=None), dict(bad=None), dict(n=-1)):
        assert call(**kw) == 1, kw                                            # IRN_ERR_ARG
        assert b"irn_detect_instance_batch_overlap" in _lib.lib.irn_last_error()
    assert call(n=0) == 0                                                      # an empty batch: nothing is done
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 0x55).all())
    with pytest.raises(ValueError, match="GT instances"):
        ops.detection_overlap_batch(rws, ams, [im["class_ids"]], [2], [1.0], insts, [256])
    assert ops.detection_overlap_batch([], [], [], [], [], [], []) == []


def test_rethreshold_equals_the_epilogue_bit_for_bit():
    from irn_amd import ops
    rng = np.random.RandomState(5)
    rws, sizes = [], []
    for c, h, w, oh, ow in ((3, 24, 32, 96, 128), (2, 29, 38, 113, 150), (1, 5, 7, 17, 25)):
        f = rng.rand(c, h // 4 + 2, w // 4 + 2).astype(np.float32)            # smooth, walk-like: a few peaks per channel
        f = np.repeat(np.repeat(f, 4, 1), 4, 2)[:, :h, :w] * (0.2 + 0.8 * rng.rand(c, h, w).astype(np.float32))
        rws.append(f)
        sizes.append((oh, ow))
    rws[1][0, 10:14, 20:25] = np.nan                                           # a NaN region in one channel
    dev_rws = [torch.from_numpy(r).to(_dev()) for r in rws]
    t_low = 0.2

    def epilogue(t):
        return ops.label_epilogue(dev_rws, sizes, t, want_labels=False, want_argmax=True, want_rw_up=True)
    low = epilogue(t_low)
    am0, up0 = low["argmax"][0].cpu().numpy(), low["rw_up"][0].cpu().numpy()
    ys, xs = np.nonzero(am0)
    k = len(ys) // 2
    t_equal = float(up0[am0[ys[k], xs[k]] - 1, ys[k], xs[k]])                  # a winning score: exactly the threshold
    assert t_low < t_equal < 1.0 and not np.isnan(t_equal)
    seen = []
    for t in (t_low, t_equal, 0.6):
        want = epilogue(t)["argmax"]
        got = ops.argmax_rethreshold_batch(low["rw_up"], low["argmax"], t)
        for a, b in zip(got, want):
            assert a.dtype == torch.int32 and a.shape == b.shape and torch.equal(a, b)
        seen.append(torch.cat([a.reshape(-1) for a in got]).cpu().numpy())
    assert seen[1].reshape(-1)[ys[k] * 128 + xs[k]] == 0 and am0[ys[k], xs[k]] > 0   # strict >: the equal score is background
    assert (seen[0] != seen[1]).any() and (seen[1] != seen[2]).any() and (seen[2] > 0).any()
    nan_px = np.isnan(low["rw_up"][1].cpu().numpy()[0])
    assert nan_px.any() and (got[1].cpu().numpy()[nan_px] == 1).all()           # a NaN keeps its channel at every threshold
    with pytest.raises(Exception, match="irn_argmax_rethreshold_batch"):
        ops.argmax_rethreshold_batch(low["rw_up"], low["argmax"], float("nan"))
