"""Instance labels as COCO run lengths straight from the detection map (the rle_* kernels of irn_amd/csrc/instance.hip
through ops.detect_instance_rle_batch) against the dense path they replace: every integer of
`ops.mask_rle(detect_instance_batch(...)["mask"])`, the scores and classes, the detection order; the same arrays alone
and inside a batch of 32; and run_sample.py end to end in both formats down to a byte-identical COCO file.

Every device step runs under a deadline (`_limit`): a step that hangs ends the process instead of holding the GPU."""
import contextlib
import faulthandler
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cocomask_ref as R  # noqa: E402
import _steps as S  # noqa: E402
from test_ins_rle_cpu import edge_maps  # noqa: E402

pytestmark = pytest.mark.gpu

os.environ.setdefault("MIOPEN_FIND_MODE", "2")     # fast find: the backbones are plumbing here, not the subject


def _dev():
    return torch.device("cuda", 0)


@contextlib.contextmanager
def _limit(seconds):
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _image(cls, c, rng, thr=0.0):
    """(score [c,h,w], class map, class ids, channels, min area) of one image, as the existing detection tests build them."""
    cls = np.asarray(cls).astype(np.int32)
    return (rng.rand(c, *cls.shape).astype(np.float32), cls, np.arange(50, 50 + c), c, thr)


def _kron(rng, h, w, c, p_bg):
    cls = np.kron(rng.randint(0, c + 1, size=((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), int))[:h, :w]
    cls[rng.rand(h, w) < p_bg] = 0
    return cls


def _call(fn, images, **kw):
    return fn([torch.from_numpy(im[0]).to(_dev()) for im in images], [torch.from_numpy(im[1]).to(_dev()) for im in images],
              [im[2] for im in images], [im[3] for im in images], [im[4] for im in images], **kw)


def _assert_same(got, want, what):
    assert set(got) == {"score", "class", "size", "counts", "offsets", "area", "bbox"}, what
    for k in ("score", "class", "counts", "offsets", "area", "bbox"):
        assert got[k].dtype == want[k].dtype, (what, k, got[k].dtype)
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    assert tuple(got["size"]) == tuple(want["size"]), what


def _check_against_dense(images, what):
    """detect_instance_rle_batch(images) == mask_rle of the dense path's masks (+ its scores and classes), field by field,
    and == the restatement of pycocotools on the host masks.  -> the rle results."""
    from irn_amd import ops
    with _limit(240):
        dense = _call(ops.detect_instance_batch, images)
        rle = _call(ops.detect_instance_rle_batch, images)
        torch.cuda.synchronize()
    assert len(rle) == len(dense) == len(images)
    for i, (d, r) in enumerate(zip(dense, rle)):
        if isinstance(d, Exception):
            assert isinstance(r, ValueError) and str(r) == str(d), (what, i)
            continue
        assert not isinstance(r, Exception), (what, i, r)
        with _limit(240):
            counts, offsets, area, bbox = ops.mask_rle(torch.from_numpy(d["mask"]).to(_dev()))
        want = {"score": d["score"], "class": d["class"], "size": d["mask"].shape[1:], "counts": counts, "offsets": offsets,
                "area": area, "bbox": bbox}
        _assert_same(r, want, (what, i))
        assert r["score"].dtype == np.float32 and r["class"].dtype == np.int64 and r["counts"].dtype == np.uint32
        assert r["offsets"].dtype == np.int64 and r["area"].dtype == np.int64 and r["bbox"].dtype == np.int32
        h_counts, h_offsets, h_area, h_bbox = R.mask_rle(d["mask"])
        assert np.array_equal(r["counts"], h_counts) and np.array_equal(r["offsets"], h_offsets), (what, i)
        assert np.array_equal(r["area"], h_area) and np.array_equal(r["bbox"], h_bbox), (what, i)
    return rle


def test_ragged_batch_with_an_empty_image_and_a_fragmented_one():
    """The batch of test_detect_instance_batch_vs_oracle_incl_empty_and_fragmented: an all-background image in the middle,
    a salt-and-pepper map with thousands of one-pixel detections, an area filter that zeroes scores."""
    rng = np.random.RandomState(11)
    images = []
    for (h, w, c, p_bg, thr) in ((37, 41, 5, 0.4, 0.0), (16, 16, 2, 1.0, 0.0), (96, 120, 7, 0.3, 0.0), (64, 80, 12, 0.2, 6.5)):
        cls = rng.randint(0, c + 1, size=(h, w)) if p_bg == 0.3 else _kron(rng, h, w, c, 0.0)
        cls[rng.rand(h, w) < p_bg] = 0
        images.append(_image(cls, c, rng, thr))
    rle = _check_against_dense(images, "ragged")
    assert isinstance(rle[1], ValueError)
    assert len(rle[2]["score"]) > 2048
    assert (rle[3]["score"] == 0).any() and (rle[3]["score"] > 0).any()          # area < min_area -> score 0


def test_random_maps_of_the_single_image_tests():
    rng = np.random.RandomState(5)
    images = []
    for (h, w, c, p_bg, thr) in ((37, 41, 5, 0.4, 0.0), (64, 80, 12, 0.2, 6.5), (128, 128, 3, 0.7, 163.84),
                                 (16, 16, 2, 0.0, 0.0), (33, 9, 40, 0.5, 2.0)):
        images.append(_image(_kron(rng, h, w, c, p_bg), c, rng, thr))
    _check_against_dense(images, "random")


def test_full_size_maps_crossing_many_tiles():
    """Spirals, combs, blocks and one region covering a whole VOC-size map (the shapes of
    test_detect_instance_full_size_maps_crossing_many_tiles): detections with tens of thousands of runs each."""
    rng = np.random.RandomState(23)

    def spiral(h, w):
        m = np.zeros((h, w), np.int32)
        y0, x0, y1, x1, k = 0, 0, h - 1, w - 1, 1
        while y0 <= y1 and x0 <= x1:
            m[y0, x0:x1 + 1] = k
            m[y0:y1 + 1, x1] = k
            if y1 > y0:
                m[y1, x0 + 2:x1 + 1] = k
            if x1 > x0 + 2:
                m[y0 + 2:y1 + 1, x0 + 2] = k
            y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
            k = 1 + (k % 3)
        return m

    def combs(h, w):
        m = np.zeros((h, w), np.int32)
        m[0, :] = 1
        m[h - 1, :] = 2
        m[1:h - 2, 0::4] = 1
        m[2:h - 1, 2::4] = 2
        return m

    maps = [spiral(512, 512), combs(512, 512), _kron(rng, 512, 512, 3, 0.0), np.full((375, 500), 2, np.int32), combs(333, 500),
            spiral(130, 67)]
    thrs = [0.0, 10.0, 0.0, 100.0, 0.0, 0.0]
    rle = _check_against_dense([_image(m, 3, rng, t) for m, t in zip(maps, thrs)], "full size")
    assert rle[3]["counts"].tolist() == [0, 375 * 500] and rle[3]["bbox"].tolist() == [[0, 0, 500, 375]]


def test_edge_maps():
    """The maps of tests/test_ins_rle_cpu.py as class maps (id -> one of 3 classes, -1 -> background), in ONE ragged batch
    together with an all-background image: 1x1, 1xW, Hx1, widths 63 / 64 / 65 / 129, a detection at pixel (0,0), one at the
    last pixel, one filling the map, a checkerboard of 2100 single-pixel detections."""
    rng = np.random.RandomState(31)
    maps = edge_maps()
    images = [_image(np.where(np.asarray(m) < 0, 0, np.asarray(m) % 3 + 1), 3, rng) for _, m in maps]
    images.insert(5, _image(np.zeros((20, 30), int), 3, rng))
    rle = _check_against_dense(images, "edge maps")
    assert isinstance(rle[5], ValueError)
    by_name = dict(zip([n for n, _ in maps], rle[:5] + rle[6:]))
    assert by_name["1x1"]["counts"].tolist() == [0, 1]
    assert by_name["one id fills the map"]["counts"].tolist() == [0, 12 * 17]
    assert len(by_name["checkerboard of 2100 single-pixel ids"]["score"]) == 2100
    assert by_name["id at (0,0)"]["counts"][0] == 0                               # the leading zero-run of 0
    last = by_name["id at the last pixel"]
    assert any(last["counts"][last["offsets"][d]:last["offsets"][d + 1]].size % 2 == 0 for d in range(len(last["score"])))


def test_image_alone_equals_image_in_a_batch_of_32_and_runs_repeat():
    from irn_amd import ops
    rng = np.random.RandomState(41)
    sizes = [(96, 128), (113, 150), (64, 80), (37, 41), (130, 67), (16, 16), (200, 333), (75, 100)]
    images = []
    for i in range(32):
        h, w = sizes[i % len(sizes)]
        c = 1 + i % 5
        cls = rng.randint(0, c + 1, size=(h, w)) if i % 7 == 3 else _kron(rng, h, w, c, 0.1 * (i % 4))
        if i == 9:
            cls[:] = 0                                                            # no detection
        images.append(_image(cls, c, rng, [0.0, 6.5][i % 2]))
    with _limit(300):
        first = _call(ops.detect_instance_rle_batch, images)
        second = _call(ops.detect_instance_rle_batch, images)
        deferred = _call(ops.detect_instance_rle_batch, images, deferred=True)
        other = _call(ops.detect_instance_rle_batch, images[:3])                   # enqueued while `deferred` is in flight
        assert isinstance(deferred, ops.PendingRleDetections)
        deferred = deferred.result()
        alone = [_call(ops.detect_instance_rle_batch, [im])[0] for im in images]
        torch.cuda.synchronize()
    assert isinstance(first[9], ValueError) and isinstance(alone[9], ValueError) and isinstance(deferred[9], ValueError)
    for i in range(32):
        if i == 9:
            continue
        _assert_same(second[i], first[i], ("second run", i))
        _assert_same(deferred[i], first[i], ("deferred", i))
        _assert_same(alone[i], first[i], ("alone", i))
    for i in range(3):
        _assert_same(other[i], first[i], ("batch of 3", i))
    empty = ops.detect_instance_rle_batch([torch.zeros(2, 8, 8, device=_dev())], [torch.zeros(8, 8, dtype=torch.int32, device=_dev())],
                                          [np.arange(2)], [2], [0.0], deferred=True).result()
    assert len(empty) == 1 and isinstance(empty[0], ValueError)


def test_cpu_tensors_and_wrong_shapes_are_refused():
    from irn_amd import ops
    with pytest.raises(ValueError):
        ops.detect_instance_rle_batch([torch.zeros(2, 8, 8)], [torch.zeros(8, 8, dtype=torch.int32)], [np.arange(2)], [2], [0.0])
    with pytest.raises(ValueError):
        ops.detect_instance_rle_batch([torch.zeros(3, 8, 8, device=_dev())], [torch.zeros(8, 8, dtype=torch.int32, device=_dev())],
                                      [np.arange(2)], [2], [0.0])


# ---------------------------------------------------------------------------------------------------------------------
# end to end through run_sample.py
# ---------------------------------------------------------------------------------------------------------------------
def _run(tmp_path, root, ins, out, extra):
    lst = str(tmp_path / "lists" / "train.txt")
    with _limit(900):
        return S.run_sample_main(["--voc12_root", str(root), "--train_list", lst, "--infer_list", lst, "--num_workers", "2",
                                  "--cam_weights_name", str(tmp_path / "res50_cam"),
                                  "--irn_weights_name", str(tmp_path / "res50_irn.pth"),
                                  "--cam_out_dir", str(tmp_path / "cam"), "--sem_seg_out_dir", str(tmp_path / "sem"),
                                  "--ins_seg_out_dir", str(ins), "--log_name", str(tmp_path / ins.name),
                                  "--cam_scales", "1.0", "0.5", "--make_sem_seg_pass", "False", "--eval_ins_seg_pass", "True",
                                  "--make_cocoann_pass", "True", "--cocoann_out", str(out)] + extra)


def test_run_sample_in_both_formats_gives_the_same_coco_file_and_ap(tmp_path, monkeypatch):
    from test_gpu_eval import _make_voc
    from irn_amd import ops
    from irn_amd.net import weights
    root, names = _make_voc(tmp_path)
    torch.save(weights.random_cam_state(1), tmp_path / "res50_cam.pth")
    torch.save(weights.random_irn_state(2), tmp_path / "res50_irn.pth")
    a = _run(tmp_path, root, tmp_path / "ins_npy", tmp_path / "A.json", [])
    timings = {}
    real = ops.detect_instance_rle_batch          # the step calls the operator; the test hands it a `timings` dict to fill
    monkeypatch.setattr(ops, "detect_instance_rle_batch", lambda *a, **kw: real(*a, **{**kw, "timings": timings}))
    b = _run(tmp_path, root, tmp_path / "ins_rle", tmp_path / "B.json", ["--make_cam_pass", "False", "--ins_seg_format", "rle"])
    monkeypatch.undo()
    assert (tmp_path / "A.json").read_bytes() == (tmp_path / "B.json").read_bytes()
    assert len(json.load(open(tmp_path / "A.json"))["annotations"]) > 0
    assert a["make_cocoann"] == b["make_cocoann"]
    assert a["eval_ins_seg"].keys() == b["eval_ins_seg"].keys()
    for k in a["eval_ins_seg"]:
        np.testing.assert_array_equal(a["eval_ins_seg"][k], b["eval_ins_seg"][k])
    npy, rle = sorted(os.listdir(tmp_path / "ins_npy")), sorted(os.listdir(tmp_path / "ins_rle"))
    assert npy and all(f.endswith(".npy") for f in npy)
    assert rle == [f[:-4] + ".rle.npz" for f in npy]                              # the same images, and no .npy among them
    # the files hold the dense path's masks, and the transfer that brought them is small
    bound = 0
    for f in npy:
        d = np.load(tmp_path / "ins_npy" / f, allow_pickle=True).item()
        with np.load(tmp_path / "ins_rle" / (f[:-4] + ".rle.npz"), allow_pickle=False) as z:
            counts, offsets, area, bbox = R.mask_rle(d["mask"])
            assert np.array_equal(z["counts"], counts) and np.array_equal(z["offsets"], offsets)
            assert np.array_equal(z["area"], area) and np.array_equal(z["bbox"], bbox)
            assert np.array_equal(z["score"], d["score"]) and np.array_equal(z["class"], d["class"])
            assert z["size"].tolist() == list(d["mask"].shape[1:])
            bound += 64 + 32 * len(z["score"]) + 4 * len(z["counts"])
    print("rle: %d bytes device-to-host for %d images (bound %d)" % (timings.get("bytes", -1), len(rle), bound))
    assert 0 < timings["bytes"] < bound
