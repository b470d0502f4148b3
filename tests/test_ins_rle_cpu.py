"""Instance labels as COCO run lengths, without a GPU: the id-map restatement of the kernels' algorithm
(tests/_detmap_rle_ref.py) equals the one-hot reference (tests/_cocomask_ref.py) mask by mask, run_sample.py parses
--ins_seg_format, the new C entries refuse bad arguments before anything touches a device, and make_cocoann builds the
annotations of an .rle.npz record on the host exactly as it builds them from dense masks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cocomask_ref as R  # noqa: E402
import _detmap_rle_ref as D  # noqa: E402


def _compact(idmap):
    """Renumber the ids that occur to 0..n-1 (ascending); -1 stays."""
    idmap = np.asarray(idmap)
    vals = np.unique(idmap[idmap >= 0])
    out = np.full(idmap.shape, -1, np.int64)
    for k, v in enumerate(vals):
        out[idmap == v] = k
    return out, len(vals)


def _blobs(rng, h, w, n, bg=0.3):
    """n seeds grown to nearest-seed cells, a share of the pixels background: ids with long shared borders."""
    yy, xx = np.mgrid[:h, :w]
    sy, sx = rng.randint(0, h, n), rng.randint(0, w, n)
    idmap = np.argmin((yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2, 0)
    idmap[rng.rand(h, w) < bg] = -1
    return idmap


def edge_maps():
    """(name, idmap) — the shapes and placements the issue lists."""
    rng = np.random.RandomState(7)
    maps = []
    for seed, (h, w, n) in enumerate(((7, 5, 3), (16, 16, 5), (13, 31, 9), (40, 70, 12), (33, 129, 20))):
        maps.append(("fuzz%d" % seed, rng.randint(-1, n, (h, w))))
        maps.append(("blobs%d" % seed, _blobs(rng, h, w, n)))
    maps.append(("1x1", np.zeros((1, 1), int)))
    maps.append(("1xW", rng.randint(-1, 3, (1, 37))))
    maps.append(("Hx1", rng.randint(-1, 3, (41, 1))))
    for w in (63, 64, 65, 129):
        maps.append(("w%d" % w, _blobs(rng, 19, w, 6)))
    first = np.full((9, 11), -1)
    first[:3, :2] = 0
    first[5:, 4:9] = 1
    maps.append(("id at (0,0)", first))
    last = np.full((9, 11), -1)
    last[6:, 8:] = 0
    last[1:4, 1:5] = 1
    maps.append(("id at the last pixel", last))
    maps.append(("one id fills the map", np.zeros((12, 17), int)))
    yy, xx = np.mgrid[:60, :70]
    maps.append(("checkerboard of 2100 single-pixel ids", np.where((yy + xx) % 2 == 0, (yy * 70 + xx) // 2, -1)))
    maps.append(("every pixel its own id", np.arange(48 * 64).reshape(48, 64)))
    return maps


@pytest.mark.parametrize("name,idmap", edge_maps(), ids=[m[0] for m in edge_maps()])
def test_idmap_restatement_equals_the_one_hot_reference(name, idmap):
    idmap, n = _compact(idmap)
    assert n >= 1
    counts, offsets, area, bbox = D.rle_from_idmap(idmap, n)
    masks = np.stack([idmap == d for d in range(n)])
    e_counts, e_offsets, e_area, e_bbox = R.mask_rle(masks)
    assert counts.dtype == np.uint32 and np.array_equal(counts, e_counts)
    assert np.array_equal(offsets, e_offsets)
    assert np.array_equal(area, e_area)
    assert np.array_equal(bbox, e_bbox)
    if "checkerboard" in name:
        assert n == 2100


def test_known_codes():
    idmap = np.array([[0, -1], [0, 1]])                      # column-major: 0 0 -1 1
    counts, offsets, area, bbox = D.rle_from_idmap(idmap, 2)
    assert counts.tolist() == [0, 2, 2, 3, 1] and offsets.tolist() == [0, 3, 5]        # leading zero-run of 0; no trailing count
    assert area.tolist() == [2, 1] and bbox.tolist() == [[0, 0, 1, 2], [1, 1, 1, 1]]
    counts, offsets, _, _ = D.rle_from_idmap(np.zeros((3, 4), int), 1)
    assert counts.tolist() == [0, 12] and offsets.tolist() == [0, 2]


def test_parser_ins_seg_format():
    import run_sample
    p = run_sample.build_parser()
    assert p.parse_args(["--voc12_root", "x"]).ins_seg_format == "npy"
    assert p.parse_args(["--voc12_root", "x", "--ins_seg_format", "rle"]).ins_seg_format == "rle"
    assert p.parse_args(["--voc12_root", "x", "--ins_seg_format", "npy"]).ins_seg_format == "npy"
    with pytest.raises(SystemExit):
        p.parse_args(["--voc12_root", "x", "--ins_seg_format", "png"])
    helps = [a.help for a in p._actions if a.dest == "ins_seg_format"]
    assert len(helps) == 1 and "not in the reference" in helps[0]
    assert run_sample.OUT_OF_SCOPE == ("train_cam_pass", "train_irn_pass")


def test_step_reads_the_format_with_a_default():
    from types import SimpleNamespace

    from irn_amd.step import make_ins_seg_labels as step
    assert step.ins_seg_format(SimpleNamespace()) == "npy"             # args built by hand, without the flag
    assert step.ins_seg_format(SimpleNamespace(ins_seg_format="rle")) == "rle"
    with pytest.raises(ValueError):
        step.ins_seg_format(SimpleNamespace(ins_seg_format="png"))


def test_rle_c_entries_refuse_bad_arguments_without_a_gpu():
    from irn_amd import _lib
    L = _lib.lib
    one = C.c_void_p(64)                                     # never dereferenced on these paths
    i32s = lambda *v: (C.c_int32 * len(v))(*v)               # noqa: E731
    h, w, nd, ch = i32s(4), i32s(4), i32s(2), i32s(1)
    area = (C.c_double * 1)(0.0)
    runs = (C.c_int64 * 1)(6)
    ptrs = (C.c_void_p * 1)(64)

    def count(n=1, rw=ptrs, am=ptrs, ch=ch, h=h, w=w, nd=nd, area=area, outs=(one,) * 5, scratch=one, rle_scratch=one):
        return L.irn_detect_instance_batch_rle_count(n, rw, am, ch, h, w, nd, area, *outs, scratch, rle_scratch, None)

    def emit(n=1, h=h, w=w, nd=nd, runs=runs, counts=one, rle_scratch=one, ws=one, ws_bytes=1 << 20):
        return L.irn_detect_instance_batch_rle_emit(n, h, w, nd, runs, counts, rle_scratch, ws, ws_bytes, None)

    for kw in ({"rw": None}, {"am": None}, {"ch": None}, {"h": None}, {"w": None}, {"nd": None}, {"area": None},
               {"scratch": None}, {"rle_scratch": None}, {"rw": (C.c_void_p * 1)(None)}, {"am": (C.c_void_p * 1)(None)},
               {"n": -1}, {"h": i32s(0)}, {"w": i32s(-3)}, {"h": i32s(65536), "w": i32s(32768)}, {"h": i32s(1 << 30), "w": i32s(2)},
               {"nd": i32s(-1)}, {"nd": i32s(17)}, {"ch": i32s(0)}):
        assert count(**kw) == 1, kw
        assert b"irn_detect_instance_batch_rle_count" in L.irn_last_error(), kw
    for i in range(5):                                       # every output in turn
        outs = [one] * 5
        outs[i] = None
        assert count(outs=tuple(outs)) == 1 and b"irn_detect_instance_batch_rle_count" in L.irn_last_error()
    for kw in ({"h": None}, {"w": None}, {"nd": None}, {"runs": None}, {"counts": None}, {"rle_scratch": None}, {"ws": None},
               {"ws_bytes": 8}, {"n": -1}, {"h": i32s(0)}, {"h": i32s(65536), "w": i32s(32768)}, {"h": i32s(1 << 30), "w": i32s(2)},
               {"nd": i32s(-1)}, {"nd": i32s(17)}, {"runs": (C.c_int64 * 1)(3)}, {"runs": (C.c_int64 * 1)(35)}):
        assert emit(**kw) == 1, kw
        assert b"irn_detect_instance_batch_rle_emit" in L.irn_last_error(), kw
    # an empty batch and a batch without detections: nothing to do, the arrays may be NULL
    assert L.irn_detect_instance_batch_rle_count(0, None, None, None, None, None, None, None, None, None, None, None, None,
                                                 None, None, None) == 0
    assert L.irn_detect_instance_batch_rle_emit(0, None, None, None, None, None, None, None, 0, None) == 0
    assert count(nd=i32s(0), outs=(None,) * 5) == 0
    assert emit(nd=i32s(0), runs=(C.c_int64 * 1)(0), counts=None, ws=None, ws_bytes=0) == 0
    S = L.irn_detect_instance_batch_rle_scratch_bytes
    assert S(-1, h, w, nd) == 0 and b"irn_detect_instance_batch_rle_scratch_bytes" in L.irn_last_error()
    assert S(1, None, w, nd) == 0 and S(1, h, w, i32s(17)) == 0 and S(1, i32s(1 << 30), i32s(2), nd) == 0
    assert S(0, None, None, None) == 0
    assert S(1, i32s(375), i32s(500), i32s(10)) >= 4 * 375 * 500 + 5 * 4 * 10
    two = S(2, i32s(375, 375), i32s(500, 500), i32s(10, 10))
    assert 2 * 4 * 375 * 500 <= two <= 2 * S(1, i32s(375), i32s(500), i32s(10))
    B = L.irn_detect_instance_batch_rle_sort_bytes
    assert B(-1, 0) == 0 and b"irn_detect_instance_batch_rle_sort_bytes" in L.irn_last_error()
    assert B(4, 5) == 0 and B((1 << 32) - 1, 1) == 0 and B(0, 0) == 0
    assert B(1000, 10) >= 2 * 8 * 1000


def _record(masks, score, cls):
    counts, offsets, area, bbox = R.mask_rle(masks)
    return {"score": np.asarray(score, np.float32), "class": np.asarray(cls, np.int64),
            "size": np.asarray(masks.shape[1:], np.int64), "counts": counts, "offsets": offsets, "area": area, "bbox": bbox}


def _expected(masks, score, cls, img_id, first_id):
    """The annotation dicts of the dense path, from the restatement (as `_cocomask_ref.cocoann` builds them)."""
    n, h, w = masks.shape
    out = []
    for s, m, c in zip(score, masks, cls):
        if s < 1e-5:
            continue
        k = R.encode(m)
        out.append({"id": first_id + len(out), "image_id": img_id, "category_id": int(c) + 1, "iscrowd": 0, "area": R.area(k),
                    "bbox": [float(v) for v in R.to_bbox(k, h, w)], "segmentation": {"size": [h, w], "counts": R.to_string(k)},
                    "width": w, "height": h})
    return out


def test_make_cocoann_builds_the_annotations_of_an_rle_record_on_the_host(tmp_path):
    import json

    from irn_amd.step import make_cocoann, make_ins_seg_labels
    rng = np.random.RandomState(3)
    idmap = _blobs(rng, 23, 37, 6)
    idmap[0, 0], idmap[-1, -1] = 0, 5
    idmap, n = _compact(idmap)
    masks = np.stack([idmap == d for d in range(n)])
    score = np.asarray([0.9, 0.0, 0.5, 9e-6, 1e-5, 0.25][:n], np.float32)
    cls = np.asarray([14, 0, 19, 7, 7, 3][:n])
    rec = _record(masks, score, cls)
    want = _expected(masks, score, cls, 2007000032, 11)
    anns, low = make_cocoann.rle_record_annotations(rec, 2007000032, 23, 37, 11, "2007_000032")
    assert low == 2 and len(anns) == n - 2
    assert anns == want
    assert [type(v) for v in anns[0]["bbox"]] == [float] * 4 and type(anns[0]["area"]) is int
    assert json.dumps(anns) == json.dumps(want)              # key order included
    # through the file the step writes: plain arrays, no pickle, size as int64[2]
    path = str(tmp_path / "2007_000032.rle.npz")
    make_ins_seg_labels.save_rle(path, dict(rec, size=(23, 37)))
    assert os.listdir(str(tmp_path)) == ["2007_000032.rle.npz"]
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["area", "bbox", "class", "counts", "offsets", "score", "size"]
        assert z["size"].dtype == np.int64 and z["size"].tolist() == [23, 37]
        assert z["counts"].dtype == np.uint32 and z["offsets"].dtype == np.int64 and z["bbox"].dtype == np.int32
        again, low2 = make_cocoann.rle_record_annotations(z, 2007000032, 23, 37, 11, "2007_000032")
    assert again == want and low2 == 2
    # a record that is not of the JPEG's size is an error that names the image
    with pytest.raises(ValueError, match="2007_000032.*23, 37.*37x23"):
        make_cocoann.rle_record_annotations(rec, 2007000032, 37, 23, 1, "2007_000032")
    with pytest.raises(ValueError, match="2007_000032"):
        make_cocoann.rle_record_annotations(dict(rec, offsets=rec["offsets"][:-1]), 2007000032, 23, 37, 1, "2007_000032")
    with pytest.raises(ValueError, match="class outside"):
        make_cocoann.rle_record_annotations(dict(rec, **{"class": cls + 15}), 1, 23, 37, 1)
    # no detections at all
    empty = _record(np.zeros((0, 23, 37), bool), [], [])
    assert make_cocoann.rle_record_annotations(empty, 1, 23, 37, 1) == ([], 0)


def test_eval_ins_seg_decodes_an_rle_record(tmp_path):
    from irn_amd.step import eval_ins_seg, make_ins_seg_labels
    rng = np.random.RandomState(4)
    idmap, n = _compact(_blobs(rng, 21, 30, 4))
    masks = np.stack([idmap == d for d in range(n)])
    rec = _record(masks, rng.rand(n), rng.randint(0, 20, n))
    path = str(tmp_path / "a.rle.npz")
    make_ins_seg_labels.save_rle(path, rec)
    det = eval_ins_seg.load_rle(path)
    assert det["mask"].dtype == np.bool_ and np.array_equal(det["mask"], masks)
    assert np.array_equal(det["score"], rec["score"]) and np.array_equal(det["class"], rec["class"])
