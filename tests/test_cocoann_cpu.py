"""COCO export without a GPU: the restatement of pycocotools' mask arithmetic (tests/_cocomask_ref.py) checks itself,
the host-side string / decode functions of irn_amd.ops equal it, run_sample.py parses the new flags, and the three C
entries refuse bad arguments before anything touches a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cocomask_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_masks(rng):
    out = [rng.rand(h, w) < p for h, w, p in ((7, 5, 0.5), (1, 9, 0.5), (9, 1, 0.5), (16, 16, 0.1), (13, 31, 0.9))]
    for h, w in ((12, 17), (30, 8)):                       # rectangles, some touching a border or a corner
        for _ in range(6):
            y0, x0 = rng.randint(0, h), rng.randint(0, w)
            y1, x1 = rng.randint(y0, h) + 1, rng.randint(x0, w) + 1
            m = np.zeros((h, w), bool)
            m[y0:y1, x0:x1] = True
            out.append(m)
    out += [np.zeros((4, 6), bool), np.ones((4, 6), bool)]
    seam = np.zeros((5, 4), bool)                          # one run from the foot of column 1 into the head of column 2
    seam[3:, 1] = True
    seam[:2, 2] = True
    out.append(seam)
    return out


def _count_lists(rng):
    """Counts that exercise the string code: zeros, values >= 2^20, negative differences to the count before last."""
    lists = [[0], [1, 3], [0, 24], [5], [1, 1, 1, 1, 1, 1], [0, 1 << 20, 3, 1, (1 << 31) - 1, 0, 7],
             [100000, 5, 99000, 1, 7, 1 << 25, 0, 0, 0, 15, 16, 31, 32, 1023, 1024, 32767, 32768],
             [(1 << 32) - 1, 0, 0, (1 << 32) - 1, (1 << 32) - 1, 0, 0]]
    for n in (1, 2, 3, 4, 50, 1000):
        scale = 2 ** rng.randint(0, 31, n).astype(np.float64)
        c = (rng.rand(n) * scale).astype(np.int64)
        c[rng.rand(n) < 0.2] = 0
        lists.append(c.tolist())
    assert any(c[i] - c[i - 2] < 0 for c in lists for i in range(3, len(c)))
    assert any(v >= 1 << 20 for c in lists for v in c) and any(v == 0 for c in lists for v in c)
    return lists


def test_restatement_known_values():
    m = np.array([[0, 1], [1, 1]])
    assert R.encode(m).tolist() == [1, 3] and R.encode_loop(m).tolist() == [1, 3]
    assert R.to_string([1, 3]) == "13"
    assert R.area([1, 3]) == 3 and R.to_bbox([1, 3], 2, 2) == [0, 0, 2, 2]
    assert R.encode(np.zeros((3, 4))).tolist() == [12] and R.encode(np.ones((3, 4))).tolist() == [0, 12]
    assert R.to_bbox([12], 3, 4) == [0, 0, 0, 0] and R.to_bbox([0, 12], 3, 4) == [0, 0, 4, 3]
    assert R.encode(np.array([[2, 255, 0, 1]])).tolist() == [0, 2, 1, 1]          # any nonzero value reads as 1
    yy, xx = np.mgrid[:64, :64]
    board = (yy + xx) % 2 == 1
    assert len(R.encode(board)) == 4033 and len(R.encode(~board)) == 4034        # runs merge at the seams of an even height
    assert len(R.encode(board[:63])) == 63 * 64 and len(R.encode(~board[:63])) == 63 * 64 + 1   # none merge at an odd one


def test_restatement_round_trips():
    rng = np.random.RandomState(0)
    for m in _random_masks(rng):
        h, w = m.shape
        c = R.encode(m)
        assert np.array_equal(c, R.encode_loop(m))
        assert int(c.astype(np.int64).sum()) == h * w
        assert np.array_equal(R.decode(c, h, w), m)
        assert R.area(c) == int(m.sum())
        assert R.to_bbox(c, h, w) == R.tight_bbox(m)
        assert np.array_equal(R.from_string(R.to_string(c)), c)
    for c in _count_lists(rng):
        s = R.to_string(c)
        assert all("0" <= ch <= "o" for ch in s)
        assert R.from_string(s).tolist() == c


def test_ops_host_functions_equal_the_restatement():
    from irn_amd import ops
    rng = np.random.RandomState(1)
    for c in _count_lists(rng):
        s = ops.rle_to_string(np.asarray(c, np.uint32))
        assert s == R.to_string(c)
        back = ops.rle_from_string(s)
        assert back.dtype == np.uint32 and back.tolist() == c
        assert ops.rle_from_string(s.encode("ascii")).tolist() == c
    assert ops.rle_to_string(np.zeros(0, np.uint32)) == "" and ops.rle_from_string("").size == 0
    for m in _random_masks(rng):
        h, w = m.shape
        c = R.encode(m)
        got = ops.rle_decode(c, h, w)
        assert got.dtype == np.bool_ and np.array_equal(got, R.decode(c, h, w)) and np.array_equal(got, m)
        assert ops.rle_to_string(c) == R.to_string(c)
    with pytest.raises(ValueError):
        ops.rle_decode([3, 4], 2, 2)
    with pytest.raises(ValueError):
        ops.rle_from_string("1P")                          # ends inside a count


def test_worst_case_voc_size_mask_string_round_trip():
    """The worst case of a VOC-size mask (one count per pixel) goes through the vectorised coder and comes back."""
    from irn_amd import ops
    yy, xx = np.mgrid[:375, :500]
    c = R.encode((yy + xx) % 2 == 1)
    s = ops.rle_to_string(c)
    assert np.array_equal(ops.rle_from_string(s), c)
    assert s.startswith(R.to_string(c[:150])) and len(s) >= len(c)


def test_restatement_against_pycocotools():
    mask_util = pytest.importorskip("pycocotools.mask")
    rng = np.random.RandomState(2)
    for m in _random_masks(rng):
        h, w = m.shape
        rle = mask_util.encode(np.asfortranarray(m.astype(np.uint8)))
        c = R.encode(m)
        assert rle["counts"].decode("ascii") == R.to_string(c)
        assert int(mask_util.area(rle)) == R.area(c)
        assert [int(v) for v in mask_util.toBbox(rle)] == R.to_bbox(c, h, w)
        assert np.array_equal(mask_util.decode(rle).astype(bool), R.decode(c, h, w))


def test_parser_flags():
    import run_sample
    p = run_sample.build_parser()
    a = p.parse_args(["--voc12_root", "x"])
    assert a.make_cocoann_pass is False and a.cocoann_out == "voc2012_train_custom.json"
    a = p.parse_args(["--voc12_root", "x", "--make_cocoann_pass", "True", "--cocoann_out", "x.json"])
    assert a.make_cocoann_pass is True and a.cocoann_out == "x.json"
    assert run_sample.OUT_OF_SCOPE == ("train_cam_pass", "train_irn_pass")


def test_categories_are_the_voc_classes_in_order():
    from irn_amd.step import make_cocoann
    cats = make_cocoann.categories()
    assert [c["id"] for c in cats] == list(range(1, 21))
    assert [c["name"] for c in cats] == R.CATEGORIES and cats[0]["name"] == "aeroplane" and cats[14]["name"] == "person"
    assert all(c["supercategory"] == "none" for c in cats)


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    from irn_amd import _lib
    L = _lib.lib
    one = C.c_void_p(64)                                   # never dereferenced on these paths
    ok_count = (one, 1, 4, 4, one, one, one, one, None)
    for i in (0, 4, 5, 6, 7):                              # every pointer in turn
        args = list(ok_count)
        args[i] = None
        assert L.irn_mask_rle_count(*args) == 1 and b"irn_mask_rle_count" in L.irn_last_error()
    for n, h, w in ((-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -3, 4), (1, 65536, 32768), (1, 1 << 30, 2)):
        assert L.irn_mask_rle_count(one, n, h, w, one, one, one, one, None) == 1
        assert b"irn_mask_rle_count" in L.irn_last_error()
        assert L.irn_mask_rle_emit(one, n, h, w, one, one, one, None) == 1
        assert b"irn_mask_rle_emit" in L.irn_last_error()
        assert L.irn_mask_rle_scratch_bytes(n, h, w) == 0
        assert b"irn_mask_rle_scratch_bytes" in L.irn_last_error()
    ok_emit = (one, 1, 4, 4, one, one, one, None)
    for i in (0, 4, 5, 6):
        args = list(ok_emit)
        args[i] = None
        assert L.irn_mask_rle_emit(*args) == 1 and b"irn_mask_rle_emit" in L.irn_last_error()
    # n == 0: nothing to do, every array may be NULL
    assert L.irn_mask_rle_count(None, 0, 4, 4, None, None, None, None, None) == 0
    assert L.irn_mask_rle_emit(None, 0, 4, 4, None, None, None, None) == 0
    assert L.irn_mask_rle_scratch_bytes(0, 4, 4) == 0
    assert L.irn_mask_rle_scratch_bytes(1, 375, 500) > 0
    assert L.irn_mask_rle_scratch_bytes(40, 375, 500) == 40 * L.irn_mask_rle_scratch_bytes(1, 375, 500)
