"""The polygon definition of `ops.mask_polygons` (include/irn_hip.h "COCO mask polygons") held to its claims on the plain-loop
restatement tests/_polygon_ref.py, `ops.polygon_fill` against it, the step's polygon annotations, and the argument refusals of
the new C entries.  No GPU: tests/test_gpu_polygon.py holds the kernels to the same restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cocomask_ref as R  # noqa: E402
import _polygon_ref as P  # noqa: E402


def _fuzz():
    rng = np.random.RandomState(7)
    out = []
    for density in (0.2, 0.5, 0.8):
        for _ in range(25):
            h, w = rng.randint(1, 14, 2)
            out.append(("fuzz_%.1f_%dx%d_%d" % (density, h, w, len(out)), rng.rand(h, w) < density))
    return out


CASES = sorted(P.hand_cases().items()) + _fuzz()


@pytest.fixture(scope="module")
def traced():
    """name -> (mask, all loops of the restatement), computed once."""
    return {name: (mask, P.all_loops(mask)) for name, mask in CASES}


def _arrays(loops):
    """(xy, loop_offsets) of a list of corner lists."""
    off = np.zeros(len(loops) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in loops]) if loops else []
    return np.asarray([v for c in loops for v in c], np.int32).reshape(-1, 2), off


def test_there_are_enough_cases(traced):
    assert len(CASES) == 75 + 13
    assert sum(1 for _, loops in traced.values() if any(a < 0 for _, a, _ in loops)) >= 10      # masks with holes
    assert sum(1 for _, loops in traced.values() if sum(a > 0 for _, a, _ in loops) >= 3) >= 20


def test_outer_loops_are_the_4_connected_components_and_holes_the_enclosed_background(traced):
    for name, (mask, loops) in traced.items():
        assert all(a != 0 for _, a, _ in loops), name
        assert sum(a > 0 for _, a, _ in loops) == P.components4(mask), name
        assert sum(a < 0 for _, a, _ in loops) == P.enclosed_background(mask)[0], name
        assert sum(n for _, _, n in loops) == len(P.edge_set(mask)), name          # the successor map is a permutation


def test_fills_give_the_mask_back(traced):
    from irn_amd import ops
    for name, (mask, loops) in traced.items():
        h, w = mask.shape
        outer = [c for c, a, _ in loops if a > 0]
        filled = ops.polygon_fill(*_arrays(outer), h, w)
        assert filled.dtype == np.bool_ and filled.shape == (h, w)
        assert np.array_equal(filled, P.fill_holes(mask)), name
        xor = np.zeros((h, w), bool)
        union = np.zeros((h, w), bool)
        for c, a, _ in loops:
            one = ops.polygon_fill(*_arrays([c]), h, w)
            assert np.array_equal(one, P.loop_fill(c, h, w)), name                 # the vectorised fill is the pixel-by-pixel one
            xor ^= one
            union |= one if a > 0 else False
        assert np.array_equal(xor, mask), name
        assert np.array_equal(union, filled), name


def test_canonical_form(traced):
    for name, (mask, loops) in traced.items():
        outer = [c for c, a, _ in loops if a > 0]
        starts = []
        for c in outer:
            assert len(c) >= 4 and len(c) % 2 == 0, name
            start = min(c, key=lambda v: (v[1], v[0]))
            assert c[0] == start and c.count(start) == 1, name
            assert c[1][1] == c[0][1] and c[1][0] > c[0][0], name                  # the first edge runs in +x
            for i in range(len(c)):                                               # corners only, axis-parallel sides
                (x0, y0), (x1, y1), (x2, y2) = c[i - 1], c[i], c[(i + 1) % len(c)]
                assert (x0 == x1) != (y0 == y1) and (x0 == x1) != (x1 == x2), name
            starts.append((start[1], start[0]))
        assert starts == sorted(starts) and len(set(starts)) == len(starts), name
        for c, a, _ in loops:
            assert len(c) >= 4 and len(c) % 2 == 0, name


def test_hand_cases():
    cases = P.hand_cases()
    assert P.all_loops(cases["one_clear"]) == []
    assert P.outer_loops(cases["one_set"]) == [[(0, 0), (1, 0), (1, 1), (0, 1)]]
    assert P.outer_loops(cases["diagonal"]) == [[(0, 0), (1, 0), (1, 1), (0, 1)], [(1, 1), (2, 1), (2, 2), (1, 2)]]
    assert P.outer_loops(cases["anti_diagonal"]) == [[(1, 0), (2, 0), (2, 1), (1, 1)], [(0, 1), (1, 1), (1, 2), (0, 2)]]
    ring = P.all_loops(cases["ring"])
    assert [(c, a) for c, a, _ in ring if a > 0] == [([(0, 0), (3, 0), (3, 3), (0, 3)], 18)]
    assert [a for _, a, _ in ring if a < 0] == [-2]
    pinch = P.all_loops(cases["pinch"])
    assert len(pinch) == 1 and pinch[0][1] == 2 * 7
    assert pinch[0][0] == [(0, 0), (3, 0), (3, 2), (2, 2), (2, 1), (1, 1), (1, 2), (2, 2), (2, 3), (0, 3)]
    _, _, mask_loops, holes = P.mask_polygons(np.stack([cases["nested"]]))
    assert mask_loops.tolist() == [0, 2] and holes.tolist() == [1]
    _, _, mask_loops, holes = P.mask_polygons(np.stack([cases["nested2"]]))
    assert mask_loops.tolist() == [0, 2] and holes.tolist() == [2]


@pytest.mark.parametrize("h,w,y0,y1,x0,x1", [(1, 1, 0, 1, 0, 1), (5, 7, 1, 4, 2, 6), (9, 4, 0, 9, 0, 4), (6, 6, 5, 6, 0, 6)])
def test_a_rectangle_is_the_corners_of_its_bbox(h, w, y0, y1, x0, x1):
    mask = np.zeros((h, w), bool)
    mask[y0:y1, x0:x1] = True
    bx, by, bw, bh = R.tight_bbox(mask)
    assert R.to_bbox(R.encode(mask), h, w) == [bx, by, bw, bh]
    assert P.outer_loops(mask) == [[(bx, by), (bx + bw, by), (bx + bw, by + bh), (bx, by + bh)]]


def test_polygon_fill_refuses_what_is_not_a_polygon_list():
    from irn_amd import ops
    with pytest.raises(ValueError):
        ops.polygon_fill(np.zeros((4, 2), np.int32), [0, 3], 4, 4)
    with pytest.raises(ValueError):
        ops.polygon_fill(np.int32([[0, 0], [5, 0], [5, 1], [0, 1]]), [0, 4], 4, 4)
    assert not ops.polygon_fill(np.zeros((0, 2), np.int32), [0], 3, 5).any()


def test_polygon_annotations_equal_the_rle_ones_but_for_the_segmentation():
    """The step's annotation builder on a small set of images: with the restatement's polygons it gives what it gives
    with the run lengths in every field but `segmentation`, which holds the loops as integer lists."""
    import json
    from irn_amd.step import make_cocoann
    rng = np.random.RandomState(5)
    cases = P.hand_cases()
    first_id = 1
    for img_id, (h, w, extra) in enumerate([(9, 11, "nested2"), (7, 7, "nested"), (5, 6, None)]):
        masks = [rng.rand(h, w) < p for p in (0.3, 0.7)] + ([cases[extra]] if extra else [])
        masks = np.stack(masks)
        counts, offsets, area, bbox = R.mask_rle(masks)
        kept = {"class": np.arange(len(masks)) % 20, "counts": counts, "offsets": offsets, "area": area, "bbox": bbox}
        xy, loop_offsets, mask_loops, _ = P.mask_polygons(masks)
        rle = make_cocoann.annotations(kept, img_id, h, w, first_id)
        poly = make_cocoann.annotations(kept, img_id, h, w, first_id, (xy, loop_offsets, mask_loops))
        assert len(rle) == len(poly) == len(masks)
        assert json.loads(json.dumps(poly)) == poly                               # plain ints: nothing numpy reaches json
        for a, b, m in zip(rle, poly, masks):
            assert list(a) == list(b)                                             # the same keys in the same order
            assert {k: v for k, v in a.items() if k != "segmentation"} == {k: v for k, v in b.items() if k != "segmentation"}
            seg = b["segmentation"]
            assert isinstance(seg, list) and all(isinstance(v, int) for loop in seg for v in loop)
            assert seg == [[v for xy_ in c for v in xy_] for c in P.outer_loops(m)]
        first_id += len(masks)


def test_argument_refusals_need_no_gpu():
    from irn_amd import _lib
    L = _lib.lib
    one = C.c_void_p(64)                                                           # never dereferenced on these paths
    assert L.irn_mask_polygon_scratch_bytes(1, 0, 4) == 0 and b"irn_mask_polygon_scratch_bytes" in L.irn_last_error()
    assert L.irn_mask_polygon_scratch_bytes(-1, 4, 4) == 0
    assert L.irn_mask_polygon_scratch_bytes(1, 46341, 46341) == 0                  # h*w >= 2^31 - 1
    assert L.irn_mask_polygon_scratch_bytes(6000, 375, 500) == 0                  # 2*n*(h+1)*(w+1) >= 2^31
    assert L.irn_mask_polygon_scratch_bytes(0, 4, 4) == 0
    assert L.irn_mask_polygon_scratch_bytes(2, 3, 3) == 4 * 4 + 2 * 256 * 2        # 16 grid points: one workgroup per mask
    assert L.irn_mask_polygon_trace_scratch_bytes(-1) == 0 and b"irn_mask_polygon_trace_scratch_bytes" in L.irn_last_error()
    assert L.irn_mask_polygon_trace_scratch_bytes(0) == 0
    assert L.irn_mask_polygon_trace_scratch_bytes(100) >= 53 * 100
    assert L.irn_mask_polygon_edges(None, 1, 4, 4, one, one, None) == 1 and b"irn_mask_polygon_edges" in L.irn_last_error()
    assert L.irn_mask_polygon_edges(one, 1, 4, 4, None, one, None) == 1
    assert L.irn_mask_polygon_edges(one, 1, 4, 0, one, one, None) == 1
    assert L.irn_mask_polygon_edges(None, 0, 4, 4, None, None, None) == 0          # no masks: nothing to do
    assert L.irn_mask_polygon_count(one, 1, 4, 4, one, 8, 9, one, one, one, one, one, None) == 1   # longest > all
    assert b"irn_mask_polygon_count" in L.irn_last_error()
    assert L.irn_mask_polygon_count(one, 1, 4, 4, one, -1, 0, one, one, one, one, one, None) == 1
    assert L.irn_mask_polygon_count(one, 1, 4, 4, one, 8, 8, one, None, one, one, one, None) == 1
    assert L.irn_mask_polygon_count(one, 1, 4, 4, one, 8, 8, one, one, one, one, None, None) == 1  # edges, no trace scratch
    assert L.irn_mask_polygon_count(None, 0, 4, 4, None, 0, 0, None, None, None, None, None, None) == 0
    assert L.irn_mask_polygon_emit(-1, one, 1, one, 1, one, None) == 1 and b"irn_mask_polygon_emit" in L.irn_last_error()
    assert L.irn_mask_polygon_emit(8, None, 1, one, 4, one, None) == 1
    assert L.irn_mask_polygon_emit(8, one, 1, one, -4, one, None) == 1
    assert L.irn_mask_polygon_emit(8, one, 1, one, 4, None, None) == 1
    assert L.irn_mask_polygon_emit(0, None, 0, None, 0, None, None) == 0           # no edges: nothing to write


def test_mask_polygons_refuses_cpu_tensors():
    import torch
    from irn_amd import ops
    with pytest.raises(ValueError):
        ops.mask_polygons(torch.zeros((1, 4, 4), dtype=torch.uint8))
