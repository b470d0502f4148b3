"""The polygon tracer (irn_amd/csrc/cocomask.hip through ops.mask_polygons) against the plain-loop restatement of its
definition (tests/_polygon_ref.py): integer equality of all four arrays in every case.

The seams of the kernels' decomposition, and the cases that cross them:
    256 grid points per workgroup     (h+1)*(w+1) at 256 exactly (15x15, 3x63), just past it (3x64, 1x129) and many workgroups
    256 edges per workgroup           every mask with more than 256 edges; the loop-offset scan runs over these workgroups
    1024 workgroup sums per scan pass two 375x500 masks (1472 workgroups of grid points); a 363x363 checkerboard (263 540
                                      edges, 1030 workgroups of edges: the three-column scan carries into a second pass)
    jumping rounds R (made even)      a single loop of 4096 unit edges (R = 12) and the next possible length, 4098 (a closed
                                      lattice loop has an even length; R = 13 -> 14); a serpentine of more than 4096 edges
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _polygon_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _same(got, want, what=""):
    names = ("xy", "loop_offsets", "mask_loops", "holes")
    dtypes = (np.int32, np.int64, np.int64, np.int64)
    for name, dtype, g, w in zip(names, dtypes, got, want):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name)


def _check(masks, tensor=None, what=""):
    """ops.mask_polygons(masks) == the restatement, in every integer; `tensor` = the GPU tensor to pass instead of an upload."""
    from irn_amd import ops
    masks = np.asarray(masks)
    got = ops.mask_polygons(torch.from_numpy(masks).to(_dev()) if tensor is None else tensor)
    assert got[0].ndim == 2 and got[0].shape[1] == 2
    _same(got, P.mask_polygons(masks), what)
    return got


def _blobs(n, h, w, seed):
    """Blob masks with a few stray pixels and stray gaps (tests/test_gpu_cocoann.py builds its masks the same way)."""
    from irn_amd import synth
    cams = synth.cam_blobs(n, (h + 3) // 4, (w + 3) // 4, seed=seed)
    up = torch.nn.functional.interpolate(torch.from_numpy(cams)[None], size=(h, w), mode="bilinear", align_corners=False)[0]
    rng = np.random.RandomState(seed)
    return ((up.numpy() > rng.uniform(0.2, 0.7, (n, 1, 1))) | (rng.rand(n, h, w) < 0.002)) & ~(rng.rand(n, h, w) < 0.002)


@pytest.mark.parametrize("name", sorted(P.hand_cases()))
def test_hand_cases(name):
    mask = P.hand_cases()[name]
    xy, loop_offsets, mask_loops, holes = _check(mask[None], what=name)
    if name == "one_set":
        assert xy.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
    if name == "one_clear":
        assert xy.shape == (0, 2) and loop_offsets.tolist() == [0] and mask_loops.tolist() == [0, 0] and holes.tolist() == [0]
    if name in ("diagonal", "anti_diagonal"):
        assert loop_offsets.tolist() == [0, 4, 8]
    if name == "ring":
        assert loop_offsets.tolist() == [0, 4] and holes.tolist() == [1]
    if name == "pinch":
        assert loop_offsets.tolist() == [0, 10] and holes.tolist() == [0] and xy.tolist().count([2, 2]) == 2
    if name == "nested":
        assert mask_loops.tolist() == [0, 2] and holes.tolist() == [1]


def test_all_hand_cases_padded_into_one_batch():
    cases = P.hand_cases()
    batch = np.zeros((len(cases), 9, 11), bool)
    for i, name in enumerate(sorted(cases)):
        m = cases[name]
        batch[i, :m.shape[0], :m.shape[1]] = m
    _check(batch)


def test_empty_and_full_mask_in_one_batch():
    h, w = 37, 70
    masks = np.zeros((4, h, w), bool)
    masks[1] = True
    masks[3, 5:9, 60:] = True
    xy, loop_offsets, mask_loops, holes = _check(masks)
    assert mask_loops.tolist() == [0, 0, 1, 1, 2] and holes.tolist() == [0, 0, 0, 0]
    assert xy[:4].tolist() == [[0, 0], [w, 0], [w, h], [0, h]]
    assert xy[4:].tolist() == [[60, 5], [70, 5], [70, 9], [60, 9]]


@pytest.mark.parametrize("h,w", [(1, 300), (300, 1), (1, 2), (2, 1)])
def test_thin_masks_with_runs(h, w):
    rng = np.random.RandomState(h * 1000 + w)
    _check(np.stack([rng.rand(h, w) < p for p in (0.5, 0.1, 0.9)] + [np.ones((h, w), bool)]))


@pytest.mark.parametrize("h,w", [(5, 5), (64, 63)])
def test_checkerboards(h, w):
    yy, xx = np.mgrid[:h, :w]
    board = (yy + xx) % 2 == 0
    xy, loop_offsets, mask_loops, holes = _check(np.stack([board, ~board]))
    assert np.array_equal(np.diff(loop_offsets), np.full(h * w, 4))                # one 4-corner loop per set pixel
    assert mask_loops.tolist() == [0, int(board.sum()), h * w] and holes.tolist() == [0, 0]


def test_checkerboard_past_1024_workgroups_of_edges():
    """363x363: 65 885 set pixels, 263 540 edges.  The expected arrays are written down directly (pixel (x, y) in raster
    order gives (x, y), (x+1, y), (x+1, y+1), (x, y+1)), and the restatement agrees with that form on the small boards."""
    from irn_amd import ops
    h = w = 363
    yy, xx = np.mgrid[:h, :w]
    board = (yy + xx) % 2 == 0
    ys, xs = np.nonzero(board)
    want = np.stack([np.stack([xs, ys], 1), np.stack([xs + 1, ys], 1), np.stack([xs + 1, ys + 1], 1), np.stack([xs, ys + 1], 1)], 1)
    assert 4 * len(ys) == 263540 > 1024 * 256
    small = (np.mgrid[:5, :5].sum(0) % 2 == 0)
    sy, sx = np.nonzero(small)
    assert P.outer_loops(small) == [[(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)] for y, x in zip(sy.tolist(), sx.tolist())]
    xy, loop_offsets, mask_loops, holes = ops.mask_polygons(torch.from_numpy(board[None]).to(_dev()))
    assert np.array_equal(xy, want.reshape(-1, 2).astype(np.int32))
    assert np.array_equal(loop_offsets, 4 * np.arange(len(ys) + 1)) and mask_loops.tolist() == [0, len(ys)] and holes.tolist() == [0]


@pytest.mark.parametrize("w", [63, 64, 65, 129])
@pytest.mark.parametrize("h", [1, 3, 4, 15])
def test_widths_and_heights_across_the_workgroup_seams(h, w):
    rng = np.random.RandomState(h * 1000 + w)
    masks = [rng.rand(h, w) < p for p in (0.5, 0.15, 0.85)] + [np.ones((h, w), bool)]
    last = np.zeros((h, w), bool)
    last[h - 1, w - 1] = True                              # the last grid points of the mask hold its only edges
    _check(np.stack(masks + [last]))


def test_15x15_is_exactly_one_workgroup_of_grid_points():
    rng = np.random.RandomState(15)
    _check(np.stack([rng.rand(15, 15) < 0.6, np.ones((15, 15), bool)]))


def test_serpentine_needs_more_than_twelve_rounds():
    mask = P.serpentine(65, 65)
    loops = P.all_loops(mask)
    assert len(loops) == 1 and loops[0][2] > 4096          # one loop, across many workgroups of edges
    xy, loop_offsets, mask_loops, holes = _check(np.stack([mask, mask.T.copy()]))
    assert mask_loops.tolist() == [0, 1, 2] and holes.tolist() == [0, 0]


@pytest.mark.parametrize("length", [4096, 4098])
def test_loop_length_at_a_power_of_two(length):
    """A 3-row bar: a single loop of 2 * (3 + w) unit edges and nothing else in the call, so the number of rounds follows
    from exactly this length."""
    w = length // 2 - 3
    mask = np.ones((3, w), bool)
    assert P.all_loops(mask)[0][2] == length
    xy, _, _, _ = _check(mask[None])
    assert xy.tolist() == [[0, 0], [w, 0], [w, 3], [0, 3]]
    pierced = mask.copy()
    pierced[1, 1:w - 1:2] = False                          # the same outer loop around a thousand one-pixel holes
    assert P.all_loops(pierced)[0][1:] == (2 * 3 * w, length)
    _, _, _, holes = _check(pierced[None])
    assert holes.tolist() == [len(range(1, w - 1, 2))]


def test_blobs_at_voc_size():
    masks = _blobs(2, 375, 500, seed=875)                  # two masks: 1472 workgroups of grid points
    assert masks.any() and not masks.all()
    _, _, mask_loops, holes = _check(masks)
    assert mask_loops[-1] >= 2


def test_any_nonzero_value_is_in_the_mask():
    from irn_amd import ops
    rng = np.random.RandomState(3)
    bits = rng.rand(3, 50, 77) < 0.4
    values = np.where(bits, rng.choice(np.uint8([1, 2, 255, 128]), bits.shape), 0).astype(np.uint8)
    _same(ops.mask_polygons(torch.from_numpy(values).to(_dev())), _check(bits))


def test_bool_and_uint8_inputs():
    from irn_amd import ops
    bits = _blobs(2, 40, 53, seed=4)
    _same(ops.mask_polygons(torch.from_numpy(bits.astype(np.uint8)).to(_dev())), _check(bits))


def test_non_contiguous_view():
    rng = np.random.RandomState(5)
    big = torch.from_numpy(rng.rand(6, 90, 140) < 0.55).to(_dev())
    view = big[::2, 3:80, 5:120:2]
    assert not view.is_contiguous()
    _check(view.cpu().numpy(), tensor=view)
    t = big.permute(0, 2, 1)[:2]
    _check(t.cpu().numpy(), tensor=t)


def test_forty_masks_equal_each_mask_alone_and_two_calls_agree():
    from irn_amd import ops
    masks = _blobs(40, 60, 83, seed=11)
    masks[7] = False
    masks[9] = True
    masks[11] = P.serpentine(60, 83)
    batch = _check(masks)
    xy, loop_offsets, mask_loops, holes = batch
    _same(ops.mask_polygons(torch.from_numpy(masks).to(_dev())), batch, "second call")
    for i in range(len(masks)):
        x1, o1, m1, h1 = ops.mask_polygons(torch.from_numpy(masks[i:i + 1]).to(_dev()))
        a, b = mask_loops[i], mask_loops[i + 1]
        assert m1.tolist() == [0, b - a] and h1[0] == holes[i], i
        assert np.array_equal(o1, loop_offsets[a:b + 1] - loop_offsets[a]), i
        assert np.array_equal(x1, xy[loop_offsets[a]:loop_offsets[b]]), i
    assert np.array_equal(xy, P.mask_polygons(masks)[0])   # an earlier result stays valid after later calls


def test_fill_of_the_gpu_polygons_is_the_hole_filled_mask():
    from irn_amd import ops
    masks = _blobs(3, 97, 131, seed=2)
    masks[1, 20:60, 30:90] = True
    masks[1, 30:50, 40:80] = False                         # a hole, with whatever the blob leaves in it
    xy, loop_offsets, mask_loops, holes = _check(masks)
    assert holes[1] >= 1
    for i, m in enumerate(masks):
        a, b = mask_loops[i], mask_loops[i + 1]
        own = loop_offsets[a:b + 1] - loop_offsets[a]
        filled = ops.polygon_fill(xy[loop_offsets[a]:loop_offsets[b]], own, 97, 131)
        assert np.array_equal(filled, P.fill_holes(m)), i


def test_no_masks():
    from irn_amd import ops
    xy, loop_offsets, mask_loops, holes = ops.mask_polygons(torch.zeros((0, 20, 30), dtype=torch.uint8, device=_dev()))
    assert xy.shape == (0, 2) and loop_offsets.tolist() == [0] and mask_loops.tolist() == [0] and holes.shape == (0,)
    _check(np.zeros((0, 20, 30), bool))
    _check(np.zeros((3, 20, 30), bool))                    # masks, and no edge


def test_cpu_tensor_and_wrong_dtype_are_refused():
    from irn_amd import ops
    with pytest.raises(ValueError):
        ops.mask_polygons(torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.mask_polygons(torch.zeros((1, 4, 4), dtype=torch.float32, device=_dev()))
    with pytest.raises(ValueError):
        ops.mask_polygons(torch.zeros((4, 4), dtype=torch.uint8, device=_dev()))


def test_pycocotools_rasterises_the_polygons_as_polygon_fill_does():
    mask_util = pytest.importorskip("pycocotools.mask")
    from irn_amd import ops
    masks = _blobs(3, 97, 131, seed=2)
    xy, loop_offsets, mask_loops, _ = ops.mask_polygons(torch.from_numpy(masks).to(_dev()))
    for i in range(len(masks)):
        a, b = mask_loops[i], mask_loops[i + 1]
        if a == b:
            continue
        polys = [xy[loop_offsets[k]:loop_offsets[k + 1]].reshape(-1).astype(float).tolist() for k in range(a, b)]
        got = mask_util.decode(mask_util.merge(mask_util.frPyObjects(polys, 97, 131))).astype(bool)
        own = loop_offsets[a:b + 1] - loop_offsets[a]
        assert np.array_equal(got, ops.polygon_fill(xy[loop_offsets[a]:loop_offsets[b]], own, 97, 131)), i
