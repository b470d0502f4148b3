"""The COCO mask encoder (irn_amd/csrc/cocomask.hip through ops.mask_rle) against the restatement of pycocotools
(tests/_cocomask_ref.py), integer for integer, and the make_cocoann step end to end on a synthetic tree.  pycocotools
itself is not a dependency; tests/test_cocoann_cpu.py compares the restatement with it wherever it is installed."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cocomask_ref as R  # noqa: E402
import _steps as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _check(masks, tensor=None):
    """ops.mask_rle(masks) == the restatement, in every integer; `tensor` = the GPU tensor to pass instead of an upload."""
    from irn_amd import ops
    masks = np.asarray(masks)
    t = torch.from_numpy(masks).to(_dev()) if tensor is None else tensor
    counts, offsets, area, bbox = ops.mask_rle(t)
    w_counts, w_offsets, w_area, w_bbox = R.mask_rle(masks)
    assert counts.dtype == np.uint32 and offsets.dtype == np.int64 and area.dtype == np.int64 and bbox.dtype == np.int32
    assert bbox.shape == (len(masks), 4) and area.shape == (len(masks),)
    assert np.array_equal(offsets, w_offsets)
    assert np.array_equal(area, w_area)
    assert np.array_equal(bbox, w_bbox)
    assert np.array_equal(counts, w_counts)
    return counts, offsets, area, bbox


def _blobs(n, h, w, seed):
    """Blob masks: irn_amd.synth.cam_blobs on a coarse grid, upsampled to the image and thresholded."""
    from irn_amd import synth
    cams = synth.cam_blobs(n, (h + 3) // 4, (w + 3) // 4, seed=seed)
    up = torch.nn.functional.interpolate(torch.from_numpy(cams)[None], size=(h, w), mode="bilinear", align_corners=False)[0]
    rng = np.random.RandomState(seed)
    return (up.numpy() > rng.uniform(0.2, 0.7, (n, 1, 1))) | (rng.rand(n, h, w) < 0.002)       # + a few stray pixels


@pytest.mark.parametrize("h,w", [(375, 500), (500, 333), (512, 512)])
def test_blob_masks(h, w):
    masks = _blobs(5, h, w, seed=h + w)
    assert masks.any() and not masks.all()
    _check(masks)


def test_empty_and_full_mask_in_one_batch():
    masks = np.zeros((4, 37, 70), bool)
    masks[1] = True
    masks[3, 5:9, 60:] = True
    counts, offsets, area, bbox = _check(masks)
    assert counts[offsets[0]:offsets[1]].tolist() == [37 * 70] and counts[offsets[1]:offsets[2]].tolist() == [0, 37 * 70]
    assert counts[offsets[2]:offsets[3]].tolist() == [37 * 70]
    assert bbox[0].tolist() == [0, 0, 0, 0] and bbox[1].tolist() == [0, 0, 70, 37] and area.tolist()[:3] == [0, 37 * 70, 0]


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (64, 64), (130, 129), (375, 500)])
def test_corner_pixels_and_column_seam(h, w):
    first = np.zeros((h, w), bool)
    first[0, 0] = True
    last = np.zeros((h, w), bool)
    last[h - 1, w - 1] = True
    both = first | last
    masks = [first, last, both]
    if w > 1:
        for x in sorted({1, w - 1, min(64, w - 1), min(65, w - 1)}):       # a run over the seam before column x
            seam = np.zeros((h, w), bool)
            seam[h - 1 - (h - 1) // 3:, x - 1] = True
            seam[:(h + 2) // 3, x] = True
            masks.append(seam)
    counts, offsets, _, _ = _check(np.stack(masks))
    assert counts[offsets[0]:offsets[1]].tolist() == ([0, 1, h * w - 1] if h * w > 1 else [0, 1])
    assert counts[offsets[1]:offsets[2]].tolist() == ([h * w - 1, 1] if h * w > 1 else [0, 1])
    if w > 1:
        assert offsets[4] - offsets[3] == 3                # zeros, ONE run of ones across the seam, zeros


@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (1, 300), (300, 1), (2, 1), (9, 3), (40, 65), (33, 333), (1000, 3), (3, 1000)])
def test_thin_and_odd_widths(h, w):
    rng = np.random.RandomState(h * 1000 + w)
    masks = np.stack([rng.rand(h, w) < p for p in (0.5, 0.05, 0.95)] + [np.zeros((h, w), bool), np.ones((h, w), bool)])
    _check(masks)


@pytest.mark.parametrize("h,w,n_board,n_comp", [(64, 64, 4033, 4034), (63, 64, 63 * 64, 63 * 64 + 1)])
def test_checkerboards(h, w, n_board, n_comp):
    yy, xx = np.mgrid[:h, :w]
    board = (yy + xx) % 2 == 1
    _, offsets, _, _ = _check(np.stack([board, ~board]))
    assert np.diff(offsets).tolist() == [n_board, n_comp]


def test_any_nonzero_value_is_in_the_mask():
    rng = np.random.RandomState(3)
    bits = rng.rand(3, 50, 77) < 0.4
    values = np.where(bits, rng.choice(np.uint8([1, 2, 255, 128]), bits.shape), 0).astype(np.uint8)
    from irn_amd import ops
    got = ops.mask_rle(torch.from_numpy(values).to(_dev()))
    want = _check(bits)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_no_masks():
    from irn_amd import ops
    counts, offsets, area, bbox = ops.mask_rle(torch.zeros((0, 20, 30), dtype=torch.uint8, device=_dev()))
    assert counts.shape == (0,) and offsets.tolist() == [0] and area.shape == (0,) and bbox.shape == (0, 4)
    _check(np.zeros((0, 20, 30), bool))


def test_forty_masks_and_batch_equals_single():
    from irn_amd import ops
    masks = _blobs(40, 120, 167, seed=11)
    masks[7] = False
    masks[9] = True
    counts, offsets, area, bbox = _check(masks)
    for i in range(len(masks)):
        c1, o1, a1, b1 = ops.mask_rle(torch.from_numpy(masks[i:i + 1]).to(_dev()))
        assert np.array_equal(c1, counts[offsets[i]:offsets[i + 1]]) and o1.tolist() == [0, len(c1)]
        assert a1[0] == area[i] and np.array_equal(b1[0], bbox[i])
    # an earlier result stays valid after later calls (the counts own their memory)
    again, _, _, _ = R.mask_rle(masks)
    assert np.array_equal(counts, again)


def test_non_contiguous_view():
    rng = np.random.RandomState(5)
    big = torch.from_numpy(rng.rand(6, 90, 140) < 0.3).to(_dev())
    view = big[::2, 3:80, 5:120:2]
    assert not view.is_contiguous()
    _check(view.cpu().numpy(), tensor=view)
    t = big.permute(0, 2, 1)                               # [N, W, H] seen as masks of 140 x 90
    _check(t.cpu().numpy(), tensor=t)


def test_decode_of_the_gpu_counts_is_the_mask():
    from irn_amd import ops
    masks = _blobs(3, 97, 131, seed=2)
    counts, offsets, _, _ = _check(masks)
    for i, m in enumerate(masks):
        c = counts[offsets[i]:offsets[i + 1]]
        assert np.array_equal(ops.rle_decode(ops.rle_from_string(ops.rle_to_string(c)), 97, 131), m)


def test_cpu_tensor_is_refused():
    from irn_amd import ops
    with pytest.raises(ValueError):
        ops.mask_rle(torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.mask_rle(torch.zeros((1, 4, 4), dtype=torch.float32, device=_dev()))


# ---------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------
SIZES = ((96, 128), (113, 150))


def _make_tree(tmp, n=7):
    """JPEGs of two sizes; ins_seg files with a low-score detection in some; image 3 has no file, image 5 an empty one."""
    root, ins = tmp / "voc", tmp / "ins"
    (root / "JPEGImages").mkdir(parents=True)
    ins.mkdir()
    rng = np.random.RandomState(0)
    names, stored = [], {}
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        h, w = SIZES[i % 2]
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8)
        Image.fromarray(img).resize((w, h), Image.BICUBIC).save(root / "JPEGImages" / (name + ".jpg"), quality=90)
        names.append(name)
        if i == 3:
            continue
        k = 0 if i == 5 else 2 + i % 3
        masks = _blobs(k, h, w, seed=100 + i) if k else np.zeros((0, h, w), bool)
        score = rng.uniform(0.1, 1.0, k).astype(np.float32)
        if k and i % 2 == 0:
            score[i % k] = 1e-6                            # below the reference's 1e-5: skipped
        cls = rng.randint(0, 20, k).astype(np.int64)
        np.save(ins / (name + ".npy"), {"score": score, "mask": masks, "class": cls})
        stored[name] = (score, masks, cls)
    (tmp / "train.txt").write_text("\n".join(names) + "\n")
    return root, ins, names, stored


def _args(tmp, root, ins, out, workers):
    return argparse.Namespace(voc12_root=str(root), infer_list=str(tmp / "train.txt"), ins_seg_out_dir=str(ins),
                              cocoann_out=str(out), num_workers=workers)


def test_step_vs_restatement(tmp_path):
    from irn_amd import ops
    from irn_amd.step import make_cocoann
    root, ins, names, stored = _make_tree(tmp_path)
    with torch.cuda.device(_dev()):
        stats = make_cocoann.run(_args(tmp_path, root, ins, tmp_path / "a.json", 0))
        stats4 = make_cocoann.run(_args(tmp_path, root, ins, tmp_path / "b.json", 4))
    want, want_stats = R.cocoann(names, str(root), str(ins))
    got = json.load(open(tmp_path / "a.json"))
    assert got == want
    assert stats == want_stats and stats4 == want_stats
    assert stats["images"] == len(names) and stats["without_detections"] == 2 and stats["skipped_low_score"] == 4
    assert (tmp_path / "a.json").read_bytes() == (tmp_path / "b.json").read_bytes()
    assert [a["id"] for a in got["annotations"]] == list(range(1, len(got["annotations"]) + 1))
    assert [im["file_name"] for im in got["images"]] == [n + ".jpg" for n in names]
    assert got["type"] == "instances" and [c["id"] for c in got["categories"]] == list(range(1, 21))
    # every segmentation decodes to the stored mask it came from
    by_image = {}
    for a in got["annotations"]:
        by_image.setdefault(a["image_id"], []).append(a)
    seen = 0
    for name, (score, masks, cls) in stored.items():
        kept = [j for j in range(len(cls)) if not score[j] < 1e-5]
        anns = by_image.get(int(name[:4] + name[5:]), [])
        assert len(anns) == len(kept)
        for a, j in zip(anns, kept):
            h, w = a["segmentation"]["size"]
            assert (h, w) == masks[j].shape == (a["height"], a["width"])
            assert isinstance(a["segmentation"]["counts"], str)
            m = ops.rle_decode(ops.rle_from_string(a["segmentation"]["counts"]), h, w)
            assert np.array_equal(m, masks[j])
            assert a["category_id"] == int(cls[j]) + 1 and a["iscrowd"] == 0 and a["area"] == int(masks[j].sum())
            assert a["bbox"] == [float(v) for v in R.tight_bbox(masks[j])]
            seen += 1
    assert seen == len(got["annotations"]) > 0


def test_step_names_the_image_of_a_mask_of_the_wrong_shape(tmp_path):
    from irn_amd.step import make_cocoann
    root, ins, names, stored = _make_tree(tmp_path, n=2)
    score, masks, cls = stored[names[1]]
    np.save(ins / (names[1] + ".npy"), {"score": score, "mask": masks[:, :-1], "class": cls})
    with pytest.raises(ValueError, match=names[1]):
        with torch.cuda.device(_dev()):
            make_cocoann.run(_args(tmp_path, root, ins, tmp_path / "c.json", 0))


def test_run_sample_writes_the_file(tmp_path):
    root, ins, names, _ = _make_tree(tmp_path)
    out = tmp_path / "coco.json"
    res = S.run_sample_main(["--voc12_root", str(root), "--infer_list", str(tmp_path / "train.txt"), "--num_workers", "2",
                             "--cam_out_dir", str(tmp_path / "cam"), "--sem_seg_out_dir", str(tmp_path / "sem"),
                             "--ins_seg_out_dir", str(ins), "--log_name", str(tmp_path / "log"),
                             "--make_cam_pass", "False", "--make_ins_seg_pass", "False", "--make_sem_seg_pass", "False",
                             "--make_cocoann_pass", "True", "--cocoann_out", str(out)])
    want, want_stats = R.cocoann(names, str(root), str(ins))
    assert res == {"make_cocoann": want_stats}
    assert json.load(open(out)) == want
