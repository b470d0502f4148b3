"""make_cocoann with --cocoann_segmentation polygon, through run_sample.py on a small synthetic tree: from <name>.npy and from
<name>.rle.npz inputs, against the rle-mode file of the same tree, and the rle mode against the run without the flag."""
import json
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cocomask_ref as R  # noqa: E402
import _polygon_ref as P  # noqa: E402
import _steps as S  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = ((40, 56), (33, 47))


def _make_tree(tmp, n=5):
    """JPEGs of two sizes with their detections twice: <name>.npy under ins_npy, <name>.rle.npz under ins_rle.  Image 1 has
    a ring with a hole and a component inside it; image 2 has no file; every other image has two or three detections, one
    of image 0's below the score threshold."""
    from irn_amd.step import make_ins_seg_labels
    root = tmp / "voc"
    (root / "JPEGImages").mkdir(parents=True)
    (tmp / "ins_npy").mkdir()
    (tmp / "ins_rle").mkdir()
    rng = np.random.RandomState(0)
    names, stored = [], {}
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        h, w = SIZES[i % 2]
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8)
        Image.fromarray(img).resize((w, h), Image.BICUBIC).save(root / "JPEGImages" / (name + ".jpg"), quality=90)
        names.append(name)
        if i == 2:
            continue
        k = 2 + i % 2
        coarse = rng.rand(k, (h + 3) // 4, (w + 3) // 4) < 0.45
        masks = coarse.repeat(4, 1).repeat(4, 2)[:, :h, :w] ^ (rng.rand(k, h, w) < 0.01)
        if i == 1:
            masks[0] = False
            masks[0, 4:28, 6:40] = True
            masks[0, 9:23, 12:34] = False
            masks[0, 13:18, 18:27] = True
        score = rng.uniform(0.1, 1.0, k).astype(np.float32)
        if i == 0:
            score[1] = 1e-6
        cls = rng.randint(0, 20, k).astype(np.int64)
        np.save(tmp / "ins_npy" / (name + ".npy"), {"score": score, "mask": masks, "class": cls})
        counts, offsets, area, bbox = R.mask_rle(masks)
        make_ins_seg_labels.save_rle(str(tmp / "ins_rle" / (name + ".rle.npz")),
                                     {"score": score, "class": cls, "size": (h, w), "counts": counts, "offsets": offsets,
                                      "area": area, "bbox": bbox})
        stored[name] = (score, masks, cls)
    (tmp / "train.txt").write_text("\n".join(names) + "\n")
    return root, names, stored


def _run(tmp, root, ins, out, extra):
    return S.run_sample_main(["--voc12_root", str(root), "--infer_list", str(tmp / "train.txt"), "--num_workers", "2",
                              "--cam_out_dir", str(tmp / "cam"), "--sem_seg_out_dir", str(tmp / "sem"),
                              "--ins_seg_out_dir", str(tmp / ins), "--log_name", str(tmp / "log"),
                              "--make_cam_pass", "False", "--make_ins_seg_pass", "False", "--make_sem_seg_pass", "False",
                              "--make_cocoann_pass", "True", "--cocoann_out", str(tmp / out)] + extra)


def test_polygon_mode_from_both_input_formats_against_the_rle_mode(tmp_path):
    from irn_amd import ops
    root, names, stored = _make_tree(tmp_path)
    plain = _run(tmp_path, root, "ins_npy", "plain.json", [])
    rle = _run(tmp_path, root, "ins_npy", "rle.json", ["--cocoann_segmentation", "rle"])
    poly = _run(tmp_path, root, "ins_npy", "poly_npy.json", ["--cocoann_segmentation", "polygon"])
    poly_rle = _run(tmp_path, root, "ins_rle", "poly_rle.json", ["--cocoann_segmentation", "polygon"])
    # the rle mode is the run without the flag, byte for byte, and what the restatement of the step gives
    assert (tmp_path / "rle.json").read_bytes() == (tmp_path / "plain.json").read_bytes()
    want, want_stats = R.cocoann(names, str(root), str(tmp_path / "ins_npy"))
    assert plain == rle == {"make_cocoann": want_stats} and json.load(open(tmp_path / "rle.json")) == want
    # both input formats end in the same bytes
    assert (tmp_path / "poly_npy.json").read_bytes() == (tmp_path / "poly_rle.json").read_bytes()
    assert poly == poly_rle
    stats = poly["make_cocoann"]
    assert {k: v for k, v in stats.items() if k not in ("masks_with_holes", "holes")} == want_stats
    got = json.load(open(tmp_path / "poly_npy.json"))
    assert got["images"] == want["images"] and got["categories"] == want["categories"] and got["type"] == want["type"]
    assert len(got["annotations"]) == len(want["annotations"]) > 0
    with_holes = holes = 0
    for a, b in zip(got["annotations"], want["annotations"]):
        assert {k: v for k, v in a.items() if k != "segmentation"} == {k: v for k, v in b.items() if k != "segmentation"}
        h, w = b["segmentation"]["size"]
        mask = ops.rle_decode(ops.rle_from_string(b["segmentation"]["counts"]), h, w)
        seg = a["segmentation"]
        assert isinstance(seg, list) and seg and all(isinstance(v, int) for loop in seg for v in loop)
        xy = np.asarray([v for loop in seg for v in loop], np.int32).reshape(-1, 2)
        offsets = np.cumsum([0] + [len(loop) // 2 for loop in seg])
        assert np.array_equal(ops.polygon_fill(xy, offsets, h, w), P.fill_holes(mask))
        n_holes = P.enclosed_background(mask)[0]
        with_holes += n_holes > 0
        holes += n_holes
    assert stats["masks_with_holes"] == with_holes >= 1 and stats["holes"] == holes
    per_image = {}
    for a in got["annotations"]:
        per_image[a["image_id"]] = per_image.get(a["image_id"], 0) + 1
    assert max(per_image.values()) >= 2
    # the ring of image 1: its outer boundary and the component inside its hole
    ring = next(a for a in got["annotations"] if a["image_id"] == 2008000002)
    assert ring["segmentation"] == [[6, 4, 40, 4, 40, 28, 6, 28], [18, 13, 27, 13, 27, 18, 18, 18]]
