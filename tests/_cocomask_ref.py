"""numpy / pure-Python restatement of the pycocotools mask arithmetic (common/maskApi.c: rleEncode, rleArea, rleToBbox,
rleToString, rleFrString, rleDecode) and of the JSON that irn_amd/step/make_cocoann.py writes, from the published
algorithm.  Test infrastructure: pycocotools itself is not a dependency, so the tests compare against this restatement
(tests/test_cocoann_cpu.py compares the restatement with the library wherever the library is installed).  Plain loops,
one count at a time, as maskApi.c has them; nothing here is shared with irn_amd/cocomask.py.
"""
import json
import os

import numpy as np

CATEGORIES = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
              "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]


def encode(mask):
    """rleEncode: run lengths of a [h,w] mask (nonzero = 1) in column-major order, starting with a run of zeros."""
    m = (np.asarray(mask) != 0)
    flat = m.T.reshape(-1)                                  # j = x*h + y
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1 if flat.size else np.zeros(0, np.int64)
    # the loop of rleEncode (`encode_loop` below), jumping from change to change
    counts, pos = [], 0
    if flat.size and flat[0]:
        counts.append(0)
    for j in change:
        counts.append(int(j) - pos)
        pos = int(j)
    counts.append(flat.size - pos)
    return np.asarray(counts, np.uint32)


def encode_loop(mask):
    """rleEncode pixel by pixel, exactly as maskApi.c writes it (slow: small masks only)."""
    flat = (np.asarray(mask) != 0).T.reshape(-1)
    counts, c, p = [], 0, False
    for v in flat:
        if bool(v) != p:
            counts.append(c)
            c = 0
            p = bool(v)
        c += 1
    counts.append(c)
    return np.asarray(counts, np.uint32)


def area(counts):
    """rleArea: the sum of the odd-indexed counts."""
    return int(np.asarray(counts, np.int64)[1::2].sum())


def to_bbox(counts, h, w):
    """rleToBbox: [x0, y0, width, height] from the counts alone."""
    cnts = [int(v) for v in counts]
    m = (len(cnts) // 2) * 2
    if m == 0:
        return [0, 0, 0, 0]
    xs, ys, xe, ye, cc, xp = w, h, 0, 0, 0, 0
    for j in range(m):
        cc += cnts[j]
        t = cc - j % 2
        y = t % h
        x = (t - y) // h
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys, ye = 0, h - 1
        xs, xe, ys, ye = min(xs, x), max(xe, x), min(ys, y), max(ye, y)
    return [xs, ys, xe - xs + 1, ye - ys + 1]


def tight_bbox(mask):
    ys, xs = np.nonzero(np.asarray(mask))
    if len(ys) == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def to_string(counts):
    """rleToString (LEB128-like: 5 bits per character, bit 5 = more follow, count i > 2 as a difference to count i-2)."""
    cnts = [int(v) for v in counts]
    s = []
    for i, x in enumerate(cnts):
        if i > 2:
            x -= cnts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                         # Python's >> on a negative int is arithmetic, like C's on a long
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            s.append(chr(c + 48))
    return "".join(s)


def from_string(s):
    """rleFrString."""
    b = s.encode("ascii") if isinstance(s, str) else bytes(s)
    cnts, p = [], 0
    while p < len(b):
        x, k, more = 0, 0, True
        while more:
            c = b[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[len(cnts) - 2]
        cnts.append(x)
    return np.asarray(cnts, np.uint32)


def decode(counts, h, w):
    """rleDecode: the [h,w] bool mask."""
    flat = np.zeros(h * w, bool)
    pos, v = 0, False
    for c in counts:
        c = int(c)
        flat[pos:pos + c] = v
        pos += c
        v = not v
    assert pos == h * w, "the counts sum to %d, the mask has %d pixels" % (pos, h * w)
    return np.ascontiguousarray(flat.reshape(w, h).T)


def mask_rle(masks):
    """What irn_amd.ops.mask_rle returns, from the restatement: (counts, offsets, area, bbox)."""
    masks = np.asarray(masks)
    n, h, w = masks.shape
    per = [encode(m) for m in masks]
    offsets = np.zeros(n + 1, np.int64)
    if n:
        offsets[1:] = np.cumsum([len(c) for c in per])
    counts = np.concatenate(per).astype(np.uint32) if n else np.zeros(0, np.uint32)
    areas = np.asarray([area(c) for c in per], np.int64).reshape(n)
    boxes = np.asarray([to_bbox(c, h, w) for c in per], np.int32).reshape(n, 4)
    return counts, offsets, areas, boxes


def cocoann(names, voc12_root, ins_seg_dir, min_score=1e-5):
    """The dict irn_amd/step/make_cocoann.py dumps, and the dict it returns."""
    from PIL import Image
    out = {"images": [], "annotations": [],
           "categories": [{"supercategory": "none", "id": i + 1, "name": n} for i, n in enumerate(CATEGORIES)],
           "type": "instances"}
    low = without = 0
    for name in names:
        img_id = int(name[:4] + name[5:])
        width, height = Image.open(os.path.join(voc12_root, "JPEGImages", name + ".jpg")).size
        out["images"].append({"id": img_id, "file_name": name + ".jpg", "width": width, "height": height})
        path = os.path.join(ins_seg_dir, name + ".npy")
        if not os.path.exists(path):
            without += 1
            continue
        det = np.load(path, allow_pickle=True).item()
        if len(det["class"]) == 0:
            without += 1
        for score, mask, cls in zip(det["score"], det["mask"], det["class"]):
            if score < min_score:
                low += 1
                continue
            c = encode(mask)
            out["annotations"].append({
                "id": len(out["annotations"]) + 1, "image_id": img_id, "category_id": int(cls) + 1, "iscrowd": 0,
                "area": area(c), "bbox": [float(v) for v in to_bbox(c, height, width)],
                "segmentation": {"size": [height, width], "counts": to_string(c)}, "width": width, "height": height})
    stats = {"images": len(out["images"]), "annotations": len(out["annotations"]), "skipped_low_score": low,
             "without_detections": without}
    return json.loads(json.dumps(out)), stats
