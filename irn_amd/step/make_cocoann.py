"""COCO export of the instance pseudo-labels — counterpart of reference step/make_cocoann.py (`run(args)`).

Reads  args.infer_list (image names, in list order), args.voc12_root/JPEGImages/<name>.jpg (header only: the size),
       args.ins_seg_out_dir/<name>.npy ({'score', 'mask', 'class'} of make_ins_seg_labels), or — when that file does not
       exist — <name>.rle.npz (its --ins_seg_format rle: the masks as run lengths, with area and bbox)
Writes args.cocoann_out: {"images", "annotations", "categories", "type": "instances"}, what a Mask R-CNN trainer reads.
Prints and returns {"images", "annotations", "skipped_low_score", "without_detections"}; with --cocoann_segmentation
polygon also {"masks_with_holes", "holes"}.

Per image the kept masks go to the device once and come back as run lengths, areas and boxes (`ops.mask_rle`,
irn_amd/csrc/cocomask.hip); COCO's string form of the run lengths is made on the host.  A detection with score < 1e-5 is
skipped before the upload (step/make_cocoann.py:39).  make_ins_seg_labels writes no file for an image without
detections: such an image keeps its image entry, gets no annotation, and is counted.  A mask whose shape is not the
JPEG's (height, width) is an error that names the image.  An .rle.npz record already holds what the annotations need:
`rle_record_annotations` builds them on the host, with no upload and no kernel.

Image entries carry id, file_name, width and height.  pycococreatortools also writes date_captured (the wall clock),
license, coco_url and flickr_url; they are left out so that the same inputs always give the same file.

Three deliberate differences from the reference:

1. RLE by default, polygons on request.  The reference asks pycococreatortools for polygons (tolerance 0, skimage
   find_contours).  Compressed RLE is exact and is what --cocoann_segmentation rle (the default) writes.  With
   --cocoann_segmentation polygon "segmentation" is a list of polygons [[x0, y0, x1, y1, ...], ...] for the readers that
   take nothing else (the Mask R-CNN code the IRN paper trained with).  They are defined exactly: the boundary of the
   mask along pixel edges, vertex (x, y) = the top-left corner of pixel (x, y) (the coordinates of "bbox"), the mask on the
   right of every edge, right turn before straight on before left turn, so that the loops follow the 4-connectivity of
   make_ins_seg_labels' components; one polygon per outer loop, its corners only, from its smallest vertex in (y, x)
   order, loops in the (y, x) order of those vertices (`ops.mask_polygons`, traced on the GPU).  Filling the loops gives
   the mask back bit for bit, which is what the tests hold the kernels to.  They are not skimage's contours, because those
   run through the midpoints of pixel edges in an order only skimage defines: nothing could be compared with them here.
   Holes are counted ("masks_with_holes", "holes"), not written: a COCO reader takes the union of a segmentation's
   polygons, so a hole loop could cut nothing out, and the polygons of a mask with holes describe it with the holes
   filled, as the reference's do once a reader unions them.  "area" and "bbox" stay the true mask's.  An .rle.npz
   record is decoded on the host and traced by the same kernels, so both input formats give the same bytes.
2. Annotation ids are unique over the file (1, 2, 3, ... in output order).  The reference restarts at 1 for every image
   (:36), and COCO readers index annotations by id.
3. Categories are generated (the 20 VOC classes, id 1..20 in class order, supercategory "none"; with --num_classes C the
   names of --class_names, or class_1 .. class_C, id 1..C), not copied from
   pascal_val2012.json (:16, a file the reference does not ship), and category_id = class + 1 so that it points into
   them; the reference passes the 0-based class through.
"""
import json
import os

import numpy as np
import torch
from PIL import Image

from .. import ops
from ..voc12 import dataloader
from . import _classes, _eval

CATEGORIES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
              "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
MIN_SCORE = 1e-5                      # step/make_cocoann.py:39


def categories(names=CATEGORIES):
    return [{"supercategory": "none", "id": i + 1, "name": name} for i, name in enumerate(names)]


def annotation(ann_id, img_id, cls, area, bbox, height, width, counts, polygons=None):
    """`polygons`: the mask's outer loops as [[x0, y0, x1, y1, ...], ...] to write instead of the run lengths."""
    seg = {"size": [height, width], "counts": ops.rle_to_string(counts)} if polygons is None else polygons
    return {"id": ann_id, "image_id": img_id, "category_id": int(cls) + 1, "iscrowd": 0, "area": int(area),
            "bbox": [float(v) for v in bbox], "segmentation": seg, "width": width, "height": height}


def polygon_lists(xy, loop_offsets, mask_loops):
    """`ops.mask_polygons`' arrays as per mask a list of [x0, y0, x1, y1, ...] lists of Python ints."""
    flat = np.asarray(xy).reshape(-1).tolist()
    off = [2 * int(v) for v in loop_offsets]
    return [[flat[off[k]:off[k + 1]] for k in range(int(a), int(b))] for a, b in zip(mask_loops[:-1], mask_loops[1:])]


def rle_record_kept(rec, height, width, name=None, n_classes=len(CATEGORIES)):
    """One <name>.rle.npz record (a mapping with the arrays `ops.detect_instance_rle_batch` returns), checked against a
    JPEG of height x width.  -> {"class" int64 [K], "counts" int64 [total], "offsets" int64 [K+1], "area" int64 [K], "bbox"
    int32 [K,4]} of the K detections that stay (score >= MIN_SCORE), "low" (the number dropped) and "n" (all of them).
    Needs no device.  Errors name the image when `name` is given; `n_classes`: the dataset's foreground classes."""
    cls, score = np.asarray(rec["class"]).reshape(-1).astype(np.int64), np.asarray(rec["score"]).reshape(-1)
    counts, offsets = np.asarray(rec["counts"]).reshape(-1).astype(np.int64), np.asarray(rec["offsets"]).reshape(-1).astype(np.int64)
    area, bbox = np.asarray(rec["area"]).reshape(-1).astype(np.int64), np.asarray(rec["bbox"]).reshape(-1, 4).astype(np.int32)
    size = tuple(int(v) for v in np.asarray(rec["size"]).reshape(-1))
    n = len(cls)
    who = "%s: " % name if name else ""
    if not (len(score) == n and len(offsets) == n + 1 and len(area) == n and len(bbox) == n):
        raise ValueError("%s%d classes, %d scores, %d offsets, %d areas, %d boxes" % (who, n, len(score), len(offsets),
                                                                                       len(area), len(bbox)))
    if size != (height, width):
        raise ValueError("%srun lengths of size %s do not match the %dx%d (height x width) JPEG" % (who, size, height, width))
    if offsets[0] != 0 or (np.diff(offsets) < 1).any() or offsets[n] != len(counts):
        raise ValueError("%soffsets do not partition the %d run lengths" % (who, len(counts)))
    if n and (cls.min() < 0 or cls.max() >= n_classes):
        raise ValueError("%sclass outside 0..%d" % (who, n_classes - 1))
    keep = np.flatnonzero(~(score < MIN_SCORE))
    parts = [counts[offsets[i]:offsets[i + 1]] for i in keep]
    for i, c in zip(keep, parts):
        if int(c.sum()) != height * width:
            raise ValueError("%sthe run lengths of detection %d sum to %d, the image has %d pixels"
                             % (who, i, int(c.sum()), height * width))
    kept_offsets = np.zeros(len(keep) + 1, np.int64)
    np.cumsum([len(c) for c in parts], out=kept_offsets[1:])
    return {"class": cls[keep], "counts": np.concatenate(parts) if parts else np.zeros(0, np.int64), "offsets": kept_offsets,
            "area": area[keep], "bbox": bbox[keep], "low": n - len(keep), "n": n}


def annotations(kept, img_id, height, width, first_id, polygons=None):
    """The annotation dicts of one image from per-detection class, area, bbox and run lengths (counts / offsets) — from the
    device's encoder for dense masks, from `rle_record_kept` for a stored record.  `polygons`: (xy, loop_offsets,
    mask_loops) of `ops.mask_polygons` for the same detections, written as the segmentations instead of the run lengths."""
    cls, counts, offsets = kept["class"], kept["counts"], kept["offsets"]
    if polygons is not None:
        lists = polygon_lists(*polygons)
        return [annotation(first_id + i, img_id, cls[i], kept["area"][i], kept["bbox"][i], height, width, None, lists[i])
                for i in range(len(cls))]
    return [annotation(first_id + i, img_id, cls[i], kept["area"][i], kept["bbox"][i], height, width,
                       counts[offsets[i]:offsets[i + 1]]) for i in range(len(cls))]


def rle_record_annotations(rec, img_id, height, width, first_id, name=None):
    """The annotations of one <name>.rle.npz record for a JPEG of height x width: exactly what the dense masks of the same
    detections give.  Needs no device.  -> (annotations with ids first_id, first_id + 1, ..., number of detections dropped)."""
    kept = rle_record_kept(rec, height, width, name)
    return annotations(kept, img_id, height, width, first_id), kept["low"]


def run(args):
    names = [dataloader.decode_int_filename(v) for v in dataloader.load_img_name_list(args.infer_list)]
    dev = _eval.device()
    class_names = _classes.class_names(args)          # refusals (a missing file, a wrong line count) before any image is read
    c = len(class_names)
    polygon = getattr(args, "cocoann_segmentation", "rle") == "polygon"

    def load(name):
        with Image.open(dataloader.get_img_path(name, args.voc12_root)) as im:
            width, height = im.size                                   # from the header: nothing is decoded
        path = os.path.join(args.ins_seg_out_dir, name + ".npy")
        mask, cls, low = np.zeros((0, height, width), bool), np.zeros(0, np.int64), 0
        found = os.path.exists(path)
        rle_path = os.path.join(args.ins_seg_out_dir, name + ".rle.npz")
        if not found and os.path.exists(rle_path):
            with np.load(rle_path, allow_pickle=False) as z:
                kept = rle_record_kept(z, height, width, n_classes=c)               # (the loader names the image of an error)
            rec = {"rle": np.int64(1), "class": kept["class"], "counts": kept["counts"], "offsets": kept["offsets"],
                   "area": kept["area"], "bbox": kept["bbox"], "size": np.int64([height, width]),
                   "low": np.int64(kept["low"]), "found": np.int64(kept["n"] > 0)}
            if polygon:                   # the tracer takes dense masks: decoded here, in the loader thread
                off = kept["offsets"]
                rec["mask"] = np.stack([ops.rle_decode(kept["counts"][off[i]:off[i + 1]], height, width)
                                        for i in range(len(kept["class"]))]) if len(kept["class"]) else np.zeros((0, height, width), bool)
            return rec
        if found:
            det = np.load(path, allow_pickle=True).item()
            cls, score = np.asarray(det["class"]).reshape(-1).astype(np.int64), np.asarray(det["score"]).reshape(-1)
            m = np.asarray(det["mask"])
            if len(score) != len(cls):
                raise ValueError("%d scores for %d classes" % (len(score), len(cls)))
            found = len(cls) > 0
            if found:
                if m.shape != (len(cls), height, width):
                    raise ValueError("masks %s do not match the %d detections of a %dx%d (height x width) JPEG"
                                     % (m.shape, len(cls), height, width))
                if cls.min() < 0 or cls.max() >= c:
                    raise ValueError("class outside 0..%d" % (c - 1))
                keep = ~(score < MIN_SCORE)
                low = int(len(cls) - keep.sum())
                mask, cls = m[keep], cls[keep]
        return {"mask": np.ascontiguousarray(mask), "class": cls, "size": np.int64([height, width]),
                "low": np.int64(low), "found": np.int64(found), "rle": np.int64(0)}

    out = {"images": [], "annotations": [], "categories": categories(class_names), "type": "instances"}
    stats = {"images": 0, "annotations": 0, "skipped_low_score": 0, "without_detections": 0}
    if polygon:
        stats.update(masks_with_holes=0, holes=0)
    with torch.cuda.device(dev):
        for name, it in _eval.items(names, load, args):
            img_id = int(name[:4] + name[5:])
            height, width = (int(v) for v in it["size"])
            out["images"].append({"id": img_id, "file_name": name + ".jpg", "width": width, "height": height})
            stats["skipped_low_score"] += int(it["low"])
            cls = it["class"].numpy()
            if not int(it["found"]):
                stats["without_detections"] += 1
            if len(cls) == 0:
                continue
            masks = it["mask"].to(dev, non_blocking=True) if polygon or not int(it["rle"]) else None
            if int(it["rle"]):          # an .rle.npz record holds what the encoder would compute: no upload, no kernel
                kept = {k: it[k].numpy() for k in ("class", "counts", "offsets", "area", "bbox")}
            else:
                counts, offsets, area, bbox = ops.mask_rle(masks)
                kept = {"class": cls, "counts": counts, "offsets": offsets, "area": area, "bbox": bbox}
            polygons = None
            if polygon:
                xy, loop_offsets, mask_loops, holes = ops.mask_polygons(masks)
                polygons = (xy, loop_offsets, mask_loops)
                stats["masks_with_holes"] += int((holes > 0).sum())
                stats["holes"] += int(holes.sum())
            out["annotations"] += annotations(kept, img_id, height, width, len(out["annotations"]) + 1, polygons)
    stats["images"], stats["annotations"] = len(out["images"]), len(out["annotations"])
    with open(args.cocoann_out, "w") as f:
        json.dump(out, f)
    print("make_cocoann:", stats)
    return stats
