"""COCO export of the instance pseudo-labels — counterpart of reference step/make_cocoann.py (`run(args)`).

Reads  args.infer_list (image names, in list order), args.voc12_root/JPEGImages/<name>.jpg (header only: the size),
       args.ins_seg_out_dir/<name>.npy ({'score', 'mask', 'class'} of make_ins_seg_labels)
Writes args.cocoann_out: {"images", "annotations", "categories", "type": "instances"}, what a Mask R-CNN trainer reads.
Prints and returns {"images", "annotations", "skipped_low_score", "without_detections"}.

Per image the kept masks go to the device once and come back as run lengths, areas and boxes (`ops.mask_rle`,
irn_amd/csrc/cocomask.hip); COCO's string form of the run lengths is made on the host.  A detection with score < 1e-5 is
skipped before the upload (step/make_cocoann.py:39).  make_ins_seg_labels writes no file for an image without
detections: such an image keeps its image entry, gets no annotation, and is counted.  A mask whose shape is not the
JPEG's (height, width) is an error that names the image.

Image entries carry id, file_name, width and height.  pycococreatortools also writes date_captured (the wall clock),
license, coco_url and flickr_url; they are left out so that the same inputs always give the same file.

Three deliberate differences from the reference:

1. RLE instead of polygons.  The reference asks pycococreatortools for polygons (tolerance 0, skimage find_contours).
   Compressed RLE is exact where polygons are not, and every COCO reader accepts it in "segmentation" (annToRLE passes a
   dict with a str "counts" through).  Polygons are out of scope.
2. Annotation ids are unique over the file (1, 2, 3, ... in output order).  The reference restarts at 1 for every image
   (:36), and COCO readers index annotations by id.
3. Categories are generated (the 20 VOC classes, id 1..20 in class order, supercategory "none"), not copied from
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
from . import _eval

CATEGORIES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
              "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
MIN_SCORE = 1e-5                      # step/make_cocoann.py:39


def categories():
    return [{"supercategory": "none", "id": i + 1, "name": name} for i, name in enumerate(CATEGORIES)]


def run(args):
    names = [dataloader.decode_int_filename(v) for v in dataloader.load_img_name_list(args.infer_list)]
    dev = _eval.device()

    def load(name):
        with Image.open(dataloader.get_img_path(name, args.voc12_root)) as im:
            width, height = im.size                                   # from the header: nothing is decoded
        path = os.path.join(args.ins_seg_out_dir, name + ".npy")
        mask, cls, low = np.zeros((0, height, width), bool), np.zeros(0, np.int64), 0
        found = os.path.exists(path)
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
                if cls.min() < 0 or cls.max() >= len(CATEGORIES):
                    raise ValueError("class outside 0..%d" % (len(CATEGORIES) - 1))
                keep = ~(score < MIN_SCORE)
                low = int(len(cls) - keep.sum())
                mask, cls = m[keep], cls[keep]
        return {"mask": np.ascontiguousarray(mask), "class": cls, "size": np.int64([height, width]),
                "low": np.int64(low), "found": np.int64(found)}

    out = {"images": [], "annotations": [], "categories": categories(), "type": "instances"}
    stats = {"images": 0, "annotations": 0, "skipped_low_score": 0, "without_detections": 0}
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
            counts, offsets, area, bbox = ops.mask_rle(it["mask"].to(dev, non_blocking=True))
            for i in range(len(cls)):
                out["annotations"].append({
                    "id": len(out["annotations"]) + 1, "image_id": img_id, "category_id": int(cls[i]) + 1, "iscrowd": 0,
                    "area": int(area[i]), "bbox": [float(v) for v in bbox[i]],
                    "segmentation": {"size": [height, width], "counts": ops.rle_to_string(counts[offsets[i]:offsets[i + 1]])},
                    "width": width, "height": height})
    stats["images"], stats["annotations"] = len(out["images"]), len(out["annotations"])
    with open(args.cocoann_out, "w") as f:
        json.dump(out, f)
    print("make_cocoann:", stats)
    return stats
