"""Image-level labels of a VOC-layout tree with its own class list — counterpart of reference voc12/make_cls_labels.py.

    python -m irn_amd.voc12.make_cls_labels --voc12_root R --class_names FILE --out cls_labels.npy [--img_list LIST]

Reads  R/Annotations/<id>.xml for every id of LIST (one '2007_000032'-style id per line; without --img_list: every .xml of
       the folder, in sorted order), FILE (one class name per line: class c is line c, 0-based)
Writes --out: {int id: float32[C]} (the id without its underscore, as voc12/dataloader.py reads it), 1.0 where an object of
       the class is annotated — the file `--num_classes C` expects beside the image lists.

An object whose name is not in the class list is an error that names the image and the object: a label file that silently
dropped a class would train a classifier that never sees it.  Standard-library XML only.
"""
import argparse
import os
import xml.etree.ElementTree as ET

import numpy as np


def read_names(path):
    with open(path) as f:
        names = [ln.strip() for ln in f if ln.strip()]
    if not 1 <= len(names) <= 80:
        raise ValueError("%s: %d class names (1..80)" % (path, len(names)))
    if len(set(names)) != len(names):
        raise ValueError("%s: a class name occurs twice" % path)
    return names


def image_label(xml_path, index, img_id):
    """float32 [C] of one annotation file; `index`: class name -> 0-based class."""
    label = np.zeros(len(index), np.float32)
    try:
        root = ET.parse(xml_path).getroot()
    except ET.ParseError as e:
        raise ValueError("%s: %s" % (xml_path, e)) from e
    for obj in root.iter("object"):
        name = (obj.findtext("name") or "").strip()
        if name not in index:
            raise ValueError("%s: object %r is not in the class list" % (img_id, name))
        label[index[name]] = 1.0
    return label


def make(voc12_root, names, ids=None):
    """{int id: float32[C]} for `ids` (default: every annotation file of the tree)."""
    ann_dir = os.path.join(voc12_root, "Annotations")
    if ids is None:
        ids = sorted(f[:-4] for f in os.listdir(ann_dir) if f.endswith(".xml"))
    index = {n: i for i, n in enumerate(names)}
    out = {}
    for img_id in ids:
        path = os.path.join(ann_dir, img_id + ".xml")
        if not os.path.exists(path):
            raise FileNotFoundError("%s: no annotation file %s" % (img_id, path))
        out[int(img_id.replace("_", ""))] = image_label(path, index, img_id)
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--voc12_root", required=True, type=str)
    p.add_argument("--class_names", required=True, type=str, help="one class name per line, in class order")
    p.add_argument("--out", default="cls_labels.npy", type=str)
    p.add_argument("--img_list", default=None, type=str, help="ids to label, one per line (default: every Annotations/*.xml)")
    args = p.parse_args(argv)
    names = read_names(args.class_names)
    ids = None
    if args.img_list:
        with open(args.img_list) as f:
            ids = [ln.strip() for ln in f if ln.strip()]
    labels = make(args.voc12_root, names, ids)
    np.save(args.out, labels)
    print("make_cls_labels: %d images, %d classes -> %s" % (len(labels), len(names), args.out))
    return labels


if __name__ == "__main__":
    main()
