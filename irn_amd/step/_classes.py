"""The dataset's class list: `--num_classes C` (foreground classes, 1..80, default 20 = VOC) and `--class_names FILE`, from
the three command lines to every step.  C + 1 (background included) is the `n_classes` of the counting operators
(irn_amd/eval_counts.py), C the width of the CAM classifier, of a `cls_labels.npy` row and of the IR labels 1..C.  An `args`
object that has no `num_classes` (older callers) means 20, so every step keeps its behaviour."""
import argparse

VOC_CLASSES = 20
MAX_CLASSES = 80                      # IRN_EVAL_MAX_CLASSES - 1: the LDS tables of the counting kernels are sized by it
VOC_NAMES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
             "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")


def _num_classes_arg(v):
    try:
        c = int(v)
    except ValueError:
        raise argparse.ArgumentTypeError("an integer in 1..%d, got %r" % (MAX_CLASSES, v))
    if not 1 <= c <= MAX_CLASSES:
        raise argparse.ArgumentTypeError("%d is outside 1..%d" % (c, MAX_CLASSES))
    return c


def add_arguments(parser):
    parser.add_argument("--num_classes", default=VOC_CLASSES, type=_num_classes_arg,
                        help="foreground classes of the dataset (not a flag of the reference, which hard-codes the 20 of VOC); "
                             "1..%d.  The CAM classifier, cls_labels.npy rows, label values 1..C and every evaluation follow it" % MAX_CLASSES)
    parser.add_argument("--class_names", default=None, type=str,
                        help="a file with one class name per line, --num_classes lines (make_cocoann's categories; unset: the VOC "
                             "names at 20 classes, class_1 .. class_C otherwise)")


def num_classes(args):
    """C of `args` (20 where it has none), checked again: not every caller comes through the parser."""
    c = getattr(args, "num_classes", None)
    c = VOC_CLASSES if c is None else int(c)
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError("num_classes %d is outside 1..%d" % (c, MAX_CLASSES))
    return c


def read_class_names(path, c):
    """The names of `path`, one per line (blank lines and surrounding white space dropped); their number must be `c`."""
    with open(path) as f:
        names = [ln.strip() for ln in f if ln.strip()]
    if len(names) != c:
        raise ValueError("%s: %d class names for --num_classes %d" % (path, len(names), c))
    if len(set(names)) != len(names):
        raise ValueError("%s: a class name occurs twice" % path)
    return names


def class_names(args):
    c = num_classes(args)
    path = getattr(args, "class_names", None)
    if path:
        return read_class_names(path, c)
    return list(VOC_NAMES) if c == VOC_CLASSES else ["class_%d" % i for i in range(1, c + 1)]
