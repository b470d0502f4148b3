"""Shared plumbing of the evaluation steps (eval_cam, eval_sem_seg, eval_ins_seg).

They run in the calling process on its current device: loader threads (`_io.make_loader`) read and decode the
prediction files and the ground truth, the counting kernels add every image into int64 accumulators that stay on the
device, and the accumulators come back once at the end.  The worker pool is not used: it has no channel to send results
back, and one process makes the counts independent of `--worker_devices` by construction."""
import numpy as np
import torch

from . import _io


class EvalDataset(torch.utils.data.Dataset):
    """Item i = load(ids[i]) (a dict of numpy arrays), in split order; errors name the id."""

    def __init__(self, ids, load):
        self.ids, self.load = list(ids), load

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, idx):
        id = self.ids[idx]
        try:
            item = self.load(id)
        except (OSError, ValueError, KeyError) as e:
            raise type(e)("%s: %s" % (id, e)) from e
        item["name"] = id
        return item


def device():
    if not torch.cuda.is_available():
        raise RuntimeError("irn_amd evaluation steps need a GPU (torch.cuda.is_available() is False)")
    return torch.device("cuda", torch.cuda.current_device())


def items(ids, load, args):
    """(id, item) in split order, decoded by loader threads; tensors without the collated batch dimension."""
    loader = _io.make_loader(EvalDataset(ids, load), int(getattr(args, "num_workers", 0) or 0))
    for pack in loader:
        pack.pop("_staging", None)
        yield pack["name"][0], {k: v[0] for k, v in pack.items() if k != "name"}


def check_shape(id, what, shape, gt_shape):
    if tuple(shape) != tuple(gt_shape):
        raise ValueError("%s: %s %s does not match the ground truth %s" % (id, what, tuple(shape), tuple(gt_shape)))


def boundary_ratio(args):
    """--boundary_iou_ratio as a float: 0 (also when the namespace has no such flag) = off; negative or nan is refused."""
    r = float(getattr(args, "boundary_iou_ratio", 0) or 0)
    if not r >= 0:
        raise ValueError("--boundary_iou_ratio %s: a ratio of the image diagonal, 0 (off) or above" % r)
    return r


def boundary_d(id, shape, ratio):
    """The band width of image `id` at `ratio`, or a ValueError naming both when it is beyond what the kernels take."""
    from .. import ops
    d = ops.boundary_distance(shape[0], shape[1], ratio)
    if d > ops.BAND_MAX_D:
        raise ValueError("%s: --boundary_iou_ratio %s gives a band of %d pixels on %dx%d (at most %d)"
                         % (id, ratio, d, shape[0], shape[1], ops.BAND_MAX_D))
    return d


def raise_if_bad(bad, what, n_fg=20):
    """`n_fg`: the foreground classes the counts were taken with (`_classes.num_classes(args)`)."""
    n = int(bad.item())
    if n:
        raise ValueError("%s: %d value(s) out of range (GT outside 0..%d and 255, a NaN CAM, a class key outside 0..%d, "
                         "a prediction above %d or an instance id above the count)" % (what, n, n_fg, n_fg - 1, n_fg))
