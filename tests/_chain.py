"""The `chain` fixture (tests/golden/chain.npz, written by tests/golden/make_golden.py --only chain): two images through the
reference's whole composition — step/make_cam.py:26-56, step/make_sem_seg_labels.py:28-51 and the instance branch of
step/make_ins_seg_labels.py — in float32, with the reference's own float32-vs-float64 distance at every stage stored next to the
values (d_cam, d_edge, d_dp, d_rw_up, d_rw_up_ins).  Shared by tests/test_chain_cpu.py and tests/test_gpu_chain.py.

The bars the chain tests hold the product to come from those distances, not from the product:
    delta = 4 * d_rw_up on the normalised upsampled scores — two independently rounded fp32-class computations, each within d of
    the exact value, are within 2 d of each other; a further factor 2 covers the split-precision trunk's 22-bit operands (its
    measured per-layer error is at most 1.5 x fp32's);
    a label may differ from the reference's only where the two best entries of the REFERENCE's score stack (background included)
    are closer than 2 * delta, and no more pixels may differ than the reference has such ties."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
IMAGES = ("a", "b")
MARGIN = 4                 # delta = MARGIN * d_rw_up
TIE_SHARE = 0.005          # the generator's condition: at most this share of the pixels are ties at 2 * delta


def load():
    return dict(np.load(os.path.join(HERE, "golden", "chain.npz")))


def size(fx, name):
    h, w, _seed = (int(v) for v in fx[name + "_seed"])
    return h, w


def photo(fx, name):
    from irn_amd import synth
    h, w, seed = (int(v) for v in fx[name + "_seed"])
    return synth.photo(h, w, seed)


def has_instances(fx, name):
    return name + "_rw_ins" in fx


def stack_gap(up, bg):
    """Top-2 gap per pixel of the score stack [background threshold, up[0], up[1], ...]."""
    stack = np.sort(np.concatenate([np.full((1,) + up.shape[1:], bg, np.float32), np.asarray(up, np.float32)], 0), 0)
    return stack[-1] - stack[-2]


def tie_count(up, bg, delta):
    return int((stack_gap(up, bg) < 2 * delta).sum())


def instance_map(fx, name):
    shape = tuple(int(v) for v in fx[name + "_instance_map_shape"])
    return np.unpackbits(fx[name + "_instance_map"])[:int(np.prod(shape))].reshape(shape).astype(bool)


def detections(fx, name):
    shape = tuple(int(v) for v in fx[name + "_det_mask_shape"])
    mask = np.unpackbits(fx[name + "_det_mask"])[:int(np.prod(shape))].reshape(shape).astype(bool)
    return {"score": fx[name + "_det_score"], "class": fx[name + "_det_class"], "mask": mask}


def paint(det):
    """The class-id map (class + 1, 0 = nothing) the detections paint; their masks are disjoint (they come from an argmax)."""
    return (np.asarray(det["mask"]).astype(np.int64) * (np.asarray(det["class"], np.int64) + 1)[:, None, None]).sum(0)
