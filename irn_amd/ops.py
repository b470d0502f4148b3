"""Host-side wrappers of the kernels in libirn_hip.so outside the walk, under one name.  Every kernel file has a host module
of its own stem next to this one, and this module re-exports their functions; steps, nets and the data loader call them
as `ops.X`, looked up at call time.

    label.py        label.hip      label_epilogue, label_sweep_confusion, cam_merge
    msf.py          msf.hip        rescale_size, bicubic_plan, bicubic_resize, normalize_lut, msf_pack
    augment.py      augment.hip    augment_tables, augment_label_tables, nearest_plan, augment_batch, augment_pair_batch
    bn_act.py       bn_act.hip     bn_act_, bn_fold, bn_param_grads, bn_act, bn_act_backward, stem_pool, upsample_bilinear
    instance.py     instance.hip   find_centroids*, cluster_centroids*, label4, detect_instance*, detect_batch_count,
                                   detection_overlap_batch, argmax_rethreshold_batch, the Pending* results
    crf.py          crf.hip        crf_filter, crf_inference_label, crf_ir_label, crf_label_sweep,
                                   crf_score_sweep, crf_prob
    eval_counts.py  eval.hip       eval_thresholds, cam_confusion, cam_confusion_matrices, label_confusion, mask_overlap,
                                   ir_label_confusion, boundary_distance, label_band, label_boundary_counts,
                                   mask_boundary_overlap
    cocomask.py     cocomask.hip   mask_rle, rle_to_string, rle_from_string, rle_decode, mask_polygons, polygon_fill
    seg_loss.py     seg_loss.hip   seg_loss_sums, seg_cross_entropy, seg_argmax
                    seg_fuse.hip   seg_fuse
    gemm.py         conv1x1.cpp, split16.hip    the hipBLASLt convolutions of the trunk
    _host.py        what more than one of them needs: cached buffers, read_back, packed layouts and their staging

Reference functions mirrored (names kept where the reference has one):
    find_centroids_with_refinement(displacement, iterations=300)   step/make_ins_seg_labels.py:18-56
    cluster_centroids(centroids, displacement, thres=2.5)          step/make_ins_seg_labels.py:58-75
    label4(mask)                = skimage.measure.label(mask, connectivity=1, background=0)  (:66,:92)
    label_epilogue(...)         = step/make_sem_seg_labels.py:43-49, step/make_ins_seg_labels.py:137-145
    detect_instance(...)        = step/make_ins_seg_labels.py:82-105
    bicubic_resize(img, size)   = misc/imutils.py:8-17 pil_resize(img, size, order=3)
    msf_pack(img, scales)       = voc12/dataloader.py:191-201 (rescale, normalise, CHW, flip pair)
    augment_batch(images, ...)  = voc12/dataloader.py:129-156 for a batch (resize_long, normalise, mirror, crop, CHW)
    augment_pair_batch(images, labels, ...) = voc12/dataloader.py:251-267 for a batch (the image as above, the IR label
                                  nearest-rescaled, mirrored, cropped into 255 and reduced)
GPU tensors in, GPU tensors out; no CPU fallback.
"""
# flake8: noqa: F401
import collections                    # (the modules and binding helpers this file had when it held the code stay reachable)
import ctypes as C

import numpy as np
import torch

from ._host import read_back
from ._lib import check, i32_array, lib, ptr_array
from .augment import (AUGMENT_DESC_WORDS, AUGMENT_LABEL_DESC_WORDS, AugmentTables, LabelTables, augment_batch, augment_label_tables,
                      augment_pair_batch, augment_tables, nearest_plan)
from .bn_act import bn_act, bn_act_, bn_act_backward, bn_fold, bn_param_grads, stem_pool, upsample_bilinear
from .cocomask import mask_polygons, mask_rle, polygon_fill, rle_decode, rle_from_string, rle_to_string
from .crf import (CRF_GT_PROB, CRF_MAX_SWEEP, CRF_SCORE_EPS, CRF_T, crf_filter, crf_inference_label, crf_ir_label,
                  crf_label_sweep, crf_prob, crf_score_sweep)
from .eval_counts import (BAND_MAX_D, EVAL_CLASSES, EVAL_MAX_CLASSES, EVAL_MAX_THRES, boundary_distance, cam_confusion, cam_confusion_matrices,
                          eval_thresholds, ir_label_confusion, label_band, label_boundary_counts, label_confusion, mask_boundary_overlap,
                          mask_overlap)
from .gemm import (conv1x1_algo_count, conv1x1_nhwc, conv3x3_split, gemm16_algo_count, gemm16_nhwc, gemm_ranks, gemm_ranks16,
                   gemm_ranks3x3, split16, split16_pad, split_overflowed, split_weight, split_weight_3x3)
from .gemm import sample_flags as split_sample_flags
from .instance import (PendingDetections, PendingOverlaps, PendingRleDetections, argmax_rethreshold_batch, cluster_centroids,
                       cluster_centroids_batch, detect_batch_count, detect_instance, detect_instance_batch, detect_instance_rle_batch,
                       detection_overlap_batch, find_centroids_batch, find_centroids_with_refinement, label4)
from .label import cam_merge, label_epilogue, label_sweep_confusion
from .seg_loss import SEG_FUSE_MAX_MAPS, seg_argmax, seg_cross_entropy, seg_fuse, seg_loss_sums
from .msf import bicubic_plan, bicubic_resize, msf_pack, normalize_lut, rescale_size

# the two helpers tests and tools used to reach under their private names: callers written against those keep working
_bn_act_backward, _detect_batch_count = bn_act_backward, detect_batch_count
