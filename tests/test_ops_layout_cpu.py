"""`irn_amd.ops` as a facade, and the packed device-to-host layouts of the three batched detection calls read back by
their `Pending*` classes.  No GPU and no library call: the buffers are plain host tensors filled here at byte offsets
written out by hand from the layouts the output arrays of irn_detect_instance_batch_emit, _rle_count and _overlap
(include/irn_hip.h) are packed in."""
import numpy as np
import torch

from irn_amd import instance, ops

# the names `ops` defined or imported (without a leading underscore) before its code moved into one module per kernel file
OPS_NAMES = [
    "AUGMENT_DESC_WORDS", "AUGMENT_LABEL_DESC_WORDS", "AugmentTables", "C", "CRF_GT_PROB", "CRF_T", "EVAL_CLASSES",
    "EVAL_MAX_THRES", "LabelTables", "PendingDetections", "PendingOverlaps", "PendingRleDetections",
    "argmax_rethreshold_batch", "augment_batch", "augment_label_tables", "augment_pair_batch", "augment_tables",
    "bicubic_plan", "bicubic_resize", "bn_act", "bn_act_", "bn_fold", "bn_param_grads", "cam_confusion",
    "cam_confusion_matrices", "cam_merge", "check", "cluster_centroids", "cluster_centroids_batch", "collections",
    "conv1x1_algo_count", "conv1x1_nhwc", "conv3x3_split", "crf_filter", "crf_inference_label", "crf_ir_label",
    "detect_instance", "detect_instance_batch", "detect_instance_rle_batch", "detection_overlap_batch", "eval_thresholds",
    "find_centroids_batch", "find_centroids_with_refinement", "gemm16_algo_count", "gemm16_nhwc", "gemm_ranks",
    "gemm_ranks16", "gemm_ranks3x3", "i32_array", "label4", "label_confusion", "label_epilogue", "label_sweep_confusion",
    "lib", "mask_overlap", "mask_rle", "msf_pack", "nearest_plan", "normalize_lut", "np", "ptr_array", "read_back",
    "rescale_size", "rle_decode", "rle_from_string", "rle_to_string", "split16", "split16_pad", "split_overflowed",
    "split_weight", "split_weight_3x3", "stem_pool", "torch", "upsample_bilinear"]


def test_ops_keeps_every_public_name():
    assert len(OPS_NAMES) == 74 and len(set(OPS_NAMES)) == 74
    assert [n for n in OPS_NAMES if not hasattr(ops, n)] == []
    assert ops.detect_batch_count is instance.detect_batch_count and callable(ops.bn_act_backward)
    # callers written against the former private names of these two still find them
    assert ops._detect_batch_count is ops.detect_batch_count and ops._bn_act_backward is ops.bn_act_backward


class _Done:
    def synchronize(self):
        pass


NDS = [2, 0, 1]
CLASS_IDS = [np.array([3, 7, 9], np.int64), np.array([1], np.int64), np.array([5, 6], np.int64)]


def _put(buf, at, values, dtype):
    """Write `values` as `dtype` at byte offset `at` of the uint8 tensor `buf`; -> the array written."""
    v = np.asarray(values, dtype).reshape(-1)
    buf.numpy()[at:at + v.nbytes] = v.view(np.uint8)
    return np.asarray(values, dtype)


def _same(got, want, dtype):
    want = np.asarray(want)
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want)


def _is_nothing(rec):
    assert isinstance(rec, ValueError) and str(rec) == "detect_instance: no foreground pixel in any channel"


def test_dense_layout_unpacks():
    """Per image score f32 [nd] | channel i32 [nd] | pad to 16 | masks u8 [nd*h*w] | pad to 16.  Image 0 (nd 2, 3x5): score 0,
    channel 8, masks 16..46, padded to 48.  Image 1 has nothing.  Image 2 (nd 1, 2x7): score 48, channel 52, the 8-byte
    head padded to 64, masks 64..78, padded to 80."""
    hs, ws = [3, 4, 2], [5, 4, 7]
    rng = np.random.RandomState(0)
    m0, m2 = rng.randint(0, 2, (2, 3, 5)), rng.randint(0, 2, (1, 2, 7))
    buf = torch.full((80,), 0xEE, dtype=torch.uint8)               # pads hold rubbish: nothing may read them
    _put(buf, 0, [0.5, 0.25], np.float32), _put(buf, 8, [2, 0], np.int32), _put(buf, 16, m0, np.uint8)
    _put(buf, 48, [0.75], np.float32), _put(buf, 52, [1], np.int32), _put(buf, 64, m2, np.uint8)
    lay = instance._dense_layout(NDS, hs, ws)
    assert lay.nbytes == 80
    timings = {}
    pending = instance.PendingDetections(NDS, buf, _Done(), timings, 0.0, lay, hs, ws, CLASS_IDS)
    out = pending.result()
    assert len(out) == 3 and sorted(out[0]) == sorted(out[2]) == ["class", "mask", "score"]
    _same(out[0]["score"], np.float32([0.5, 0.25]), np.float32)
    _same(out[0]["class"], [9, 3], np.int64)
    _same(out[0]["mask"], m0.astype(bool), np.bool_)
    _is_nothing(out[1])
    _same(out[2]["score"], np.float32([0.75]), np.float32)
    _same(out[2]["class"], [6], np.int64)
    _same(out[2]["mask"], m2.astype(bool), np.bool_)
    assert np.shares_memory(out[0]["mask"], buf.numpy()) and np.shares_memory(out[2]["score"], buf.numpy())      # views
    assert set(timings) == {"emit_d2h", "unpack"}
    assert pending.result() is out
    # a batch without any detection brings nothing back
    empty = instance.PendingDetections([0, 0], None, None, None, 0.0, instance._dense_layout([0, 0], [3, 4], [5, 4]), [3, 4], [5, 4],
                                       CLASS_IDS)
    res = empty.result()
    assert len(res) == 2 and empty.result() is res
    _is_nothing(res[0]), _is_nothing(res[1])


def test_rle_layout_unpacks():
    """Head for G = 3 detections: score f32 [G] at 0 | channel i32 [G] at 12 | area i32 [G] at 24 | n_runs i32 [G] at 36 |
    bbox i32 [G][4] at 48, 96 bytes; the run lengths are uint32, detection after detection."""
    hs, ws = [3, 4, 2], [5, 4, 7]
    head = torch.zeros(96, dtype=torch.uint8)
    _put(head, 0, [0.5, 0.25, 0.75], np.float32), _put(head, 12, [2, 0, 1], np.int32), _put(head, 24, [7, 15, 4], np.int32)
    _put(head, 36, [3, 1, 4], np.int32)
    bbox = _put(head, 48, [[0, 1, 2, 2], [0, 0, 5, 3], [3, 0, 2, 2]], np.int32)
    counts = torch.zeros(32, dtype=torch.uint8)
    runs = _put(counts, 0, [4, 7, 4, 15, 6, 2, 4, 2], np.uint32)
    lay = instance._rle_head_layout(3)
    assert lay.nbytes == 96
    pending = instance.PendingRleDetections(NDS, counts, _Done(), None, 0.0, lay, head.numpy(), hs, ws, CLASS_IDS)
    out = pending.result()
    assert len(out) == 3 and sorted(out[0]) == sorted(out[2]) == ["area", "bbox", "class", "counts", "offsets", "score", "size"]
    _same(out[0]["score"], np.float32([0.5, 0.25]), np.float32)
    _same(out[0]["class"], [9, 3], np.int64)
    assert out[0]["size"] == (3, 5) and out[2]["size"] == (2, 7)
    _same(out[0]["counts"], runs[:4], np.uint32)
    _same(out[0]["offsets"], [0, 3, 4], np.int64)
    _same(out[0]["area"], [7, 15], np.int64)
    _same(out[0]["bbox"], bbox[:2], np.int32)
    _is_nothing(out[1])
    _same(out[2]["score"], np.float32([0.75]), np.float32)
    _same(out[2]["class"], [6], np.int64)
    _same(out[2]["counts"], runs[4:], np.uint32)
    _same(out[2]["offsets"], [0, 4], np.int64)
    _same(out[2]["area"], [4], np.int64)
    _same(out[2]["bbox"], bbox[2:], np.int32)
    assert np.shares_memory(out[2]["counts"], counts.numpy())                                                     # views
    assert pending.result() is out


def test_overlap_layout_unpacks():
    """inter i64 [NI] | area_gt i64 [NG] | area_pred i64 [G] | score f32 [G] | channel i32 [G] with nds = [2, 0, 1] and
    gs = [1, 2, 0]: NI = 2, NG = 3, G = 3, so inter at 0, area_gt at 16, area_pred at 40, score at 64, channel at 76; 88 bytes.
    Image 1 has GT and no detection, image 2 a detection and no GT."""
    gs = [1, 2, 0]
    buf = torch.zeros(88, dtype=torch.uint8)
    _put(buf, 0, [11, 2 ** 40], np.int64), _put(buf, 16, [30, 31, 32], np.int64), _put(buf, 40, [20, 21, 22], np.int64)
    _put(buf, 64, [0.5, 0.25, 0.75], np.float32), _put(buf, 76, [2, 0, 1], np.int32)
    lay = instance._overlap_layout(NDS, gs)
    assert lay.nbytes == 88
    pending = instance.PendingOverlaps(NDS, buf, _Done(), lay, gs, CLASS_IDS)
    out = pending.result()
    assert len(out) == 3 and all(sorted(r) == ["area_gt", "area_pred", "inter", "pred_class", "pred_score"] for r in out)
    _same(out[0]["pred_class"], [9, 3], np.int64)
    _same(out[0]["pred_score"], np.float32([0.5, 0.25]), np.float32)
    _same(out[0]["inter"], [[11], [2 ** 40]], np.int64)
    _same(out[0]["area_pred"], [20, 21], np.int64)
    _same(out[0]["area_gt"], [30], np.int64)
    _same(out[1]["pred_class"], np.zeros(0, np.int64), np.int64)                      # the N = 0 record with its GT areas
    _same(out[1]["pred_score"], np.zeros(0, np.float32), np.float32)
    _same(out[1]["inter"], np.zeros((0, 2), np.int64), np.int64)
    _same(out[1]["area_pred"], np.zeros(0, np.int64), np.int64)
    _same(out[1]["area_gt"], [31, 32], np.int64)
    _same(out[2]["pred_class"], [6], np.int64)
    _same(out[2]["pred_score"], np.float32([0.75]), np.float32)
    _same(out[2]["inter"], np.zeros((1, 0), np.int64), np.int64)
    _same(out[2]["area_pred"], [22], np.int64)
    _same(out[2]["area_gt"], np.zeros(0, np.int64), np.int64)
    assert not any(np.shares_memory(a, buf.numpy()) for r in out for a in r.values())                             # copies
    assert pending.result() is out


def test_packed_layout_offsets():
    from irn_amd._host import PackedLayout
    f32, u8, i64, i32 = (np.dtype(t) for t in (np.float32, np.uint8, np.int64, np.int32))
    lay = PackedLayout([("a", f32, 3, 16), ("b", u8, 5, 1), ("c", i64, 0, 8), ("d", i32, 2, 16), ("end", u8, 0, 16)])
    assert lay.offsets == {"a": 0, "b": 12, "c": 24, "d": 32, "end": 48} and lay.nbytes == 48
    assert lay.ptrs(1000) == [1000, 1012, None, 1032, None]
    views = lay.views(np.arange(48, dtype=np.uint8))
    assert [(v.dtype, v.shape) for v in views] == [(np.float32, (3,)), (np.uint8, (5,)), (np.int64, (0,)), (np.int32, (2,)), (np.uint8, (0,))]
    assert views[1].tolist() == [12, 13, 14, 15, 16] and views[3].tobytes() == bytes(range(32, 40))
