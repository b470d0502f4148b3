"""ctypes binding of libirn_hip.so (C ABI declared in include/irn_hip.h).

There is no CPU fallback: if the library is missing, importing this module raises.  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C irn_amd/csrc``.
"""
import ctypes as C
import os

# PyTorch-ROCm owns the process's HIP runtime (it ships its own libamdhip64.so.7).  It must be
# loaded BEFORE libirn_hip.so so that the library binds to the same runtime instance: loading ours
# first pulls in /opt/rocm's copy, the process ends up with two runtimes, and ours then reports
# "no ROCm-capable device" while torch works (seen on the GPU box under pytest's import order).
import torch  # noqa: F401  (side effect: HIP runtime of the process)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IRN_HIP_LIB") or os.path.join(_HERE, "lib", "libirn_hip.so")   # override: A/B runs of two builds

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "irn_amd: %s not found — the HIP extension is the product path and has no fallback; "
        "build it with `make -C irn_amd/csrc` (needs hipcc, targets gfx950)" % LIB_PATH)

lib = C.CDLL(LIB_PATH)

# The bindings below are by name only, so a library built from another commit would be called with argument lists it
# does not have.  IRN_ABI_VERSION of include/irn_hip.h moves with every such change; this is the value _SIGS is written for.
ABI_VERSION = 106
lib.irn_version.restype, lib.irn_version.argtypes = C.c_int, []
if lib.irn_version() != ABI_VERSION:
    raise ImportError("irn_amd: %s reports ABI version %d, these bindings need %d — it was built from another commit; "
                      "rebuild it with `make -C irn_amd/csrc`" % (LIB_PATH, lib.irn_version(), ABI_VERSION))

vp, i32, f32, sz, i64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64
pi32 = C.POINTER(C.c_int32)
ppv = C.POINTER(C.c_void_p)

_SIGS = {
    "irn_version": (C.c_int, []),
    "irn_last_error": (C.c_char_p, []),
    "irn_path_count": (i32, [i32, C.POINTER(i32), C.POINTER(i32)]),
    "irn_path_table": (i32, [i32, i32, pi32, pi32, pi32]),
    "irn_edge_to_affinity": (i32, [vp, i32, i32, i32, i32, vp, vp]),
    "irn_edge_to_affinity_backward": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    "irn_pair_displacement": (i32, [vp, i32, i32, i32, i32, i32, vp, vp]),
    "irn_pair_displacement_backward": (i32, [vp, i32, i32, i32, i32, i32, vp, vp]),
    "irn_aff_loss_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "irn_aff_loss_forward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    "irn_aff_loss_backward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "irn_aff_loss_backward_ordered": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "irn_seg_loss_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32, i32]),
    "irn_seg_loss_forward": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "irn_seg_loss_backward": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp]),
    "irn_seg_argmax": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
    "irn_seg_fuse": (i32, [ppv, pi32, pi32, pi32, pi32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "irn_walk_create": (i32, [i32, C.POINTER(vp)]),
    "irn_walk_destroy": (i32, [vp]),
    "irn_walk_configure": (i32, [vp, i32, pi32, pi32, pi32, C.POINTER(sz)]),
    "irn_walk_run": (i32, [vp, ppv, ppv, ppv, pi32, ppv, f32, i32, vp, sz, vp]),
    "irn_walk_set_option": (i32, [vp, C.c_char_p, i32]),
    "irn_walk_steps": (i32, [vp, i32, C.POINTER(i32)]),
    "irn_power_series": (i32, [i32, i32, C.POINTER(C.c_double), i32, C.POINTER(i32), C.POINTER(i32)]),
    "irn_walk_sync": (i32, [vp, C.POINTER(i32)]),
    "irn_walk_check": (i32, [vp]),
    "irn_walk_fallback_runs": (i32, [vp]),
    "irn_walk_tuning": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(f32)]),
    "irn_walk_plan_rounds": (i32, [i32, i32, pi32, pi32, pi32, i32, i32, pi32, i32, C.POINTER(i32)]),
    "irn_walk_read_profile": (i32, [vp, vp]),
    "irn_walk_enable_timing": (i32, [vp, i32]),
    "irn_walk_last_sweep_ms": (i32, [vp, C.POINTER(f32), C.POINTER(i32)]),
    "irn_walk_export_weights": (i32, [vp, i32, vp, vp, vp, vp]),
    "irn_label_epilogue": (i32, [i32, ppv, pi32, pi32, pi32, pi32, pi32, f32, ppv, ppv, ppv, ppv, vp, vp]),
    "irn_cam_merge": (i32, [i32, ppv, pi32, pi32, i32, vp, i32, i32, i32, vp, vp, vp, vp]),
    "irn_bicubic_plan": (i32, [i32, i32, pi32, pi32, pi32, pi32, sz]),
    "irn_bicubic_scratch_bytes": (sz, [i32, i32, i32, i32, i32]),
    "irn_bicubic_resize_u8": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    "irn_msf_pack": (i32, [vp, i32, i32, i32, pi32, pi32, vp, ppv, vp, vp]),
    "irn_augment_batch": (i32, [i32, i32, pi32, sz, vp, sz, vp, vp, sz, vp, sz, vp, sz, vp]),
    "irn_augment_label_batch": (i32, [i32, i32, i32, pi32, sz, vp, sz, vp, sz, vp, sz, vp]),
    "irn_bn_act": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, i64, i32, vp]),
    "irn_bn_act_nhwc": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp]),
    "irn_bn_fold": (i32, [vp, vp, vp, vp, C.c_double, i32, vp, vp, vp]),
    "irn_bn_act_forward": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i32, i64, i32, vp]),
    "irn_bn_act_backward_workspace_bytes": (sz, [i64, i32, i64]),
    "irn_bn_act_backward": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i64, i32, vp, sz, vp]),
    "irn_conv1x1_workspace_bytes": (sz, []),
    "irn_conv1x1_algo_count": (i32, [i64, i32, i32, i32, i32, i32, sz, C.POINTER(i32)]),
    "irn_conv1x1_nhwc": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, sz, vp]),
    "irn_split16": (i32, [vp, vp, vp, i32, vp, i64, i32, i64, vp, vp]),
    "irn_split16_pad": (i32, [vp, vp, vp, i32, vp, i64, i32, i32, i32, i32, i32, i32, vp, vp]),
    "irn_conv3x3_split_gemm": (i32, [vp, vp, vp, i64, i32, i32, i32, i32, f32, i32, i32, vp, sz, vp]),
    "irn_gemm16_algo_count": (i32, [i64, i32, i32, i32, i32, i32, sz, C.POINTER(i32)]),
    "irn_gemm16_nhwc": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, f32, i32, vp, sz, vp]),
    "irn_stem_pool": (i32, [vp, vp, vp, i64, i32, i32, i32, vp, vp]),
    "irn_upsample_bilinear": (i32, [vp, i64, i32, i32, i32, i32, vp, vp]),
    "irn_upsample_bilinear_backward": (i32, [vp, vp, i64, i32, i32, i32, i32, vp, vp]),
    "irn_find_centroids_batch": (i32, [i32, ppv, pi32, pi32, i32, ppv, vp]),
    "irn_cluster_batch_scratch_bytes": (sz, [i32, pi32, pi32]),
    "irn_cluster_centroids_batch": (i32, [i32, ppv, ppv, pi32, pi32, f32, ppv, vp, vp, vp]),
    "irn_ccl_scratch_bytes": (sz, [i32, i32, i32]),
    "irn_label4": (i32, [vp, i32, i32, i32, vp, vp, vp, vp]),
    "irn_detect_batch_scratch_bytes": (sz, [i32, pi32, pi32, pi32]),
    "irn_detect_instance_batch_count": (i32, [i32, ppv, ppv, pi32, pi32, pi32, vp, vp, vp]),
    "irn_detect_instance_batch_emit": (i32, [i32, ppv, ppv, pi32, pi32, pi32, pi32, C.POINTER(C.c_double), ppv, ppv, ppv, vp, vp]),
    "irn_detect_instance_batch_rle_scratch_bytes": (sz, [i32, pi32, pi32, pi32]),
    "irn_detect_instance_batch_rle_count": (i32, [i32, ppv, ppv, pi32, pi32, pi32, pi32, C.POINTER(C.c_double), vp, vp, vp, vp, vp, vp, vp, vp]),
    "irn_detect_instance_batch_rle_sort_bytes": (sz, [i64, i32]),
    "irn_detect_instance_batch_rle_emit": (i32, [i32, pi32, pi32, pi32, C.POINTER(i64), vp, vp, vp, sz, vp]),
    "irn_detect_instance_batch_overlap": (i32, [i32, ppv, ppv, pi32, pi32, pi32, pi32, C.POINTER(C.c_double), ppv, pi32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "irn_argmax_rethreshold_batch": (i32, [i32, ppv, ppv, pi32, pi32, pi32, f32, ppv, vp]),
    "irn_crf_filter_workspace_bytes": (sz, [i32, i32, i32]),
    "irn_crf_filter": (i32, [vp, i32, i32, vp, i32, vp, pi32, vp, vp, vp, sz, vp]),
    "irn_crf_workspace_bytes": (sz, [i32, i32, i32]),
    "irn_crf_inference_label": (i32, [vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, sz, vp]),
    "irn_crf_ir_label": (i32, [vp, vp, vp, i32, i32, i32, f32, f32, i32, f32, vp, vp, sz, vp]),
    "irn_crf_sweep_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "irn_crf_label_sweep": (i32, [vp, vp, vp, i32, i32, i32, C.POINTER(f32), i32, i32, f32, vp, vp, sz, vp]),
    "irn_crf_score_sweep_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "irn_crf_score_sweep": (i32, [vp, vp, vp, i32, i32, i32, C.POINTER(f32), i32, i32, vp, vp, vp, sz, vp]),
    "irn_crf_prob_workspace_bytes": (sz, [i32, i32, i32]),
    "irn_crf_prob": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    "irn_mask_overlap": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "irn_ir_label_confusion": (i32, [vp, i32, pi32, i32, pi32, i32, vp, i32, i32, i32, vp, vp, vp]),
    "irn_cam_confusion": (i32, [vp, vp, i32, vp, i32, i32, vp, i32, i32, vp, vp, vp]),
    "irn_cam_confusion_reduce": (i32, [vp, i32, i32, vp, vp, vp]),
    "irn_label_confusion": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "irn_label_band": (i32, [vp, i32, i32, i32, vp, vp]),
    "irn_label_boundary_counts": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    "irn_mask_boundary_overlap": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "irn_label_sweep_confusion": (i32, [i32, ppv, pi32, pi32, pi32, pi32, pi32, ppv, ppv, vp, i32, i32, vp, vp, vp, vp]),
    "irn_mask_rle_scratch_bytes": (sz, [i32, i32, i32]),
    "irn_mask_rle_count": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "irn_mask_rle_emit": (i32, [vp, i32, i32, i32, vp, vp, vp, vp]),
    "irn_mask_polygon_scratch_bytes": (sz, [i32, i32, i32]),
    "irn_mask_polygon_trace_scratch_bytes": (sz, [i32]),
    "irn_mask_polygon_edges": (i32, [vp, i32, i32, i32, vp, vp, vp]),
    "irn_mask_polygon_count": (i32, [vp, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
    "irn_mask_polygon_emit": (i32, [i32, vp, i64, vp, i64, vp, vp]),
}

EXPORTS = tuple(_SIGS)

for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)          # AttributeError here = header and library disagree
    _fn.restype = _res
    _fn.argtypes = _args


class IrnHipError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        msg = lib.irn_last_error()
        raise IrnHipError("libirn_hip status %d: %s" % (rc, msg.decode() if msg else "?"))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise ValueError("%s must be a GPU tensor: the HIP path has no CPU fallback" % what)


def _need_cl(t, what, shape=None, device=None):
    """`t` is a channels-last fp32 4-D tensor (of `shape`, on `device`, where given); `what` = "function: argument"."""
    if (t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous(memory_format=torch.channels_last)
            or (shape is not None and tuple(t.shape) != tuple(shape)) or (device is not None and t.device != device)):
        raise ValueError("%s must be a channels-last fp32 %s tensor%s, got %s %s %s" % (
            what, "[N, C, H, W]" if shape is None else tuple(shape), "" if device is None else " on %s" % device, t.dtype, tuple(t.shape), t.stride()))


def _need_vec(t, what, n, device):
    """`t` is a contiguous fp32 [n] tensor on `device`."""
    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
        raise ValueError("%s must be a contiguous fp32 [%d] tensor on %s" % (what, n, device))


def i32_array(values):
    return (C.c_int32 * len(values))(*[int(v) for v in values])


def ptr_array(ptrs):
    """Host array of device pointers; None -> NULL."""
    return (C.c_void_p * len(ptrs))(*[None if p is None else int(p) for p in ptrs])
