"""Host logic of step/tune_ir_label.py and the argument checks of its two entries, no GPU: the three new symbols are
declared, exported and bound; the ops refuse CPU tensors; irn_crf_label_sweep and irn_ir_label_confusion refuse bad arguments
by name before touching a device (null device pointers throughout); the sweep's workspace bound; the grid (the configured
values are always on it, values told apart as float32, the refusals); the scores of a hand-made histogram; `best` and its
ties; the printed lines; the command line."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("irn_crf_sweep_workspace_bytes", "irn_crf_label_sweep", "irn_ir_label_confusion")
IRN_ERR_ARG = 1


def test_symbols_are_declared_exported_and_bound():
    from irn_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "irn_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS and getattr(_lib.lib, name).argtypes is not None, name
    assert re.search(r"#define\s+IRN_CRF_MAX_SWEEP\s+16\b", src) and ops.CRF_MAX_SWEEP == 16
    assert callable(ops.crf_label_sweep) and callable(ops.ir_label_confusion)


def test_ops_refuse_cpu_tensors():
    from irn_amd import ops
    img = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.crf_label_sweep(img, torch.zeros((1, 4, 4)), [0], [0.1, 0.2])
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.ir_label_confusion(torch.zeros((2, 4, 4), dtype=torch.uint8), [0], [1], torch.zeros((4, 4), dtype=torch.uint8))


def _sweep(thres, k=1, h=4, w=4):
    from irn_amd import _lib
    th = (C.c_float * max(len(thres), 1))(*thres)
    rc = _lib.lib.irn_crf_label_sweep(None, None, None, k, h, w, th, len(thres), 10, 0.7, None, None, 0, None)
    return rc, _lib.lib.irn_last_error().decode()


@pytest.mark.parametrize("kw,cause", [
    (dict(thres=[]), r"t_count 0 outside 1\.\.16"),
    (dict(thres=list(np.linspace(0.1, 0.9, 17))), r"t_count 17 outside 1\.\.16"),
    (dict(thres=[0.3, 0.2]), "not strictly ascending"),
    (dict(thres=[0.1, 0.2, 0.2]), "not strictly ascending"),
    (dict(thres=[0.1, float("nan"), 0.3]), "threshold 1 is NaN"),
    (dict(thres=[float("nan")]), "threshold 0 is NaN"),
    (dict(thres=[0.1], k=32), r"n_labels 33 outside 1\.\.32"),
    (dict(thres=[0.1], h=0), "bad image size 0x4"),
    (dict(thres=[0.1, 0.2]), "null pointer"),
])
def test_label_sweep_refusals_name_the_cause(kw, cause):
    rc, msg = _sweep(**kw)
    assert rc == IRN_ERR_ARG and msg.startswith("irn_crf_label_sweep: ") and re.search(cause, msg), msg


def _confusion(t_count, fg, bg):
    from irn_amd import _lib
    f = (C.c_int32 * max(len(fg), 1))(*fg)
    b = (C.c_int32 * max(len(bg), 1))(*bg)
    rc = _lib.lib.irn_ir_label_confusion(None, t_count, f, len(fg), b, len(bg), None, 4, 4, 21, None, None, None)
    return rc, _lib.lib.irn_last_error().decode()


@pytest.mark.parametrize("args,cause", [
    ((4, [], [0]), r"f=0 x b=1"),
    ((4, [0], [0] * 17), r"f=1 x b=17"),
    ((4, [1, 4], [0]), r"fg_idx\[1\] = 4 outside \[0, t_count = 4\)"),
    ((4, [0], [3, 4]), r"bg_idx\[1\] = 4 outside"),
    ((4, [0], [-1]), r"bg_idx\[0\] = -1 outside"),
    ((0, [0], [0]), r"t_count 0 outside"),
    ((17, [0], [0]), r"t_count 17 outside"),
    ((4, [3], [0]), "null pointer"),
])
def test_ir_label_confusion_refusals_name_the_cause(args, cause):
    rc, msg = _confusion(*args)
    assert rc == IRN_ERR_ARG and msg.startswith("irn_ir_label_confusion: ") and re.search(cause, msg), msg


def test_sweep_workspace_is_bounded_by_the_largest_single_call():
    from irn_amd._lib import lib
    single = lib.irn_crf_workspace_bytes(375, 500, 32)
    assert single > 0
    for n_labels, t_count in ((21, 16), (32, 16), (2, 16), (21, 1), (4, 8)):
        need = lib.irn_crf_sweep_workspace_bytes(375, 500, n_labels, t_count)
        assert 0 < need <= single + 16 * 375 * 500 * 8, (n_labels, t_count, need)
    # the lattice value arrays do not scale with t_count: 16 thresholds cost 15 more seed planes of int32 than one
    one, many = lib.irn_crf_sweep_workspace_bytes(375, 500, 32, 2), lib.irn_crf_sweep_workspace_bytes(375, 500, 32, 16)
    assert many - one <= 14 * (375 * 500 * 4 + 256)
    assert lib.irn_crf_sweep_workspace_bytes(375, 500, 21, 17) == 0 and lib.irn_crf_sweep_workspace_bytes(375, 500, 21, 0) == 0
    assert lib.irn_crf_sweep_workspace_bytes(375, 500, 33, 4) == 0 and lib.irn_crf_sweep_workspace_bytes(0, 500, 21, 4) == 0


def _args(**kw):
    base = dict(conf_fg_thres=0.30, conf_bg_thres=0.05, tune_conf_fg_thres=[], tune_conf_bg_thres=[])
    base.update(kw)
    return argparse.Namespace(**base)


def test_grid_holds_the_configured_values_sorted_and_deduped_as_float32():
    from irn_amd.step import tune_ir_label as T
    fgs, bgs, th32, fi, bi = T.grid_axes(_args())
    assert fgs == [0.3] and bgs == [0.05] and th32.dtype == np.float32 and np.array_equal(th32, np.float32([0.05, 0.3]))
    assert fi.tolist() == [1] and bi.tolist() == [0]
    fgs, bgs, th32, fi, bi = T.grid_axes(_args(tune_conf_fg_thres=[0.5, 0.2, 0.3, 0.2 + 1e-10, 0.5],
                                               tune_conf_bg_thres=[0.2, 0.01, 0.05]))
    assert fgs == [0.2, 0.3, 0.5] and bgs == [0.01, 0.05, 0.2]
    assert np.array_equal(th32, np.float32([0.01, 0.05, 0.2, 0.3, 0.5]))                # 0.2 is one CRF for both axes
    assert fi.tolist() == [2, 3, 4] and bi.tolist() == [0, 1, 2] and fi.dtype == np.int32
    # a configured value that differs from a swept one only below float32 resolution names the point
    fgs, _, th32, _, _ = T.grid_axes(_args(conf_fg_thres=0.3, tune_conf_fg_thres=[0.3 + 1e-12, 0.4]))
    assert fgs == [0.3, 0.4] and len(th32) == 3
    # a Namespace built by hand without the tune axes
    assert T.grid_axes(argparse.Namespace(conf_fg_thres=0.3, conf_bg_thres=0.05))[:2] == ([0.3], [0.05])


def test_grid_refusals():
    from irn_amd.step import tune_ir_label as T
    T.grid_axes(_args(conf_bg_thres=0.3, tune_conf_fg_thres=list(np.linspace(0.31, 0.9, 15))))            # 16 on one axis, 16 in all
    with pytest.raises(ValueError, match="17 foreground thresholds"):
        T.grid_axes(_args(conf_bg_thres=0.3, tune_conf_fg_thres=list(np.linspace(0.31, 0.9, 16))))
    with pytest.raises(ValueError, match="17 background thresholds"):
        T.grid_axes(_args(conf_fg_thres=0.05, tune_conf_bg_thres=list(np.linspace(0.06, 0.2, 16))))
    with pytest.raises(ValueError, match="17 distinct thresholds over both axes"):
        T.grid_axes(_args(tune_conf_fg_thres=list(np.linspace(0.31, 0.9, 8)), tune_conf_bg_thres=list(np.linspace(0.06, 0.2, 7))))
    with pytest.raises(ValueError, match="foreground threshold is NaN"):
        T.grid_axes(_args(tune_conf_fg_thres=[float("nan")]))
    with pytest.raises(ValueError, match="background threshold is NaN"):
        T.grid_axes(_args(conf_bg_thres=float("nan")))


def _hand_hist():
    """3 classes (0, 1, 2) and a void row.  Class 2 has ground truth but no confident pixel anywhere."""
    h = np.zeros((22, 22), np.int64)
    h[0, 0], h[0, 1], h[0, 21] = 50, 4, 6
    h[1, 0], h[1, 1], h[1, 21] = 3, 20, 7
    h[2, 21] = 10                                   # every class-2 pixel is unsure
    h[21, 0], h[21, 1], h[21, 21] = 5, 2, 9         # void ground truth: counted nowhere in the scores
    return h


def test_scores_of_a_hand_made_histogram():
    from irn_amd.misc import evaluation
    s = evaluation.ir_label_scores(_hand_hist())
    # confident pixels: conf = [[50, 4], [3, 20]] over the observed classes 0..1 (class 2 never occurs among them)
    assert np.allclose(s["iou"], [50 / 57, 20 / 27], rtol=0, atol=1e-15) and s["miou"] == pytest.approx((50 / 57 + 20 / 27) / 2, abs=1e-15)
    assert s["coverage"] == 77 / 100
    want_all = np.full(21, np.nan)
    want_all[:3] = [50 / (60 + 53 - 50), 20 / (30 + 24 - 20), 0 / 10]
    assert np.array_equal(s["iou_all"], want_all, equal_nan=True)
    assert s["miou_all"] == np.mean(want_all[:3])
    # a class with ground truth, labelled pixels elsewhere, but no confident pixel of its own GT: iou 0; never seen at all: NaN
    h = _hand_hist()
    h[2, 21] = 0
    h[2, 1] = 10
    s = evaluation.ir_label_scores(h)
    assert len(s["iou"]) == 3 and s["iou"][2] == 0 and s["coverage"] == 87 / 100
    empty = evaluation.ir_label_scores(np.zeros((22, 22), np.int64))
    assert np.isnan(empty["miou"]) and np.isnan(empty["coverage"]) and np.isnan(empty["miou_all"])
    # a class with no confident pixel in a matrix that reaches beyond it gives a NaN iou
    h = _hand_hist()
    h[3, 3] = 5
    s = evaluation.ir_label_scores(h)
    assert len(s["iou"]) == 4 and np.isnan(s["iou"][2]) and s["miou"] == pytest.approx((50 / 57 + 20 / 27 + 1) / 3, abs=1e-15)


def test_best_prefers_miou_all_then_small_fg_then_small_bg():
    from irn_amd.step import tune_ir_label as T
    assert T.pick_best({(0.3, 0.05): 0.5, (0.45, 0.15): 0.7, (0.3, 0.15): 0.6}) == (0.45, 0.15)
    assert T.pick_best({(0.45, 0.05): 0.7, (0.3, 0.15): 0.7, (0.3, 0.05): 0.7, (0.2, 0.2): 0.6}) == (0.3, 0.05)
    assert T.pick_best({(0.3, 0.05): float("nan"), (0.9, 0.9): 0.0}) == (0.9, 0.9)
    assert T.pick_best({(0.3, 0.05): float("nan")}) == (0.3, 0.05)


def test_report_prints_the_configured_point_the_grid_and_the_best(capsys):
    from irn_amd.misc import evaluation
    from irn_amd.step import tune_ir_label as T
    fgs, bgs, _, _, _ = T.grid_axes(_args(tune_conf_fg_thres=[0.45], tune_conf_bg_thres=[0.15]))
    hist = np.zeros((2, 2, 22, 22), np.int64)
    hist[:] = _hand_hist()
    hist[1, 0, 1, 1] += 10                          # (0.45, 0.05) scores best ...
    hist[1, 0, 1, 21] -= 7
    hist[1, 1] = hist[1, 0]                         # ... tied with (0.45, 0.15): the smaller bg wins
    out = T.report(hist, fgs, bgs, (0.3, 0.05))
    lines = capsys.readouterr().out.splitlines()
    here = evaluation.ir_label_scores(hist[0, 0])
    assert lines[0] == str({k: here[k] for k in ("iou", "miou", "coverage", "miou_all")})
    points = [(0.3, 0.05), (0.3, 0.15), (0.45, 0.05), (0.45, 0.15)]
    for ln, (p, (i, j)) in zip(lines[1:5], zip(points, ((0, 0), (0, 1), (1, 0), (1, 1)))):
        s = evaluation.ir_label_scores(hist[i, j])
        assert ln == "fg %g bg %g miou %.6f coverage %.6f miou_all %.6f" % (p + (s["miou"], s["coverage"], s["miou_all"]))
    assert out["best"] == (0.45, 0.05) and lines[5] == "best " + lines[3] and len(lines) == 6
    assert list(out["grid"]) == points and out["grid"][(0.3, 0.05)] == here["miou_all"] == out["miou_all"]
    assert out["grid"][(0.45, 0.05)] > out["grid"][(0.3, 0.05)] and out["hist"] is hist
    assert set(out) == {"iou", "miou", "coverage", "miou_all", "grid", "scores", "hist", "best"}


def test_parser_accepts_the_flags_and_the_pass_is_off_by_default():
    import run_sample
    p = run_sample.build_parser()
    a = p.parse_args(["--voc12_root", "x"])
    assert a.tune_ir_label_pass is False and a.tune_conf_fg_thres == [] and a.tune_conf_bg_thres == []
    a = p.parse_args(["--voc12_root", "x", "--tune_ir_label_pass", "True", "--tune_conf_fg_thres", "0.45", "0.2",
                      "--tune_conf_bg_thres", "0.15"])
    assert a.tune_ir_label_pass is True and a.tune_conf_fg_thres == [0.45, 0.2] and a.tune_conf_bg_thres == [0.15]
    assert (a.conf_fg_thres, a.conf_bg_thres) == (0.30, 0.05)
