"""Host logic of step/tune_sem_seg.py, no GPU: the grid (the configured point is always on it, thresholds told apart as
float32, the refusals), the tie-breaking of `best`, the printed lines on a hand-made accumulator, and the command line
(`--tune_sem_seg_pass` parses; without it nothing of the step is imported or run; without a GPU the step refuses loudly)."""
import argparse
import sys

import numpy as np
import pytest


def _args(**kw):
    base = dict(beta=10.0, exp_times=8, sem_seg_bg_thres=0.25, tune_beta=[], tune_exp_times=[], tune_bg_thres=[])
    base.update(kw)
    return argparse.Namespace(**base)


def test_grid_always_holds_the_configured_point_and_dedupes_as_float32():
    from irn_amd.step import tune_sem_seg as T
    assert T.grid_axes(_args()) [:3] == ([10.0], [8], [0.25])
    betas, exps, req, th32 = T.grid_axes(_args(tune_beta=[6, 14, 10], tune_exp_times=[5, 8, 5],
                                               tune_bg_thres=[0.4, 0.1, 0.25, 0.1 + 1e-10, 0.4]))
    assert betas == [6.0, 10.0, 14.0] and exps == [5, 8]
    assert req == [0.1, 0.25, 0.4] and th32.dtype == np.float32 and np.array_equal(th32, np.float32([0.1, 0.25, 0.4]))
    # a configured value that only differs from a swept one below float32 resolution names the point
    _, _, req, th32 = T.grid_axes(_args(sem_seg_bg_thres=0.3, tune_bg_thres=[0.3 + 1e-12, 0.2]))
    assert req == [0.2, 0.3] and len(th32) == 2
    # no axis given as None either (a Namespace built by hand)
    assert T.grid_axes(argparse.Namespace(beta=10, exp_times=8, sem_seg_bg_thres=0.25))[:3] == ([10.0], [8], [0.25])


def test_grid_refusals():
    from irn_amd.step import tune_sem_seg as T
    T.grid_axes(_args(tune_bg_thres=list(np.linspace(0.3, 0.9, 255))))                   # 256 with the configured one
    with pytest.raises(ValueError, match="257 background thresholds"):
        T.grid_axes(_args(tune_bg_thres=list(np.linspace(0.3, 0.9, 256))))
    with pytest.raises(ValueError, match="72 walks"):                                    # beta 10 is on the grid too: 9 x 8
        T.grid_axes(_args(tune_beta=list(range(1, 9)), tune_exp_times=list(range(1, 9))))
    assert len(T.grid_axes(_args(beta=8, tune_beta=list(range(1, 9)), tune_exp_times=list(range(1, 9))))[0]) == 8   # 64: allowed
    with pytest.raises(ValueError, match="NaN"):
        T.grid_axes(_args(tune_bg_thres=[float("nan")]))
    with pytest.raises(ValueError, match="negative"):
        T.grid_axes(_args(tune_exp_times=[-1]))


def test_best_prefers_miou_then_small_exp_times_beta_threshold():
    from irn_amd.step import tune_sem_seg as T
    assert T.pick_best({(10.0, 8, 0.25): 0.5, (6.0, 5, 0.4): 0.7, (14.0, 8, 0.1): 0.6}) == (6.0, 5, 0.4)
    tie = {(6.0, 8, 0.1): 0.7, (14.0, 5, 0.4): 0.7, (10.0, 5, 0.4): 0.7, (10.0, 5, 0.25): 0.7, (12.0, 6, 0.05): 0.7}
    assert T.pick_best(tie) == (10.0, 5, 0.25)                    # exp_times 5, then beta 10, then threshold 0.25
    assert T.pick_best({(10.0, 8, 0.25): float("nan"), (6.0, 9, 0.9): 0.0}) == (6.0, 9, 0.9)
    assert T.pick_best({(10.0, 8, 0.25): float("nan")}) == (10.0, 8, 0.25)


def test_report_prints_the_eval_lines_then_the_grid_then_the_best(capsys):
    from irn_amd.misc import evaluation
    from irn_amd.step import tune_sem_seg as T
    axes = T.grid_axes(_args(tune_beta=[6], tune_bg_thres=[0.4]))               # pairs (6, 8), (10, 8); thresholds 0.25, 0.4
    conf = np.zeros((2, 2, 21, 21), np.int64)
    void = np.zeros((2, 2, 21), np.int64)
    for p in range(2):
        for i in range(2):
            conf[p, i, 0, 0], conf[p, i, 3, 3], conf[p, i, 3, 0], conf[p, i, 0, 3] = 50, 10 + 20 * p + 5 * i, 30 - 20 * p - 5 * i, 4
            void[p, i, 3] = 2
    out = T.report(conf, void, axes, (10.0, 8, 0.25))
    lines = capsys.readouterr().out.strip().split("\n")
    s = evaluation.sem_seg_scores(conf[1, 0], void[1, 0])
    assert lines[0] == "%s %s" % (s["fp"][0], s["fn"][0])
    assert lines[1] == "%s %s" % (evaluation.mean(s["fp"][1:]), evaluation.mean(s["fn"][1:]))
    assert lines[2].startswith("{'iou': array(") and "'miou'" in " ".join(lines)
    tail = [l for l in lines if l.startswith(("beta ", "best "))]
    miou = {k: evaluation.nanmean(evaluation.sem_seg_scores(conf[p, i], void[p, i])["iou"])
            for p, b in enumerate((6.0, 10.0)) for i, t in enumerate((0.25, 0.4)) for k in [(b, 8, t)]}
    assert tail == ["beta %g exp_times %d thres %g miou %.6f" % (k + (m,)) for k, m in miou.items()] + \
        ["best beta 10 exp_times 8 thres 0.4 miou %.6f" % miou[(10.0, 8, 0.4)]]
    assert out["best"] == (10.0, 8, 0.4) and out["grid"] == miou and set(out["ious"]) == set(miou)
    assert np.array_equal(out["iou"], s["iou"], equal_nan=True) and out["miou"] == miou[(10.0, 8, 0.25)]
    assert np.array_equal(out["ious"][(6.0, 8, 0.4)], evaluation.sem_seg_scores(conf[0, 1], void[0, 1])["iou"], equal_nan=True)


def _main(tmp_path, extra):
    import _steps
    return _steps.run_sample_main(["--voc12_root", str(tmp_path), "--log_name", str(tmp_path / "log"), "--cam_out_dir", str(tmp_path / "cam"),
                                   "--sem_seg_out_dir", str(tmp_path / "sem"), "--ins_seg_out_dir", str(tmp_path / "ins"),
                                   "--make_cam_pass", "False", "--make_ins_seg_pass", "False", "--make_sem_seg_pass", "False"] + extra)


def test_command_line(tmp_path, monkeypatch):
    import run_sample
    p = run_sample.build_parser()
    a = p.parse_args(["--voc12_root", "x"])
    assert a.tune_sem_seg_pass is False and a.tune_beta == [] and a.tune_exp_times == [] and a.tune_bg_thres == []
    assert "tune_sem_seg_pass" not in run_sample.OUT_OF_SCOPE
    a = p.parse_args(["--voc12_root", "x", "--tune_sem_seg_pass", "True", "--tune_beta", "6", "14", "--tune_exp_times", "5",
                      "--tune_bg_thres", "0.1", "0.4"])
    assert a.tune_sem_seg_pass is True and a.tune_beta == [6.0, 14.0] and a.tune_exp_times == [5] and a.tune_bg_thres == [0.1, 0.4]
    assert (a.beta, a.exp_times, a.sem_seg_bg_thres) == (10, 8, 0.25)           # the defaults are unchanged
    p.format_help()
    # without the flag: the step is neither imported nor run
    import irn_amd.step
    monkeypatch.delitem(sys.modules, "irn_amd.step.tune_sem_seg", raising=False)
    monkeypatch.delattr(irn_amd.step, "tune_sem_seg", raising=False)
    assert _main(tmp_path, []) == {}
    assert "irn_amd.step.tune_sem_seg" not in sys.modules and not hasattr(irn_amd.step, "tune_sem_seg")
    # with it: the step runs — and names what it misses (the split file, before any device work)
    with pytest.raises(FileNotFoundError, match="train.txt"):
        _main(tmp_path, ["--tune_sem_seg_pass", "True"])
    assert "irn_amd.step.tune_sem_seg" in sys.modules


def test_step_refuses_loudly_without_gpu(tmp_path, monkeypatch):
    import torch
    import run_sample
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from irn_amd.step import tune_sem_seg as T
    (tmp_path / "ImageSets" / "Segmentation").mkdir(parents=True)
    (tmp_path / "ImageSets" / "Segmentation" / "train.txt").write_text("2008_000001\n")
    args = run_sample.build_parser().parse_args(["--voc12_root", str(tmp_path)])
    with pytest.raises(RuntimeError, match="need a GPU"):
        T.run(args)
