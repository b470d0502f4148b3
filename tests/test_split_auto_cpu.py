"""`--split_gemm auto` without a GPU: the command line and the module switches, the redo bookkeeping as a pure function of
the flag words, the report line, the worker counter (run_sample.py, net/resnet50.set_split_mode, step/_split_auto.py,
step/_report.py)."""
import os

import numpy as np
import pytest


@pytest.fixture
def split_state(monkeypatch):
    """Whatever a test sets through `set_split_mode` is put back: the environment variable and both module switches."""
    from irn_amd.net import resnet50 as r50
    monkeypatch.setattr(r50, "SPLIT_GEMM", r50.SPLIT_GEMM)
    monkeypatch.setattr(r50, "SPLIT_AUTO", r50.SPLIT_AUTO)
    monkeypatch.setenv("IRN_SPLIT_GEMM", os.environ.get("IRN_SPLIT_GEMM", "1"))
    return r50


@pytest.mark.parametrize("value,parsed,env,split,auto", [("0", 0, "0", False, False), ("1", 1, "1", True, False),
                                                         ("auto", "auto", "auto", True, True), ("AUTO", "auto", "auto", True, True)])
def test_the_parser_takes_0_1_and_auto_and_sets_the_switches(split_state, value, parsed, env, split, auto):
    import run_sample
    from irn_amd.step import _split_auto
    r50 = split_state
    args = run_sample.build_parser().parse_args(["--voc12_root", "x", "--split_gemm", value])
    assert args.split_gemm == parsed and type(args.split_gemm) is type(parsed)
    run_sample.apply_split_gemm(args)
    assert os.environ["IRN_SPLIT_GEMM"] == env and r50.SPLIT_GEMM is split and r50.SPLIT_AUTO is auto
    assert _split_auto.enabled() is auto
    # a command whose steps keep the end-of-step check runs "auto" as 1
    run_sample.apply_split_gemm(args, auto=False)
    assert os.environ["IRN_SPLIT_GEMM"] == ("1" if auto else env) and r50.SPLIT_GEMM is split and r50.SPLIT_AUTO is False


def test_the_parser_leaves_the_environment_alone_and_refuses_other_values(split_state):
    import run_sample
    r50 = split_state
    before = (os.environ["IRN_SPLIT_GEMM"], r50.SPLIT_GEMM, r50.SPLIT_AUTO)
    args = run_sample.build_parser().parse_args(["--voc12_root", "x"])
    assert args.split_gemm is None
    run_sample.apply_split_gemm(args)
    assert (os.environ["IRN_SPLIT_GEMM"], r50.SPLIT_GEMM, r50.SPLIT_AUTO) == before
    for bad in ("2", "on", ""):
        with pytest.raises(SystemExit):
            run_sample.build_parser().parse_args(["--voc12_root", "x", "--split_gemm", bad])
    with pytest.raises(ValueError):
        r50.set_split_mode("2")
    assert "auto" in run_sample.build_parser().format_help()


def test_fp32_gemms_puts_the_switch_back_also_after_an_exception(split_state):
    r50 = split_state
    r50.set_split_mode("auto")
    with r50.fp32_gemms():
        assert r50.SPLIT_GEMM is False and r50.SPLIT_AUTO is True
    assert r50.SPLIT_GEMM is True
    with pytest.raises(KeyError):
        with r50.fp32_gemms():
            raise KeyError("x")
    assert r50.SPLIT_GEMM is True
    r50.set_split_mode("0")
    with r50.fp32_gemms():
        pass
    assert r50.SPLIT_GEMM is False


def test_redo_names_from_the_flag_words():
    """flags [n_scales, 2 n_images], rows as [image, flip, image, flip, ...]: an image is redone when its own row or its flip's
    has a word set at any scale — and only then."""
    from irn_amd.step._split_auto import redo_names
    names = ["a", "b", "c", "d"]
    f = np.zeros((4, 8), np.int32)
    assert redo_names(f, names) == []
    f[2, 3] = 1                     # the flip of b, third scale
    assert redo_names(f, names) == ["b"]
    f[0, 6] = 1                     # d itself, first scale
    f[3, 0] = 5                     # any bit counts
    assert redo_names(f, names) == ["a", "b", "d"]
    assert redo_names(f[0], names) == ["d"]                     # one pass: a vector of words
    assert redo_names(np.ones((2, 8), np.uint32), names) == names
    assert redo_names(np.zeros((3, 0), np.int32), []) == []
    with pytest.raises(ValueError):
        redo_names(np.zeros((4, 7), np.int32), names)


def test_the_redo_list_keeps_one_entry_per_image():
    from irn_amd.step._split_auto import Redo
    r = Redo()
    assert len(r) == 0 and r.items() == []
    r.add("b", (3, 4))
    r.add("a")
    r.add("b", (9, 9))               # the second flush that names it changes nothing
    assert len(r) == 2 and sorted(r.items()) == [("a", None), ("b", (3, 4))]


def test_the_report_line_and_the_counter(monkeypatch):
    from irn_amd.step import _pool, _report, _split_auto
    assert _report.split_fallback_line([]) == ""
    line = _report.split_fallback_line(["2008_000001"])
    assert "1 image(s)" in line and line.endswith(": 2008_000001") and "fp32" in line and "\n" not in line
    many = ["n%02d" % i for i in range(11)]
    line = _report.split_fallback_line(many)
    assert "11 image(s)" in line and ", ".join(many[:8]) in line and "n08" not in line and line.endswith("... (3 more)")

    said = []
    monkeypatch.setattr(_report, "say", said.append)
    monkeypatch.setitem(_report.SPLIT_STATS, "fallback_images", 0)
    assert _report.worker_stats()["split_fallback_images"] == 0
    r = _split_auto.Redo()
    r.report(3)
    assert said == [] and _report.worker_stats()["split_fallback_images"] == 0          # nothing to say at 0
    r.add("x"), r.add("y")
    r.report(3)
    assert len(said) == 1 and said[0].startswith("[worker 3] ") and "2 image(s)" in said[0] and said[0].endswith(": x, y")
    assert _report.worker_stats()["split_fallback_images"] == 2
    assert _pool.pool_stats() == [] or all(isinstance(s, dict) for s in _pool.pool_stats())
