"""`irn_amd._tuned`: the device key, the shipped MIOpen databases and GEMM tables, MIOpen's set-up; the lowest layer of the
package (nothing of the package is imported with it); and `process_mode`, the one statement of "this is the caller's
process: apply the mode, hand everything back".  No GPU."""
import os
import subprocess
import sys

import pytest
import torch

from irn_amd import _tuned
from irn_amd.net import resnet50 as r50

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIOPEN_ENV = ("IRN_MIOPEN_DB_SET", "IRN_MIOPEN_DB_DEV", "IRN_MIOPEN_BASE", "MIOPEN_USER_DB_PATH", "MIOPEN_FIND_MODE")


def _state():
    return (torch.backends.cudnn.deterministic, r50.DETERMINISTIC, r50.TRAIN_FUSED_TAIL)


@pytest.mark.parametrize("env,before,fused_tail,inside", [
    # (IRN_DETERMINISTIC, what the caller had, the argument, what the block must see): never what the mode would choose
    ("1", (False, None, True), 0, (True, True, False)),
    ("1", (False, False, False), 1, (True, True, True)),
    ("0", (True, True, True), None, (False, False, True)),          # fused_tail=None leaves TRAIN_FUSED_TAIL alone
])
def test_process_mode_applies_the_mode_and_hands_the_process_back(monkeypatch, env, before, fused_tail, inside):
    monkeypatch.setenv("IRN_DETERMINISTIC", env)
    for k in MIOPEN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", "/the/callers/own")
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", before[0])
    monkeypatch.setattr(r50, "DETERMINISTIC", before[1])
    monkeypatch.setattr(r50, "TRAIN_FUSED_TAIL", before[2])
    with _tuned.process_mode(fused_tail=fused_tail) as db_dir:
        assert db_dir is None and _state() == inside
    assert _state() == before
    boom = RuntimeError("the step failed")
    with pytest.raises(RuntimeError) as info:
        with _tuned.process_mode(fused_tail=fused_tail):
            assert _state() == inside
            r50.TRAIN_FUSED_TAIL = "left behind by the block"
            raise boom
    assert info.value is boom and _state() == before
    # without a device MIOpen is the caller's: no database claimed, no find mode chosen
    assert os.environ["MIOPEN_USER_DB_PATH"] == "/the/callers/own"
    assert not [k for k in MIOPEN_ENV if k != "MIOPEN_USER_DB_PATH" and k in os.environ]


def test_process_mode_with_a_device_sets_miopen_up_and_yields_the_database(monkeypatch, tmp_path):
    for k in MIOPEN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("IRN_MIOPEN_CACHE", str(tmp_path))
    monkeypatch.setenv("IRN_DETERMINISTIC", "1")
    monkeypatch.setattr(_tuned, "_MIOPEN_LOCKS", [])
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    monkeypatch.setattr(r50, "DETERMINISTIC", None)
    before = _state()
    with _tuned.process_mode(2) as db_dir:
        assert db_dir == os.path.join(str(tmp_path), _tuned.miopen_mode_key(), "dev2") == os.environ["MIOPEN_USER_DB_PATH"]
        assert os.environ["MIOPEN_FIND_MODE"] == "2" and _state()[:2] == (True, True)
    assert _state() == before


def test_tuned_imports_nothing_of_the_package():
    """The trunk, the GEMM host side and the walk import `_tuned` at their top: it must not import them, or the step layer."""
    code = ("import sys; sys.path.insert(0, %r); import irn_amd._tuned; "
            "print(sorted(m for m in sys.modules if m.startswith('irn_amd')))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-1500:]
    loaded = eval(out.stdout.strip().splitlines()[-1])
    assert "irn_amd.step._common" not in loaded and "irn_amd.net.resnet50" not in loaded
    assert loaded == ["irn_amd", "irn_amd._tuned"]


def test_miopen_setup_is_stable_seeded_and_exclusive(tmp_path, monkeypatch):
    """One MIOpen user database per (device, HIP version, device ordinal), stable across runs, seeded from the package's
    shipped database when empty, and never shared by two live processes (a second claimant gets a private copy)."""
    import subprocess
    import sys
    from irn_amd import _tuned
    from irn_amd.step import _common
    for k in ("IRN_MIOPEN_DB_SET", "IRN_MIOPEN_BASE", "MIOPEN_USER_DB_PATH", "MIOPEN_FIND_MODE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("IRN_MIOPEN_CACHE", str(tmp_path))
    monkeypatch.setattr(_tuned, "_MIOPEN_LOCKS", [])
    monkeypatch.delenv("IRN_DETERMINISTIC", raising=False)
    d0 = _common.miopen_setup(0)
    key = _common.miopen_mode_key()
    assert key == _common.miopen_cache_key() + "-det"             # the reproducible mode is the default and has its own databases
    import torch
    from irn_amd.net import resnet50 as r50
    assert r50.DETERMINISTIC is True and torch.backends.cudnn.deterministic is True
    assert d0 == os.path.join(str(tmp_path), key, "dev0") and os.environ["MIOPEN_USER_DB_PATH"] == d0
    assert os.environ["MIOPEN_FIND_MODE"] == "2" and _common.miopen_setup(0) == d0
    open(os.path.join(d0, "gfx950_256.ufdb.txt"), "w").write("found")
    # a second live process on the same device: private copy of what the first one has, removed when it exits
    code = ("import os, sys; sys.path.insert(0, %r); from irn_amd.step import _common; d = _common.miopen_setup(0); "
            "print(d); print(sorted(os.listdir(d)))" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    env = {k: v for k, v in os.environ.items() if k not in ("IRN_MIOPEN_DB_SET",)}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-1500:]
    d1, files = out.stdout.strip().splitlines()[-2:]
    assert d1 == os.path.join(str(tmp_path), key, "dev0-pid%s" % d1.rsplit("pid", 1)[1]) and "gfx950_256.ufdb.txt" in files
    assert not os.path.exists(d1)
    # another ordinal is another directory; a user-chosen find mode survives
    monkeypatch.delenv("IRN_MIOPEN_DB_SET")
    monkeypatch.setenv("MIOPEN_FIND_MODE", "1")
    assert _common.miopen_setup(3).endswith(os.path.join(key, "dev3")) and os.environ["MIOPEN_FIND_MODE"] == "1"
    # the fast mode: its own key, PyTorch's flag off
    monkeypatch.delenv("IRN_MIOPEN_DB_SET")
    monkeypatch.setenv("IRN_DETERMINISTIC", "0")
    assert _common.miopen_setup(3).endswith(os.path.join(_common.miopen_cache_key(), "dev3"))
    assert r50.DETERMINISTIC is False and torch.backends.cudnn.deterministic is False
    monkeypatch.setattr(r50, "DETERMINISTIC", None)


def test_det_database_is_the_tuned_one_minus_the_split_k_implicit_gemms():
    """irn_amd/data/miopen/<key>-det (tools/miopen_det_filter.py): same problems, same channels-last shape list; the NHWC
    implicit-GEMM solver is gone from exactly the forward records whose tuned configuration splits K, another fast solver
    remains in every one of them, nothing else changed."""
    import glob
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "irn_amd", "data", "miopen")
    fast = sorted(d for d in glob.glob(os.path.join(root, "*")) if os.path.isdir(d) and not d.endswith("-det"))
    assert fast
    for src in fast:
        dst = src + "-det"
        assert os.path.isdir(dst), "run tools/miopen_det_filter.py"
        assert open(os.path.join(src, "nhwc_shapes.json")).read() == open(os.path.join(dst, "nhwc_shapes.json")).read()
        rec = lambda d: dict(l.rstrip("\n").split("=", 1) for l in open(glob.glob(os.path.join(d, "*.ufdb.txt"))[0]) if "=" in l)
        a, b = rec(src), rec(dst)
        assert a.keys() == b.keys()
        gtc = "ConvAsmImplicitGemmGTCDynamicFwdXdlopsNHWC:"
        changed = [k for k in a if a[k] != b[k]]
        assert changed and all("NHWC" in k and k.endswith("-F") for k in changed)
        for k in changed:
            ents_a, ents_b = a[k].split(";"), b[k].split(";")
            assert [e for e in ents_a if not e.startswith(gtc)] == ents_b
            assert any(not e.startswith("ConvDirectNaive") for e in ents_b), k


def test_merge_miopen_db_adds_missing_entries_only(tmp_path):
    """The shipped find database completes a user database: entries the user database lacks are appended, entries it has
    (what this machine measured) are kept, other files are left alone."""
    from irn_amd.step import _common
    src, dst = tmp_path / "src", tmp_path / "dst"
    src.mkdir()
    dst.mkdir()
    (src / "gfx.ufdb.txt").write_text("a-NCHW=solverA:1\nb-NHWC-NHWC-NHWC=solverB:2\n")
    (src / "gfx.udb.txt").write_text("p=1,2,3")
    (src / "nhwc_shapes.json").write_text("[[16, 512, 512]]")
    (dst / "gfx.ufdb.txt").write_text("a-NCHW=mine:0.5\n")
    assert _common.merge_miopen_db(str(src), str(dst)) == 2
    assert (dst / "gfx.ufdb.txt").read_text() == "a-NCHW=mine:0.5\nb-NHWC-NHWC-NHWC=solverB:2\n"
    assert (dst / "gfx.udb.txt").read_text() == "p=1,2,3\n" and not (dst / "nhwc_shapes.json").exists()
    assert _common.merge_miopen_db(str(src), str(dst)) == 0


def test_missing_shipped_data_warns_once_and_names_the_remedy(monkeypatch, tmp_path):
    """the tuned find database and the GEMM rank table exist for one (architecture, CU count, HIP
    version) key; on any other box the steps ran ~10 % slower without a word.  Now one RuntimeWarning per process and kind
    names the key looked for, the keys shipped and the tool that writes the data; the per-step summary lists the sizes
    whose trunk passes fell to NCHW."""
    import warnings
    from irn_amd import _tuned
    from irn_amd.step import _common
    from irn_amd.net import resnet50 as r50
    monkeypatch.setattr(_tuned, "miopen_cache_key", lambda: "gfx999-cu1-hip0.0")
    monkeypatch.setattr(_tuned, "_WARNED", set())
    monkeypatch.delenv("IRN_DETERMINISTIC", raising=False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rep = _common.warn_missing_shipped_data()
        _common.warn_missing_shipped_data()                                    # once per process
    assert rep["miopen"] is False and rep["gemm"] is False and rep["mode_key"] == "gfx999-cu1-hip0.0-det"
    msgs = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
    assert len(msgs) == 2
    mi = [m for m in msgs if "MIOpen" in m][0]
    ge = [m for m in msgs if "GEMM rank table" in m][0]
    assert "gfx999-cu1-hip0.0-det" in mi and "gfx950-cu256-hip7.0.51831-det" in mi and "tools/miopen_warmup.py" in mi and "miopen_det_filter" in mi
    assert "gfx999-cu1-hip0.0" in ge and "gfx950-cu256-hip7.0.51831" in ge and "tools/conv1x1_tune.py" in ge
    # the shipped key itself: nothing to say
    monkeypatch.setattr(_tuned, "miopen_cache_key", lambda: "gfx950-cu256-hip7.0.51831")
    monkeypatch.setattr(_tuned, "_WARNED", set())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rep = _common.warn_missing_shipped_data()
    assert rep["miopen"] and rep["gemm"] and not [x for x in w if issubclass(x.category, RuntimeWarning)]
    # miopen_setup is where every worker / rank / in-process step passes: it warns too
    monkeypatch.setattr(_tuned, "miopen_cache_key", lambda: "gfx999-cu1-hip0.0")
    monkeypatch.setattr(_tuned, "_WARNED", set())
    monkeypatch.setattr(_tuned, "_MIOPEN_LOCKS", [])
    for k in ("IRN_MIOPEN_DB_SET", "IRN_MIOPEN_BASE", "MIOPEN_USER_DB_PATH"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("IRN_MIOPEN_CACHE", str(tmp_path))
    saved = (torch.backends.cudnn.deterministic, r50.DETERMINISTIC)
    try:
        with pytest.warns(RuntimeWarning, match="no tuned MIOpen find database for 'gfx999-cu1-hip0.0-det'"):
            _common.miopen_setup(0)
    finally:
        torch.backends.cudnn.deterministic, r50.DETERMINISTIC = saved
    # step summary: NCHW passes by size, then reset
    monkeypatch.setattr(r50, "PASS_STATS", {"channels_last": 5, "nchw": 3, "pad_rows": 4, "nchw_sizes": {"281x500": 2, "96x112": 1}})
    line = _common.untuned_report()
    assert "3 of 8 trunk passes ran NCHW" in line and "281x500 x2" in line and "96x112 x1" in line and "4 zero rows" in line
    assert _common.untuned_report() == "" and r50.PASS_STATS["nchw"] == 0
    line = _common.startup_line(3, 8, 0, "/db")
    assert "worker 3/8" in line and "NOT SHIPPED" in line and "reproducible" in line


def test_rank_table_is_read_once_and_a_malformed_one_raises_with_its_path(monkeypatch, tmp_path):
    """irn_amd/gemm.py: the three rank dicts come from ONE read of `<gemm_table_root>/<key>.json`; no file or IRN_GEMM_TABLE=0 mean
    empty tables; a file that is there but is not JSON, or holds a key or a rank that is no integer, raises and names the file (a
    shipped table that silently does nothing costs ~10 % and nobody sees it)."""
    import json
    from irn_amd import gemm, ops
    from irn_amd import _tuned
    monkeypatch.setattr(_tuned, "gemm_table_root", lambda: str(tmp_path))
    monkeypatch.setattr(_tuned, "miopen_cache_key", lambda: "gfx999-cu1-hip0.0")
    monkeypatch.delenv("IRN_GEMM_TABLE", raising=False)
    path = tmp_path / "gfx999-cu1-hip0.0.json"
    monkeypatch.setattr(gemm, "_TABLE", None)
    assert gemm.gemm_ranks() == {} and gemm.gemm_ranks16() == {} and gemm.gemm_ranks3x3() == {}          # no file
    path.write_text(json.dumps({"ranks": {"4096,256,64,1,0,1": 3}, "ranks16": {"4096,768,64,1,0,1": 2}, "ranks3x3": {"1156,128,128": 5}}))
    assert gemm.gemm_ranks() == {}                                                                       # ... and not looked for again
    monkeypatch.setattr(gemm, "_TABLE", None)
    opened = []
    real_load = json.load
    monkeypatch.setattr(json, "load", lambda fh: opened.append(fh.name) or real_load(fh))
    assert ops.gemm_ranks() == {(4096, 256, 64, 1, 0, 1): 3} and ops.gemm_ranks16() == {(4096, 768, 64, 1, 0, 1): 2}
    assert ops.gemm_ranks3x3() == {(1156, 128, 128): 5} and opened == [str(path)]
    monkeypatch.setattr(gemm, "_TABLE", None)
    monkeypatch.setenv("IRN_GEMM_TABLE", "0")
    assert gemm.gemm_ranks() == {} and gemm.gemm_ranks3x3() == {} and opened == [str(path)]
    monkeypatch.delenv("IRN_GEMM_TABLE")
    for text in ("{\"ranks\": {", "[1, 2]", json.dumps({"ranks": {"4096,256,sixty-four,1,0,1": 3}}), json.dumps({"ranks": {"4096,256,64,1,0,1": 3}, "ranks16": {"8,8,8,0,0,0": 1.5}}),
                 json.dumps({"ranks3x3": {"1156,128,128": "5"}}), json.dumps({"ranks": [3]})):
        path.write_text(text)
        for accessor in (gemm.gemm_ranks, gemm.gemm_ranks16, gemm.gemm_ranks3x3):
            monkeypatch.setattr(gemm, "_TABLE", None)
            with pytest.raises(ValueError) as e:
                accessor()
            assert str(path) in str(e.value) and "malformed" in str(e.value), text
    monkeypatch.setattr(gemm, "_TABLE", None)           # (the next reader of this process loads the real one)


def test_device_key_comes_from_the_architecture_not_the_marketing_name(monkeypatch):
    """`torch.cuda.get_device_name` is empty under rocprofv3 and generic without amdgpu.ids: the key of the shipped databases
    (MIOpen find database, GEMM rank table) is built from gcnArchName + CU count + HIP version."""
    import types
    import torch
    from irn_amd.step import _common
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda i: types.SimpleNamespace(gcnArchName="gfx950:sramecc+:xnack-", multi_processor_count=256))
    monkeypatch.setattr(torch.cuda, "get_device_name", lambda i=0: "")
    key = _common.miopen_cache_key()
    assert key.startswith("gfx950-cu256-hip") and " " not in key
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "irn_amd", "data")
    shipped = os.listdir(os.path.join(root, "miopen"))
    assert any(d.startswith("gfx950-cu256-hip") for d in shipped), shipped
    assert any(f.startswith("gfx950-cu256-hip") and f.endswith(".json") for f in os.listdir(os.path.join(root, "gemm")))
