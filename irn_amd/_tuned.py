"""What this build's speed rests on per device, and the process mode that goes with it: the device key (architecture, compute
units, HIP version), the MIOpen find databases and GEMM rank tables shipped under `irn_amd/data/`, MIOpen's per-process set-up
and the reproducible mode of the backbones.  The lowest layer of the package: the trunk (net/resnet50.py), the GEMM host side
(gemm.py), the walk (misc/indexing.py) and the steps all read it, and it imports nothing from the package at import time."""
import atexit
import contextlib
import fcntl
import os
import re
import shutil
import warnings

import torch

_PACKAGE_ROOT = os.path.dirname(os.path.abspath(__file__))


def arch_name(props, missing=""):
    """`gcnArchName` of a device's properties without its feature suffix ("gfx950:sramecc+:xnack-" -> "gfx950"); `missing` for
    properties without the attribute, "" for an empty one."""
    return str(getattr(props, "gcnArchName", missing) or "").split(":")[0]


def miopen_cache_key():
    """(architecture, compute units, HIP version) as a directory name: MIOpen's find results and the GEMM rank table are only
    valid for the chip and library build that measured them.  From the device PROPERTIES (`gcnArchName`, e.g. gfx950), not from
    the marketing name: `torch.cuda.get_device_name` is "AMD Radeon Graphics" on boxes without amdgpu.ids and EMPTY under
    rocprofv3 — a profiled run then found no shipped database and silently ran the NCHW trunk (round 5, session 6)."""
    try:
        props = torch.cuda.get_device_properties(0)
        name = "%s-cu%d" % (arch_name(props) or "unknown", int(props.multi_processor_count))
    except Exception:
        name = "unknown_device"
    return "%s-hip%s" % (name, (torch.version.hip or "none").replace("/", "_"))


def merge_miopen_db(src_dir, dst_dir):
    """Add to the MIOpen user database in `dst_dir` every entry of the one in `src_dir` that it does not have yet (the
    find database `*.ufdb.txt` and the tuning database `*.udb.txt` are text files of `problem=solvers` lines; entries
    already present — what this machine measured itself — win).  -> number of entries added.  The channels-last mode of
    the trunk relies on this: an existing user database without the shipped NHWC entries would leave those problems
    untuned, which is 2x slower than not using the layout at all."""
    added = 0
    for f in sorted(os.listdir(src_dir)):
        if not (f.endswith(".ufdb.txt") or f.endswith(".udb.txt")):
            continue
        have = set()
        dst = os.path.join(dst_dir, f)
        if os.path.exists(dst):
            with open(dst) as fh:
                have = {line.split("=", 1)[0] for line in fh if "=" in line}
        with open(os.path.join(src_dir, f)) as fh:
            new = [line if line.endswith("\n") else line + "\n" for line in fh if "=" in line and line.split("=", 1)[0] not in have]
        if new:
            with open(dst, "a") as fh:
                fh.writelines(new)
            added += len(new)
    return added


_MIOPEN_LOCKS = []           # lock files held for the life of the process


def miopen_seed_root():
    """Directory of the find databases shipped with the package (one sub-directory per device / HIP version);
    IRN_MIOPEN_SEED_DIR names another one (A/B runs of a freshly tuned database)."""
    return os.environ.get("IRN_MIOPEN_SEED_DIR") or os.path.join(_PACKAGE_ROOT, "data", "miopen")


def gemm_table_root():
    """Directory of the shipped GEMM rank tables (`<arch>-cu<N>-hip<v>.json`, written by tools/conv1x1_tune.py)."""
    return os.path.join(_PACKAGE_ROOT, "data", "gemm")


def shipped_data_report():
    """What this build ships for THIS device / HIP version: {"key", "mode_key", "miopen" (is there a find database for
    the mode key), "miopen_keys" (the ones shipped), "gemm", "gemm_keys"}.  The tuned database and the rank table are this
    build's additions (all the reference says about solvers is `cudnn.enabled = True`, step/make_cam.py:14), so their
    absence is this build's to report."""
    def listing(root, strip=""):
        try:
            return sorted(f[:len(f) - len(strip)] if strip and f.endswith(strip) else f for f in os.listdir(root)
                          if not f.startswith("."))
        except OSError:
            return []
    key, mode_key = miopen_cache_key(), miopen_mode_key()
    mi_keys, ge_keys = listing(miopen_seed_root()), listing(gemm_table_root(), ".json")
    return {"key": key, "mode_key": mode_key, "miopen": mode_key in mi_keys and os.environ.get("IRN_MIOPEN_SEED", "1") != "0",
            "miopen_keys": mi_keys, "gemm": key in ge_keys and os.environ.get("IRN_GEMM_TABLE", "1") != "0", "gemm_keys": ge_keys}


_WARNED = set()


def warn_missing_shipped_data():
    """One `warnings.warn` per process and kind when the find database or the GEMM rank table for this (architecture, CU
    count, HIP version) is not shipped: the steps still run and still give the reference's results, ~10-20 % slower (NCHW
    trunk without the fused 1x1 GEMMs; hipBLASLt's first heuristic pick instead of the measured one) — a cliff that used to
    be silent.  -> the report."""
    rep = shipped_data_report()
    if rep["key"].startswith("unknown_device"):          # no GPU in this process (CPU tests, tooling): nothing runs slower
        return rep
    if not rep["miopen"] and "miopen" not in _WARNED:
        _WARNED.add("miopen")
        warnings.warn("irn_amd: no tuned MIOpen find database for '%s' under %s (shipped: %s): every trunk pass runs NCHW without "
                      "the fused 1x1 GEMMs, ~0.8x the throughput of the tuned channels-last trunk.  Remedy, on a box with this "
                      "GPU: python tools/miopen_warmup.py --channels-last 1, then python tools/miopen_det_filter.py (the "
                      "reproducible mode's '-det' database)." % (rep["mode_key"], miopen_seed_root(), ", ".join(rep["miopen_keys"]) or "none"),
                      RuntimeWarning, stacklevel=2)
    if not rep["gemm"] and "gemm" not in _WARNED:
        _WARNED.add("gemm")
        warnings.warn("irn_amd: no GEMM rank table for '%s' under %s (shipped: %s): the 1x1 convolutions use hipBLASLt's first "
                      "heuristic pick for every problem.  Remedy, on a box with this GPU: python tools/conv1x1_tune.py."
                      % (rep["key"], gemm_table_root(), ", ".join(rep["gemm_keys"]) or "none"), RuntimeWarning, stacklevel=2)
    return rep


def deterministic_backbones():
    """IRN_DETERMINISTIC (default 1; run_sample.py --deterministic 0/1): the backbones' outputs are a function of their inputs
    only, whichever process, worker layout or run computes them — an N-GPU run writes bit for bit the files of a 1-GPU run
    (reference step/make_cam.py:67-74: any `n_gpus` must give the same files).  How (net/resnet50.channels_last_for):
      * input shapes the shipped database is tuned for run the channels-last trunk (fused GEMMs) on `<key>-det`, the tuned
        database WITHOUT the one order-dependent kind of kernel in it — MIOpen's NHWC implicit GEMM with a configuration that
        splits K across workgroups and adds with atomics (tools/miopen_det_filter.py: 86 of 264 records fall to the
        composable-kernel convolution); measured bit-identical across repeats and processes for every layer of CAM and IRNet
        at 8 pairs, `cam` 114.5 against 117.4 images/s (profiles/r05_s11_deterministic_database.txt);
      * every other convolution (untuned sizes, partial batches, the heads) runs under MIOpen's deterministic attribute
        (`torch.backends.cudnn.deterministic`) in NCHW — the attribute alone leaves no fast NHWC fp32 solver
        (profiles/r05_s3_deterministic_ab.txt), which is why the tuned shapes do not use it.
    IRN_DETERMINISTIC=0: the last 2.5 %, with split-K accumulations that move the CAMs by ~1e-5 from run to run (labels then
    differ only at exact ties; tests prove each).  The mode belongs to the PROCESS: it is fixed before the first convolution
    (MIOpen keeps the solver it resolved for a problem, whatever the attribute says later)."""
    return os.environ.get("IRN_DETERMINISTIC", "1") != "0"


def miopen_mode_key():
    """Directory name of the databases of this process's mode: `<arch>-cu<N>-hip<v>` or, reproducible mode, `…-det`."""
    return miopen_cache_key() + ("-det" if deterministic_backbones() else "")


def apply_deterministic_setting():
    """Hand the mode to the trunk (net/resnet50.DETERMINISTIC) and put PyTorch's process-wide flag in the mode's resting
    state: on in the reproducible mode (the trunk switches it off for the duration of a channels-last pass on the filtered
    database), off otherwise."""
    from .net import resnet50 as _r50
    det = deterministic_backbones()
    _r50.DETERMINISTIC = det
    torch.backends.cudnn.deterministic = det


def miopen_setup(device_ordinal):
    """MIOpen's settings for the process that is about to run the backbones on `device_ordinal` — the SAME for a pool
    worker and for the in-process single-GPU path, so that one-GPU and N-GPU runs pick their convolution solvers the
    same way: find mode 2 ("fast": the find database first, the immediate-mode heuristic on a miss)
    unless the user chose one, and a user database directory that is
      * stable across runs — `$IRN_MIOPEN_CACHE` or `~/.cache/irn_amd/miopen`, / (device name, HIP version) / dev<ordinal>
        — so that what one run's workers found the next run's workers reuse (each worker process used to start with
        a cold database named after its rank);
      * completed from the database shipped with the package for this (device, HIP) pair (`irn_amd/data/miopen/<key>/`,
        written on a GPU box by `tools/miopen_warmup.py`): every shipped entry the user database lacks is added
        (`merge_miopen_db`), what this machine measured itself is kept — the trunk's channels-last layout, chosen per
        input shape (net/resnet50.py), depends on the shipped NHWC entries being there;
      * never shared by two live processes: the directory is claimed with an advisory lock, and a process that finds
        it taken (a second job on the same host and GPU) works on a private copy `dev<ordinal>-pid<pid>` instead
        (eight workers appending to one database collided in round 2).
    A `MIOPEN_USER_DB_PATH` the user exported is respected as the base.  Must run before the process's first
    convolution; returns the directory."""
    os.environ.setdefault("MIOPEN_FIND_MODE", "2")
    apply_deterministic_setting()
    warn_missing_shipped_data()
    marker = os.environ.get("IRN_MIOPEN_DB_SET")
    if marker and os.environ.get("MIOPEN_USER_DB_PATH") == marker and os.environ.get("IRN_MIOPEN_DB_DEV", str(int(device_ordinal))) == str(int(device_ordinal)):
        return marker                                    # this process (or the parent it inherited from, if it holds no lock itself) did it, for this device
    # (IRN_MIOPEN_BASE: the base the first caller of this job resolved — a worker must not take its parent's claimed
    # directory, which it inherits in MIOPEN_USER_DB_PATH, for the user's base)
    base = os.environ.get("IRN_MIOPEN_BASE") or os.environ.get("IRN_MIOPEN_CACHE") or os.environ.get("MIOPEN_USER_DB_PATH") or \
        os.path.join(os.path.expanduser("~"), ".cache", "irn_amd", "miopen")
    os.environ["IRN_MIOPEN_BASE"] = base
    key = miopen_mode_key()
    stable = os.path.join(base, key, "dev%d" % int(device_ordinal))
    os.makedirs(stable, exist_ok=True)
    use = stable
    try:
        fh = open(os.path.join(stable, ".lock"), "w")
        fcntl.flock(fh, fcntl.LOCK_EX | fcntl.LOCK_NB)
        _MIOPEN_LOCKS.append(fh)
    except OSError:                                      # another live process owns it: private copy
        use = os.path.join(base, key, "dev%d-pid%d" % (int(device_ordinal), os.getpid()))
        os.makedirs(use, exist_ok=True)
        for f in os.listdir(stable):
            if f != ".lock" and os.path.isfile(os.path.join(stable, f)):
                shutil.copy2(os.path.join(stable, f), os.path.join(use, f))
        atexit.register(shutil.rmtree, use, True)           # (a pool worker is terminated, not exited: WorkerPool.close() cleans up then)
    seed = os.path.join(miopen_seed_root(), key)
    if os.environ.get("IRN_MIOPEN_SEED", "1") != "0" and os.path.isdir(seed):
        merge_miopen_db(seed, use)         # (after the claim: nobody else appends to `use` now)
    os.environ["MIOPEN_USER_DB_PATH"] = use
    os.environ["IRN_MIOPEN_DB_SET"] = use
    os.environ["IRN_MIOPEN_DB_DEV"] = str(int(device_ordinal))
    return use


def reap_private_miopen_dbs(pids):
    """Private database copies (`dev<N>-pid<pid>`) of worker processes that are gone: what they found is merged back into the
    stable per-device directory (entries it lacks), the copy is removed.  Called by WorkerPool.close() — a terminated daemon
    process never runs its atexit handlers."""
    base = os.environ.get("IRN_MIOPEN_BASE")
    if not base:
        return 0
    root = os.path.join(base, miopen_mode_key())
    n = 0
    try:
        entries = os.listdir(root)
    except OSError:
        return 0
    for d in entries:
        m = re.match(r"^(dev\d+)-pid(\d+)$", d)
        if not m or int(m.group(2)) not in pids:
            continue
        src, stable = os.path.join(root, d), os.path.join(root, m.group(1))
        try:
            if os.path.isdir(stable):
                merge_miopen_db(src, stable)
            shutil.rmtree(src, ignore_errors=True)
            n += 1
        except OSError:
            pass
    return n


@contextlib.contextmanager
def process_mode(device=None, fused_tail=None):
    """The mode for the length of a block that runs in the CALLER's process (a step without a second process, a training or
    tuning step, a benchmark): the caller's own `torch.backends.cudnn.deterministic` and the trunk's DETERMINISTIC and
    TRAIN_FUSED_TAIL are put back however the block ends.  With a `device`, `miopen_setup(device)` — the MIOpen settings a
    pool worker runs with — and the block gets the database directory; without one only `apply_deterministic_setting()`
    (MIOpen is left as the caller has it) and the block gets None.  `fused_tail` sets TRAIN_FUSED_TAIL.  Enter it before
    the model is built or a convolution runs: MIOpen keeps the solver it resolved for a problem."""
    from .net import resnet50 as _r50
    saved = (torch.backends.cudnn.deterministic, _r50.DETERMINISTIC, _r50.TRAIN_FUSED_TAIL)
    try:
        db_dir = None
        if device is None:
            apply_deterministic_setting()
        else:
            db_dir = miopen_setup(device)
        if fused_tail is not None:
            _r50.TRAIN_FUSED_TAIL = bool(fused_tail)
        yield db_dir
    finally:
        torch.backends.cudnn.deterministic, _r50.DETERMINISTIC, _r50.TRAIN_FUSED_TAIL = saved
