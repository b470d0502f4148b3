"""One worker process per GPU over strided shards (reference step/make_cam.py:67-74), fail-fast, no communication between
workers.

Unlike the reference, which forks a fresh set of workers inside every `run(args)` (`multiprocessing.spawn`,
step/make_cam.py:74, step/make_sem_seg_labels.py:70, step/make_ins_seg_labels.py:171), the workers here are spawned
ONCE per process and device list and serve every later step (`WorkerPool`): a HIP context, MIOpen's solver search and
the CAMs `make_cam` left in device memory (`_stores.CamStore`) survive from one step of `run_sample.py` to the next.  The step
API is unchanged: `step.X.run(args)` works on its own and returns when every shard is done."""
import atexit
import functools
import importlib
import os
import pickle
import time
import traceback
from multiprocessing.reduction import ForkingPickler

import torch
from torch import multiprocessing

from .. import _tuned
from . import _report

_NET_ALIASES = {"net.resnet50_cam": "irn_amd.net.resnet50_cam", "net.resnet50_irn": "irn_amd.net.resnet50_irn"}


def import_network(dotted):
    """`--cam_network net.resnet50_cam` style names of the reference resolve to this package."""
    return importlib.import_module(_NET_ALIASES.get(dotted, dotted))


class ModelSpec:
    """What a step hands its workers instead of a constructed network: the class and the checkpoint to build it from.
    The reference pickles the whole model into every spawned process (`spawn(args=(model, ...))`, step/make_cam.py:74);
    with persistent workers that would be ~270 shared-memory tensors (one file descriptor each) per worker and step.  A
    worker builds the network itself (`net/weights.load_checkpoint`: memory-mapped file, no random initialisation) and
    keeps it on its device for later steps that name the same checkpoint — make_sem_seg_labels and make_ins_seg_labels
    share one EdgeDisplacement."""

    def __init__(self, network, cls_name, path, strict, n_classes=None):
        """`n_classes`: the class count a network that has one (the CAM classifier) is built with; None: its default."""
        self.network, self.cls_name, self.path, self.strict = network, cls_name, os.path.abspath(path), bool(strict)
        self.n_classes = None if n_classes is None else int(n_classes)

    def key(self):
        st = os.stat(self.path)
        return (self.network, self.cls_name, self.path, self.strict, st.st_mtime_ns, st.st_size, self.n_classes)

    def build(self):
        from ..net import weights
        factory = getattr(import_network(self.network), self.cls_name)
        if self.n_classes is not None:
            factory = functools.partial(factory, n_classes=self.n_classes)
        return weights.load_checkpoint(factory, self.path, strict=self.strict)


_MODELS = {}          # per process: ModelSpec.key() -> network (on this worker's device once a step has used it)


def materialise(model):
    """The network a `_work` function computes with: `model` itself, or the one a ModelSpec describes (cached per process;
    a checkpoint file that changed on disk is a different key)."""
    if not isinstance(model, ModelSpec):
        return model
    key = model.key()
    net = _MODELS.get(key)
    if net is None:
        for k in [k for k in _MODELS if k[:3] == key[:3]]:      # an older version of the same checkpoint: let it go
            del _MODELS[k]
        net = _MODELS[key] = model.build()
    return net


def worker_devices(args=None):
    """Device ordinal of every worker process: one per visible GPU like the reference (`torch.cuda.device_count()`
    shards, step/make_cam.py:67), unless `args.worker_devices` (run_sample.py --worker_devices, or the environment
    variable IRN_WORKER_DEVICES) lists them, e.g. "0,0" = two workers sharing GPU 0 (tests of the N > 1 path on a
    one-GPU box), "0,2,4,6" = every other GPU."""
    spec = getattr(args, "worker_devices", None) if args is not None else None
    if spec is None or spec == "" or spec == []:
        spec = os.environ.get("IRN_WORKER_DEVICES")
    if spec:
        devs = [int(v) for v in (spec.split(",") if isinstance(spec, str) else spec)]
        n = torch.cuda.device_count()
        if n < 1 or any(d < 0 or d >= n for d in devs):
            raise RuntimeError("worker_devices %s: %d GPU(s) visible" % (devs, n))
        return devs
    n = torch.cuda.device_count()
    if n < 1:
        # the reference silently does nothing with zero GPUs (spawn(nprocs=0)); fail loudly instead
        raise RuntimeError("irn_amd steps need at least one GPU (torch.cuda.device_count() == 0)")
    return list(range(n))


def n_gpus_or_raise(args=None):
    """Number of shards = number of worker processes (reference: torch.cuda.device_count())."""
    return len(worker_devices(args))


_WORKER_DEVICE = [None]      # set inside a pool worker process
_POOL = [None]               # the parent's pool


def worker_device(process_id, args=None):
    """The device worker `process_id` computes on.  The reference uses the process id itself
    (`torch.cuda.device(process_id)`, step/make_cam.py:24); a pool worker was told its device at start-up."""
    if _WORKER_DEVICE[0] is not None:
        return _WORKER_DEVICE[0]
    devs = worker_devices(args)
    return devs[process_id] if process_id < len(devs) else process_id


def _pool_worker(rank, device, n_workers, cmd_q, res_q):
    """Main loop of a pool worker: bound to one device for its whole life, runs the `_work` functions the parent names."""
    try:
        _WORKER_DEVICE[0] = int(device)
        if int(device) >= 0:                  # negative ordinals: workers without a GPU (the pool's own CPU tests)
            os.environ.pop("IRN_MIOPEN_DB_SET", None)    # the parent's claim is the parent's: this process makes its own
            os.environ.pop("IRN_MIOPEN_DB_DEV", None)
            db_dir = _tuned.miopen_setup(int(device))    # stable per-device database, never shared by two live processes
            torch.cuda.set_device(int(device))
            _report.say(_report.startup_line(rank, n_workers, device, db_dir))
        res_q.put((rank, "ready", None))
        while True:
            cmd = cmd_q.get()
            if cmd is None:
                break
            res_q.put((rank, "ack", None))          # the command arrived: the parent tells "never received" from "never finished"
            try:
                mod, fn, model, shards, args = pickle.loads(cmd)
                work = getattr(importlib.import_module(mod), fn)
                work(rank, model, shards, args)
                if int(device) >= 0:
                    _report.after_step(rank, "%s.%s" % (mod, fn))
                res_q.put((rank, "ok", _report.worker_stats()))
            except BaseException:
                res_q.put((rank, "error", traceback.format_exc()))
    except BaseException:
        res_q.put((rank, "error", traceback.format_exc()))


class WorkerPool:
    """One process per entry of `devices`, spawned once and alive until `close()` (or interpreter exit)."""

    def __init__(self, devices):
        self.devices = list(devices)
        ctx = multiprocessing.get_context("spawn")       # a forked child cannot use the parent's HIP runtime
        self._res_q = ctx.Queue()
        self._cmd_qs = [ctx.Queue() for _ in self.devices]
        self._procs = []
        self.stats = [{} for _ in self.devices]
        for rank, dev in enumerate(self.devices):
            p = ctx.Process(target=_pool_worker, args=(rank, dev, len(self.devices), self._cmd_qs[rank], self._res_q), daemon=True)
            p.start()
            self._procs.append(p)
        self._collect("ready", float(os.environ.get("IRN_WORKER_START_TIMEOUT_S", "900")), "worker start-up")

    def _collect(self, want, timeout_s=0.0, what="step"):
        """Wait until every worker has answered `want`.  Fail fast on a worker's exception or death (like
        spawn(join=True)); with `timeout_s` > 0 also on a worker that is alive but silent — wedged in a GPU or RCCL call,
        stuck behind another tenant of its device: the pool is stopped and the error names the ranks that never answered
        (and whether the command had reached them)."""
        answered, acked = set(), set()
        t0 = time.monotonic()
        while len(answered) < len(self._procs):
            try:
                rank, status, payload = self._res_q.get(timeout=1.0 if timeout_s > 0 else 5.0)
            except Exception:            # queue.Empty: is everybody still alive, and inside the deadline?
                dead = [i for i, p in enumerate(self._procs) if not p.is_alive()]
                if dead:
                    codes = [self._procs[i].exitcode for i in dead]
                    self.close(force=True)
                    raise RuntimeError("step worker(s) %s died without reporting (exit codes %s)" % (dead, codes))
                if timeout_s > 0 and time.monotonic() - t0 > timeout_s:
                    silent = sorted(set(range(len(self._procs))) - answered)
                    self.close(force=True)
                    raise RuntimeError("%s: worker(s) %s (device(s) %s) did not answer within %.0f s; the command had reached %s; "
                                       "all workers were stopped" % (what, silent, [self.devices[i] for i in silent], timeout_s,
                                                                     sorted(acked & set(silent)) or "none of them"))
                continue
            if status == "error":        # fail fast like spawn(join=True): the other workers are stopped, the error surfaces
                self.close(force=True)
                raise RuntimeError("step worker %d failed:\n%s" % (rank, payload))
            if status == "ack":
                acked.add(rank)
            elif status == want:
                if payload:
                    self.stats[rank] = payload
                answered.add(rank)

    def run(self, work, model, shards, args, timeout_s=0.0):
        # pickled HERE, not by the queue's feeder thread: an unpicklable model / shard / argument (a lambda, an open handle)
        # raises in the caller like the reference's spawn() does, instead of being printed by the feeder while the parent
        # waits for workers that never got a command
        # (once per worker: a pickled tensor carries a one-shot handle of its shared-memory file)
        blobs = [bytes(ForkingPickler.dumps((work.__module__, work.__name__, model, shards, args))) for _ in self._cmd_qs]
        for q, blob in zip(self._cmd_qs, blobs):
            q.put(blob)
        self._collect("ok", timeout_s, "%s.%s" % (work.__module__, work.__name__))

    def alive(self):
        return bool(self._procs) and all(p.is_alive() for p in self._procs)

    def close(self, force=False):
        for q, p in zip(self._cmd_qs, self._procs):
            if p.is_alive() and not force:
                try:
                    q.put(None)
                except Exception:
                    pass
        pids = set()
        for p in self._procs:
            p.join(timeout=0.1 if force else 20.0)
            if p.is_alive():
                p.terminate()
                p.join(timeout=5.0)
            if p.pid is not None and not p.is_alive():
                pids.add(p.pid)
        self._procs = []
        if pids:
            try:
                _tuned.reap_private_miopen_dbs(pids)
            except Exception:
                pass


def get_pool(devices):
    pool = _POOL[0]
    if pool is not None and (pool.devices != list(devices) or not pool.alive()):
        pool.close()
        pool = _POOL[0] = None
    if pool is None:
        pool = _POOL[0] = WorkerPool(devices)
    return pool


def shutdown_workers():
    """Stop the worker processes (they otherwise live until the interpreter exits)."""
    if _POOL[0] is not None:
        _POOL[0].close()
        _POOL[0] = None


atexit.register(shutdown_workers)


def pool_stats():
    """Per-worker counters after the last step ({} entries before any): CAM hand-offs served from device memory, batches the
    persistent walk handed to the streaming sweeps, and `split_fallback_images` — images `--split_gemm auto` computed again on
    the fp32 GEMMs (_report.worker_stats)."""
    return [] if _POOL[0] is None else [dict(s) for s in _POOL[0].stats]


def spawn_workers(work, model, shards, args):
    """Run `work(process_id, model, shards, args)` for every shard, one worker process per shard, and wait for all of
    them (reference: `multiprocessing.spawn(_work, nprocs=n_gpus, args=(model, dataset, args), join=True)`).  One shard
    on the process's current device runs in-process; otherwise the shards go to the persistent pool.  `work` functions
    that never touch a GPU (CPU tests) may pass args without device information."""
    n = len(shards)
    try:
        devs = worker_devices(args if not isinstance(args, dict) else None)[:n]
    except RuntimeError:
        devs = None                      # no GPU: the callers that need one have raised already (n_gpus_or_raise)
    if devs is None or len(devs) != n:
        if n == 1:
            work(0, model, shards, args)
        else:
            multiprocessing.spawn(work, nprocs=n, args=(model, shards, args), join=True)
        return
    if n == 1 and not getattr(args, "always_use_workers", False):
        # same code path, no second process needed for a single GPU, with the MIOpen settings a pool worker would run with
        # (`process_mode` hands the caller's process back as it found it)
        with _tuned.process_mode(devs[0]) as db_dir:
            if "startup" not in _tuned._WARNED:
                _tuned._WARNED.add("startup")
                _report.say(_report.startup_line(0, 1, devs[0], db_dir))
            work(0, model, shards, args)
            _report.after_step(0, "%s.%s" % (work.__module__, work.__name__))
        return
    get_pool(devs).run(work, model, shards, args, timeout_s=step_timeout(args))


def step_timeout(args=None):
    """Seconds a step may spend in its workers before the pool is stopped (0 = no limit, the reference's behaviour):
    `args.step_timeout` (run_sample.py --step_timeout) or the environment variable IRN_STEP_TIMEOUT_S."""
    v = getattr(args, "step_timeout", None) if args is not None and not isinstance(args, dict) else None
    if v in (None, "", 0, 0.0):
        v = os.environ.get("IRN_STEP_TIMEOUT_S", 0)
    return max(0.0, float(v or 0))
