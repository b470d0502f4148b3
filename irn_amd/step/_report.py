"""What a step says and checks about itself: the start-up line of a worker, the summary line and the fp16-range check at the
end of a step (`after_step`: the same for a pool worker and for the in-process path), and the counters bench.py reads."""
import os
import sys

import torch

from .. import _tuned
from . import _stores

# make_cam's trunk passes of this process, by layout (net/resnet50.channels_last_for: channels-last only for input shapes the
# shipped find database is tuned for), and its size-group flushes (full groups of `cam_batch` images vs partial ones)
CAM_STATS = {"channels_last": 0, "nchw": 0, "full_group_flushes": 0, "partial_group_flushes": 0}      # (passes, not flushes: a partial group is one padded pass, an untuned size one pass per image — net/resnet50.run_rows)
WALK_STATS = {"fallback_runs": 0}
# `--split_gemm auto`: images of this process that left fp16's range on the split-precision GEMMs and were computed again on the
# fp32 ones (step/_split_auto.py), summed over the steps
SPLIT_STATS = {"fallback_images": 0}


def untuned_report(reset=True):
    """One line about the trunk passes of this process that took the NCHW branch (network-input sizes the shipped database
    is not tuned for: net/resnet50.channels_last_for), counts per size, or "" when there were none; printed at the end of
    every step by whoever ran it.  `reset` starts the next step's count."""
    from ..net import resnet50 as _r50
    sizes = dict(_r50.PASS_STATS["nchw_sizes"])
    n_cl, n_nchw, pad = _r50.PASS_STATS["channels_last"], _r50.PASS_STATS["nchw"], _r50.PASS_STATS["pad_rows"]
    if reset:
        _r50.PASS_STATS.update({"channels_last": 0, "nchw": 0, "pad_rows": 0, "nchw_sizes": {}})
    if not sizes:
        return ""
    top = sorted(sizes.items(), key=lambda kv: -kv[1])
    return ("irn_amd: %d of %d trunk passes ran NCHW (~0.8x) because their network-input size is not in the tuned database: %s%s"
            "%s; tools/miopen_warmup.py --channels-last 1 --sizes ... (or --from-list <image list>) adds sizes" % (
                n_nchw, n_nchw + n_cl, ", ".join("%s x%d" % kv for kv in top[:8]), ", ... (%d sizes)" % len(top) if len(top) > 8 else "",
                "; %d zero rows filled partial passes" % pad if pad else ""))


def say(line):
    """One whole line on stderr in ONE write: eight ranks starting at once must not interleave each other's lines."""
    try:
        sys.stderr.flush()
        os.write(sys.stderr.fileno(), (line.rstrip("\n") + "\n").encode("utf-8", "replace"))
    except Exception:            # no real file behind sys.stderr (a capturing harness)
        print(line, file=sys.stderr, flush=True)


def startup_line(rank, n_workers, device, db_dir):
    """One line per worker / rank at start-up (stderr): which device it owns and whether the data this build's speed rests
    on was found for it — the things that differ between the box the defaults were measured on and an eight-GPU node met for
    the first time (reference step/make_cam.py:67-74 spawns its workers without a word)."""
    rep = _tuned.shipped_data_report()
    try:
        props = torch.cuda.get_device_properties(int(device))
        chip = "%s, %d CUs, %.0f GB" % (_tuned.arch_name(props, "?"), props.multi_processor_count, props.total_memory / 2 ** 30)
    except Exception:
        chip = "no GPU"
    try:
        from ..misc import indexing
        poll = indexing.poll_delay_report(int(device))
    except Exception:
        poll = "poll delay: n/a"
    return ("irn_amd worker %d/%d: cuda:%d (%s) | %s backbones | MIOpen database '%s': %s, user database %s | GEMM rank table: %s | %s"
            % (int(rank), int(n_workers), int(device), chip, "reproducible" if _tuned.deterministic_backbones() else "fast",
               rep["mode_key"], "shipped" if rep["miopen"] else "NOT SHIPPED (NCHW trunk)", db_dir, "shipped" if rep["gemm"] else "not shipped", poll))


def step_summary(rank, walker=None):
    """One line at the end of a step (stderr) when there is something to say: trunk passes that fell to the NCHW branch by
    size, and the walk's self-checks (block -> XCD placement, poll delay and where it came from, fall-backs)."""
    parts = []
    msg = untuned_report()
    if msg:
        parts.append(msg)
    if walker is not None:
        try:
            t = walker.tuning()
            parts.append("irn_amd: walk radius %d: XCD placement %s, poll delay %d (%s), %d fall-back run(s)" % (
                walker.radius, {0: "not checked", 1: "round robin holds", 2: "does NOT hold (no XCD packing)"}.get(t["placement"], "?"),
                t["poll_delay"], getattr(walker, "poll_delay_source", "library default"), walker.fallback_runs))
        except Exception:
            pass
    for m in parts:
        say("[worker %d] %s" % (int(rank), m))


def split_fallback_line(names):
    """The line a worker says at the end of a step that recomputed `names` on the fp32 GEMMs; "" for none."""
    names = list(names)
    if not names:
        return ""
    return ("irn_amd: split_gemm auto: %d image(s) left fp16's range on the split-precision GEMMs and were computed again on the fp32 "
            "GEMMs (no file was written from the split pass): %s%s" % (len(names), ", ".join(names[:8]),
                                                                      ", ... (%d more)" % (len(names) - 8) if len(names) > 8 else ""))


def check_split_overflow(what):
    """End of a step: did an activation leave fp16's range inside the split-precision 1x1 convolutions (net/resnet50.py
    SPLIT_GEMM)?  Then this step's outputs are invalid and the step raises — loudly, like a worker's exception.  (The process-wide
    flag: with `--split_gemm auto` the passes of make_cam and the label steps record per sample instead and recover, so only a
    split pass outside them can raise here.)"""
    from .. import ops
    if ops.split_overflowed():
        raise RuntimeError("%s: an activation of the backbone was beyond fp16's range (|x| > 65504) or NaN inside the split-precision "
                           "1x1 convolutions; the outputs of this step are INVALID.  Run with IRN_SPLIT_GEMM=0 (run_sample.py "
                           "--split_gemm 0): the fp32 GEMMs have no such limit." % what)


def after_step(rank, what):
    """What follows a shard's `work` on its device, whichever process ran it: wait for the device, the summary line, the
    fp16-range check.  A 1-GPU run and an N-GPU run check the same things because both come through here."""
    torch.cuda.synchronize()
    step_summary(rank)
    check_split_overflow(what)


def worker_stats():
    """The counters of this process that a pool worker sends back with every finished step (`_pool.pool_stats`)."""
    return {"cam_store_hits": _stores.CAM_STORE.hits, "cam_store_misses": _stores.CAM_STORE.misses,
            "edge_store_hits": _stores.EDGE_STORE.hits, "edge_store_misses": _stores.EDGE_STORE.misses,
            "walk_fallback_runs": WALK_STATS["fallback_runs"], "cam_trunk_passes": dict(CAM_STATS),
            "split_fallback_images": SPLIT_STATS["fallback_images"]}
