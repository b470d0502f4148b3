"""Semantic pseudo-label step — drop-in for reference step/make_sem_seg_labels.py (`run(args)`).

Reads  args.irn_network, args.irn_weights_name, args.infer_list, args.voc12_root, args.cam_out_dir,
       args.beta, args.exp_times, args.sem_seg_bg_thres, args.num_workers
       args.sem_seg_crf_iters (not in the reference; 0 = off)
Writes args.sem_seg_out_dir/<name>.png  uint8 [H,W] (0 = background, class+1 otherwise)

Per image (step/make_sem_seg_labels.py:28-51): EdgeDisplacement forward (PyTorch-ROCm) -> edge; the image's CAM —
from the device store when make_cam ran in this process, else from its file; random walk of the CAMs over the edge
affinities and the label epilogue run in libirn_hip.so.  Unlike the reference's batch-1 loop the IRNet forward runs
`irn_batch` images per pass (default 8) and the walk is issued for `walk_batch` images at a time (default 64) so one
launch fills the GPU for several rounds; results per image are unchanged.  `args.radius` (default 5 = the
reference's hard-coded value) selects the walk radius.  With `args.sem_seg_crf_iters` T > 0 the epilogue hands its normalised
scores to a dense CRF of T mean-field iterations whose unary is their logarithm (`ops.crf_score_sweep`), one
call per image on the pixels the IRNet saw; the read-back, the writers and the files' format stay as they are.
"""
import os

import torch
from PIL import Image

from .. import ops
from ..net import resnet50 as _r50
from . import _io, _labels, _split_auto


def _save_png(path, label):
    Image.fromarray(label).save(path)


def _start_copy(batch, args):
    """Label epilogue of the batch's walk; its maps (views of one device buffer) leave for the host as ONE copy into page-locked
    memory on the copy stream, behind everything enqueued so far; `_collect` waits for it when the next batch is already queued.
    With `--sem_seg_crf_iters` the maps are the CRF's (`_labels.crf_refine`), in the same buffer layout."""
    t = _labels.crf_iters(args)
    if t:
        flat = _labels.crf_refine(batch["rws"], batch["sizes"], batch["keys"], batch["rgbs"], batch["names"],
                                  float(args.sem_seg_bg_thres), t)
    else:
        flat = ops.label_epilogue(batch["rws"], batch["sizes"], float(args.sem_seg_bg_thres), keys=batch["keys"],
                                  packed=True)["labels_flat"]
    batch["flat"] = flat
    batch["staging"] = _io.PINNED.take(flat.numel())
    batch["done"] = ops.read_back(flat, batch["staging"], side=True)      # (behind the batch's flag words, if any: `_enqueue`)


def _enqueue(model, walker, pend, args, auto=False):
    """IRNet forward, walk, label epilogue and the transfer of the label maps of the images in `pend`, enqueued only;
    returns what `_collect` needs.  `auto` (`--split_gemm auto`): the forward's per-image fp16-range flags leave for the host in
    front of the label maps, on the same stream."""
    kw = _labels.edge_store_kw(model, args)
    _labels.edges_for(model, pend, _labels.irn_batch(args), auto=auto, **kw)
    rws = walker([p["edge"] for p in pend], [p["cam"] for p in pend], beta=float(args.beta), exp_times=int(args.exp_times))
    batch = {"names": [p["name"] for p in pend], "rws": rws, "sizes": [p["size"] for p in pend], "keys": [p["keys_dev"] for p in pend],
             "flags": _labels.flag_read(pend) if auto else None, "store": kw.get("store"),
             "rgbs": [p.get("rgb") for p in pend]}
    _start_copy(batch, args)
    pend.clear()
    return batch


def _collect(walker, batch, args, writer, redo=None):
    """Wait for the batch enqueued last and hand its label maps (already on their way to the host) to the writer threads —
    except those of images that left fp16's range (`--split_gemm auto`): they go on `redo`, nothing is written."""
    if batch is None:
        return
    if walker.sync():                       # the persistent walk gave up and the batch was re-run on the streaming sweeps
        _io.PINNED.give(batch.pop("staging"))
        _start_copy(batch, args)
    batch["done"].synchronize()
    host = batch["staging"].numpy()
    # the flag words were copied on the current stream BEFORE the epilogue whose output `done` marks as landed
    bad = _labels.drop_flagged(batch.pop("flags", None), redo, batch.get("store"))
    off = 0
    for name, (hh, ww) in zip(batch["names"], batch["sizes"]):
        lab = host[off:off + hh * ww].reshape(hh, ww).copy()      # 256 KB: the staging buffer goes back at once
        off += hh * ww
        if name in bad:
            continue
        writer.submit(_save_png, os.path.join(args.sem_seg_out_dir, name + ".png"), lab)
    _io.PINNED.give(batch.pop("staging"))


def _work(process_id, model, dataset, args):
    batch = _labels.walk_batch(args, 64)    # 64 VOC-size images = 3-4 rounds of the resident walk
    with _labels.worker(process_id, model, dataset, args, keep_rgb=_labels.crf_iters(args) > 0) as w:
        # a batch is enqueued and left running while the loop gathers the next one (decoded images from the loader
        # threads, their uploads, the CAMs); it is collected just before the next batch is enqueued
        pend, running = [], None
        auto = _split_auto.enabled()
        redo = _split_auto.Redo() if auto else None
        try:
            for item in _labels.items(w, args):
                pend.append(item)
                if len(pend) == batch:
                    _collect(w.walker, running, args, w.writer, redo)
                    running = _enqueue(w.model, w.walker, pend, args, auto)
            _collect(w.walker, running, args, w.writer, redo)
            running = None
            if pend:
                running = _enqueue(w.model, w.walker, pend, args, auto)
                _collect(w.walker, running, args, w.writer, redo)
                running = None
            if auto:
                # the images that left fp16's range once more, IRNet on the fp32 GEMMs: their maps go back into the store
                todo = _labels.redo_items(redo, w, args)
                with _r50.fp32_gemms():
                    for i in range(0, len(todo), batch):
                        running = _enqueue(w.model, w.walker, todo[i:i + batch], args)
                        _collect(w.walker, running, args, w.writer)
                        running = None
                redo.report(process_id)
        except BaseException:           # the batch in flight stays uncollected: its buffer goes back once the copy into it has landed
            if running is not None and "staging" in running:
                running["done"].synchronize()
                _io.PINNED.give(running.pop("staging"))
            raise


def run(args):
    if _labels.crf_iters(args):
        _labels.check_crf(args, "make_sem_seg_labels", args.sem_seg_bg_thres)
    _labels.run_step(_work, args.sem_seg_out_dir, args)
    torch.cuda.empty_cache()
