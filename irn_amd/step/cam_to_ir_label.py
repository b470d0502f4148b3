"""IR-label step — drop-in for reference step/cam_to_ir_label.py (`run(args)`).

Reads  args.train_list, args.voc12_root, args.cam_out_dir (the `high_res` / `keys` of make_cam's <name>.npy),
       args.conf_fg_thres, args.conf_bg_thres, args.num_workers
Writes args.ir_label_out_dir/<name>.png  uint8 [H,W]: 0 confident background, class+1 confident foreground, 255 unsure

Per image (step/cam_to_ir_label.py:22-39): the fg- and bg-threshold seeds of the CAMs, two dense CRFs
(misc/imutils.py:156-170, t = 10, gt_prob = 0.7) and their combination run in libirn_hip.so as ONE call
(`ops.crf_ir_label`): both CRFs share the image's lattices and run as one filter over 2 * (classes + 1) channels; one
uint8 map comes back.  Images are decoded and their CAM files read by loader threads; PNGs are written by the writer
threads.  Every image is computed on its own, so outputs do not depend on the number or layout of the workers.
"""
import os

import numpy as np
import torch
from PIL import Image

from .. import ops
from ..voc12 import dataloader as voc12_dataloader
from . import _io, _pool


def _save_png(path, label):
    Image.fromarray(label).save(path)


class IrLabelDataset(torch.utils.data.Dataset):
    """Images of `img_name_list_path` (uint8 HWC RGB, voc12/dataloader.py convert("RGB")) with their CAMs."""

    def __init__(self, img_name_list_path, voc12_root, cam_out_dir):
        self.img_name_list = voc12_dataloader.load_img_name_list(img_name_list_path)
        self.voc12_root = voc12_root
        self.cam_out_dir = cam_out_dir

    def __len__(self):
        return len(self.img_name_list)

    def __getitem__(self, idx):
        name = voc12_dataloader.decode_int_filename(self.img_name_list[idx])
        img = np.array(Image.open(voc12_dataloader.get_img_path(name, self.voc12_root)).convert("RGB"))
        cam = np.load(os.path.join(self.cam_out_dir, name + ".npy"), allow_pickle=True).item()
        keys = np.asarray(cam["keys"], np.int64).reshape(-1)
        high_res = np.ascontiguousarray(cam["high_res"], np.float32)
        if keys.size == 0:
            high_res = np.zeros((0,) + img.shape[:2], np.float32)
        return {"name": name, "img": torch.from_numpy(img), "high_res": torch.from_numpy(high_res),
                "keys": torch.from_numpy(keys)}


def _work(process_id, model, dataset, args):
    del model                                   # no network: the CRF is the whole step
    fg_thres, bg_thres = float(args.conf_fg_thres), float(args.conf_bg_thres)
    with _io.shard_io(process_id, dataset, args) as (databin, n_workers, loader, writer):
        dev_id = _pool.worker_device(process_id, args)
        with torch.cuda.device(dev_id):
            pending = None
            for it, pack in enumerate(loader):
                name = pack["name"][0]
                # uploads through page-locked buffers: the host never waits for the previous image's CRF here
                img = _io.upload(pack["img"][0], pack.pop("_staging", None))
                high_res = _io.upload(pack["high_res"][0])
                keys = _io.upload(pack["keys"][0])
                conf = ops.crf_ir_label(img, high_res, keys, fg_thres, bg_thres)
                host = _io.PINNED.take(conf.numel())
                host[:conf.numel()].copy_(conf.view(-1), non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                if pending is not None:          # the previous image's map is home while this one runs
                    _finish(pending, args, writer)
                pending = (name, tuple(conf.shape), host, done)
                _io.progress(process_id, n_workers, it, len(databin))
            if pending is not None:
                _finish(pending, args, writer)


def _finish(pending, args, writer):
    name, (h, w), host, done = pending
    done.synchronize()
    conf = host[:h * w].numpy().reshape(h, w).copy()
    _io.PINNED.give(host)
    writer.submit(_save_png, os.path.join(args.ir_label_out_dir, name + ".png"), conf)


def run(args):
    n_gpus = _pool.n_gpus_or_raise(args)
    dataset = IrLabelDataset(args.train_list, args.voc12_root, args.cam_out_dir)
    from ..misc import torchutils
    dataset = torchutils.split_dataset(dataset, n_gpus)
    os.makedirs(args.ir_label_out_dir, exist_ok=True)
    print("[", end="")
    _pool.spawn_workers(_work, None, dataset, args)
    print("]")
