"""What the training benches (train_cam_bench, train_irn_bench, train_seg_bench) share: the synthetic tree, the host
pipeline's timing and the timed step loop."""
import os
import statistics
import time

import numpy as np
import torch

from irn_amd import synth


def write_tree(root, n, repeat=1, labels=None):
    """n synthetic VOC-size JPEGs under `root` and a list that names each `repeat` times (so that one pass over it is long
    enough to time without a loader start inside).  `labels`: "cls" writes cls_labels.npy; "ir" IR label PNGs (0 / class + 1
    / 255 in 16-pixel blocks) into ir_label/; "sem_seg" blob label maps (0, two classes, 255 between them) into sem_seg/ as
    `result/sem_seg` would hold them.  -> (list file, label directory or None)."""
    from PIL import Image
    os.makedirs(os.path.join(root, "JPEGImages"), exist_ok=True)
    label_dir = os.path.join(root, {"ir": "ir_label", "sem_seg": "sem_seg"}[labels]) if labels in ("ir", "sem_seg") else None
    if label_dir:
        os.makedirs(label_dir, exist_ok=True)
    names, cls_labels = [], {}
    for i in range(n):
        name = "2008_%06d" % (i + 1)
        h, w = synth.voc_image_size(i)
        Image.fromarray(synth.photo(h, w, seed=i)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=90)
        if labels == "cls":
            lab = np.zeros(20, np.float32)
            lab[synth.voc_keys(synth.voc_num_classes(i), i)] = 1
            cls_labels[int(name.replace("_", ""))] = lab
        elif labels == "ir":
            values = np.asarray([0, 255] + [int(k) + 1 for k in synth.voc_keys(synth.voc_num_classes(i), i)], np.uint8)
            lab = np.random.RandomState(i).choice(values, (h // 16 + 1, w // 16 + 1)).repeat(16, 0).repeat(16, 1)[:h, :w]
            Image.fromarray(np.ascontiguousarray(lab)).save(os.path.join(label_dir, name + ".png"))
        elif labels == "sem_seg":
            cls, _ = synth.blob_ground_truth(synth.cam_blobs(2, h, w, seed=i), [i % 20, (i + 7) % 20], 0.5, 0.35)
            Image.fromarray(cls).save(os.path.join(label_dir, name + ".png"))
        names.append(name)
    lst = os.path.join(root, "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(names * repeat) + "\n")
    if labels == "cls":
        np.save(os.path.join(root, "cls_labels.npy"), cls_labels, allow_pickle=True)
    return lst, label_dir


def bench_host_pipeline(raw, host, n):
    """The worker's share of a host item beyond the decodes both forms pay: item(raw=False) - item(raw=True)."""
    t_raw, t_host = [], []
    for i in range(n):
        t0 = time.perf_counter()
        raw[i]
        t1 = time.perf_counter()
        host[i]
        t2 = time.perf_counter()
        t_raw.append((t1 - t0) * 1e3)
        t_host.append((t2 - t1) * 1e3)
    return {"images": n, "decode_only_ms_median": statistics.median(t_raw), "decode_and_augment_ms_median": statistics.median(t_host)}


def timed_steps(dataset, make_loader, step, warmup, steps, batch):
    """`step(pack)` over the batches of `make_loader(epoch)`, epochs rolling over, until `warmup + steps` are done; the clock
    starts behind a device synchronise before step `warmup` and stops behind another.  -> (the figures every `step` line
    carries, what the last `step` returned)."""
    torch.cuda.reset_peak_memory_stats()
    done, t0, ep, last = 0, None, 0, None
    while done < warmup + steps:
        dataset.set_epoch(ep)
        for pack in make_loader(ep):
            if done == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            last = step(pack)
            done += 1
            if done == warmup + steps:
                break
        ep += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"steps": steps, "seconds": dt, "images_per_s": steps * batch / dt, "ms_per_step": dt / steps * 1e3,
            "max_memory_allocated_mb": torch.cuda.max_memory_allocated() / 2 ** 20}, last
