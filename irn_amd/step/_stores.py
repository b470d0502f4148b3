"""What one step leaves on the device for the next one of the same run: the CAMs of `make_cam` (`CAM_STORE`), the boundary and
displacement maps of whichever label step ran first (`EDGE_STORE`), the run stamp that tells a stale CAM from a current one,
and the shard split that sends an image to the worker holding its CAM (`CAM_OWNERS`)."""
import os
import uuid

import numpy as np
import torch
from torch.utils.data import Subset


class _DeviceStore:
    """A byte-capped, insertion-ordered dictionary of device tensors: the oldest entries leave first, an entry larger than
    the cap is not kept.  What a key and an entry are, and what counts as a hit, is the subclass's."""

    def __init__(self, max_bytes):
        self._items = {}             # insertion-ordered: key -> (entry, nbytes)
        self._bytes = 0
        self._max = max_bytes
        self.hits = self.misses = 0

    def _forget(self, key):
        old = self._items.pop(key, None)
        if old is not None:
            self._bytes -= old[1]

    def _insert(self, key, entry, nbytes):
        self._forget(key)
        while self._items and self._bytes + nbytes > self._max:
            self._forget(next(iter(self._items)))
        if nbytes <= self._max:
            self._items[key] = (entry, nbytes)
            self._bytes += nbytes

    def _entry(self, key):
        hit = self._items.get(key)
        return None if hit is None else hit[0]

    def clear(self):
        self._items.clear()
        self._bytes = 0

    def __len__(self):
        return len(self._items)


class CamStore(_DeviceStore):
    """CAMs of this process kept on the device between steps: `make_cam` puts every image's
    {keys, cam} here besides writing the reference's `.npy` (step/make_cam.py:55-56), and the label steps take them
    from here instead of reading the 1-6 MB pickle back and uploading it again (step/make_sem_seg_labels.py:34-39).
    Entries are keyed by (cam_out_dir, image name) and a later `put` replaces an earlier one, so a second make_cam run
    (other weights, scales or output directory) can never be answered with the first run's CAMs.  A miss — another
    process or an earlier run made the CAM — falls back to the file, so results never depend on the store.  One store
    per process (= per worker and device); a 128x128 CAM is 64 KB per class, so all of VOC12 train_aug (10 582 images)
    is ~1 GB of the 288 GB: capped at `max_bytes` anyway (oldest entries leave first)."""

    def __init__(self, max_bytes=16 << 30):
        super().__init__(max_bytes)

    @staticmethod
    def _key(name, cam_out_dir):
        return (os.path.abspath(cam_out_dir) if cam_out_dir else "", name)

    def put(self, name, keys_cpu, keys_dev, cam, cam_out_dir=None, run_id=None):
        self._insert(self._key(name, cam_out_dir), (keys_cpu, keys_dev, cam, run_id), cam.numel() * cam.element_size())

    def get(self, name, cam_out_dir, device, run_id=None, use_store=True):
        """-> (keys int64 on the CPU, keys on the device, cam fp32 [K,h,w] on the device).  An entry is served only when
        the caller allows it (`use_store`: args.keep_cams_on_device) and it was made by the make_cam run whose stamp the
        output directory carries now (`run_id` = `current_cam_run(cam_out_dir)`): a later make_cam of the same directory —
        in this process, in another pool, with another worker layout — rewrote the files, and this worker's older CAMs
        must not answer for them."""
        hit = self._entry(self._key(name, cam_out_dir)) if use_store else None
        if hit is not None and hit[2].device == device and hit[3] is not None and hit[3] == run_id:
            self.hits += 1
            return hit[:3]
        self.misses += 1
        d = np.load(os.path.join(cam_out_dir, name + ".npy"), allow_pickle=True).item()
        keys = torch.as_tensor(d["keys"])
        return keys, keys.to(device), torch.as_tensor(d["cam"]).to(device)

    def drop(self, name, cam_out_dir):
        """Forget one image's entry (`--split_gemm auto`: a CAM computed from an activation beyond fp16's range)."""
        self._forget(self._key(name, cam_out_dir))

    def drop_dir(self, cam_out_dir):
        """Forget the entries of one output directory (make_cam.run starts with this: its files are about to change)."""
        d = os.path.abspath(cam_out_dir)
        for key in [k for k in self._items if k[0] == d]:
            self._forget(key)


CAM_STORE = CamStore()
_RUN_STAMP = ".irn_cam_run"


def new_cam_run(cam_out_dir):
    """make_cam.run: stamp the output directory with a fresh run id (and return it); the CAMs kept on the device carry
    it, the label steps compare it with the directory's."""
    run_id = uuid.uuid4().hex
    os.makedirs(cam_out_dir, exist_ok=True)
    tmp = os.path.join(cam_out_dir, _RUN_STAMP + ".tmp%d" % os.getpid())
    with open(tmp, "w") as f:
        f.write(run_id)
    os.replace(tmp, os.path.join(cam_out_dir, _RUN_STAMP))
    return run_id


def current_cam_run(cam_out_dir):
    """The run id make_cam last stamped `cam_out_dir` with, or None (CAM files written by something else)."""
    try:
        with open(os.path.join(cam_out_dir, _RUN_STAMP)) as f:
            return f.read().strip() or None
    except OSError:
        return None


def keep_cams(args):
    return bool(getattr(args, "keep_cams_on_device", True))


class EdgeStore(_DeviceStore):
    """Boundary and displacement maps of this process kept on the device between the two label steps.  The reference runs
    `EdgeDisplacement` once per image in make_ins_seg_labels (step/make_ins_seg_labels.py:119-129) and again, on the same
    image with the same weights, in make_sem_seg_labels (step/make_sem_seg_labels.py:28-34): 2 ms of a 2.7 ms image in the
    second step.  Whichever label step runs first puts {edge [1,h,w], dp [2,h,w]} here (196 KB at 512^2; all of VOC12
    train_aug is 1.5 GB), the other one takes them and skips its IRNet forward.  An entry is keyed by the network
    (class + checkpoint path + the file's mtime and size; a network not built from a ModelSpec gets no hand-off), the crop / stride of the forward, and the
    image FILE (path + mtime + size): other weights or another image under the same name is another key.  A miss is simply
    computed.  `args.keep_edges_on_device = False` (run_sample.py --keep_edges_on_device 0) switches it off.  Results: the
    maps are what the first step computed — identical to a recomputation up to MIOpen's choice of solver for another batch
    composition (the tail batch of a shard), like every batched forward here."""

    def __init__(self, max_bytes=8 << 30):
        super().__init__(max_bytes)

    def get(self, key, device):
        hit = self._entry(key)
        if hit is not None and hit[0].device == device:
            self.hits += 1
            return hit
        self.misses += 1
        return None

    def peek(self, key, device):
        """Is the entry there (no hit / miss accounting)?  For the loader threads' `skip_image`."""
        hit = self._entry(key)
        return hit is not None and hit[0].device == device

    def put(self, key, edge, dp):
        self._insert(key, (edge, dp), (edge.numel() + dp.numel()) * 4)

    def drop(self, key):
        """Forget one entry (`--split_gemm auto`: maps computed from an activation beyond fp16's range)."""
        self._forget(key)


EDGE_STORE = EdgeStore()


def keep_edges(args):
    return bool(getattr(args, "keep_edges_on_device", True))


def image_stamp(voc12_root, name):
    """(path, mtime, size) of an image file: part of the EdgeStore key."""
    from ..voc12.dataloader import get_img_path
    path = os.path.abspath(get_img_path(name, voc12_root))
    try:
        st = os.stat(path)
        return (path, st.st_mtime_ns, st.st_size)
    except OSError:
        return (path, -1, -1)


CAM_OWNERS = {}       # abspath(cam_out_dir) -> {image name: worker that made (and still holds) its CAM}


def split_by_owner(dataset, n_splits, names, owners, slack=0.25):
    """Shards for a label step that follows `make_cam` in the same run: image `names[i]` goes to the worker that holds
    its CAM in device memory (`owners[name]`, what `make_cam.run` recorded) as long as that worker's shard stays within
    (1 + slack) of the even share; everything else goes to the least loaded worker, like the reference's strided split
    (misc/torchutils.py:66-68) would balance it.  Which worker processes an image never changes its outputs."""
    n_items = len(names)
    cap = int(np.ceil(n_items / float(n_splits) * (1.0 + slack)))
    shards = [[] for _ in range(n_splits)]
    later = []
    for i, name in enumerate(names):
        o = owners.get(name)
        if o is not None and 0 <= o < n_splits and len(shards[o]) < cap:
            shards[o].append(i)
        else:
            later.append(i)
    for i in later:
        k = min(range(n_splits), key=lambda j: len(shards[j]))
        shards[k].append(i)
    return [Subset(dataset, np.asarray(sorted(s), dtype=np.int64)) for s in shards]


def label_step_shards(dataset, n_workers, args):
    """Shards of make_sem_seg_labels / make_ins_seg_labels: CAM-owner aware when make_cam ran before in this process
    with the same worker layout, else the reference's strided split."""
    from ..misc import torchutils
    owners = CAM_OWNERS.get(os.path.abspath(args.cam_out_dir)) if keep_cams(args) else None
    if owners and owners.get("__n_workers__") == n_workers and n_workers > 1:
        from ..voc12.dataloader import decode_int_filename
        return split_by_owner(dataset, n_workers, [decode_int_filename(v) for v in dataset.img_name_list], owners)
    return torchutils.split_dataset(dataset, n_workers)
