"""`irn_amd.step._common` as a facade over the modules its code moved into, and those modules' host logic: the device stores,
the thread loader and writer, the worker-side model cache, the label worker and the shard scaffolding (`_io.shard_io`).  No GPU."""
import os

import numpy as np
import pytest
import torch

from irn_amd import _tuned
from irn_amd.step import _common, _io, _labels, _pool, _report, _stores

# the names `_common` defined or imported (without a leading underscore) when all of the step plumbing was that one file
COMMON_NAMES = [
    "AsyncWriter", "CAM_OWNERS", "CAM_STATS", "CAM_STORE", "CamStore", "EDGE_STORE", "EdgeStore", "ForkingPickler",
    "MAX_LOADER_THREADS", "ModelSpec", "PINNED", "PinnedPool", "Subset", "ThreadPoolExecutor", "WALK_STATS", "WorkerPool",
    "apply_deterministic_setting", "atexit", "check_split_overflow", "current_cam_run", "deterministic_backbones",
    "device_images", "device_preprocess", "gemm_table_root", "get_pool", "image_stamp", "import_network", "importlib",
    "keep_cams", "keep_edges", "label_step_shards", "make_loader", "make_walker", "materialise", "merge_miopen_db",
    "miopen_cache_key", "miopen_mode_key", "miopen_seed_root", "miopen_setup", "multiprocessing", "n_gpus_or_raise",
    "new_cam_run", "np", "os", "pickle", "pool_stats", "progress", "reap_private_miopen_dbs", "say", "set_skip_image",
    "shipped_data_report", "shutdown_workers", "spawn_workers", "split_by_owner", "startup_line", "step_summary",
    "step_timeout", "torch", "traceback", "untuned_report", "upload", "walk_radius", "warn_missing_shipped_data",
    "worker_device", "worker_devices", "writer_threads"]


def test_common_keeps_every_public_name_and_shares_the_one_object():
    assert len(COMMON_NAMES) == 66 and len(set(COMMON_NAMES)) == 66
    assert [n for n in COMMON_NAMES if not hasattr(_common, n)] == []
    # bench.py reads the counters and stores through the facade: they must be the objects the steps write to
    assert _common.CAM_STORE is _stores.CAM_STORE and _common.EDGE_STORE is _stores.EDGE_STORE
    assert _common.CAM_OWNERS is _stores.CAM_OWNERS and _common.PINNED is _io.PINNED
    assert _common.CAM_STATS is _report.CAM_STATS and _common.WALK_STATS is _report.WALK_STATS
    # and the functions are the home modules' own, not copies
    assert _common.miopen_setup is _tuned.miopen_setup and _common.spawn_workers is _pool.spawn_workers
    assert _common.make_walker is _labels.make_walker and _common.worker_device is _pool.worker_device


def test_async_writer_writes_everything_and_surfaces_errors(tmp_path):
    from irn_amd.step import _common
    w = _common.AsyncWriter(threads=2, max_pending=3)
    for i in range(10):
        w.submit(np.save, str(tmp_path / ("f%d.npy" % i)), {"i": i})
    w.close()
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted("f%d.npy" % i for i in range(10))
    assert np.load(str(tmp_path / "f7.npy"), allow_pickle=True).item() == {"i": 7}
    w = _common.AsyncWriter(threads=1, max_pending=1)
    w.submit(np.save, str(tmp_path / "no_such_dir" / "x.npy"), 1)
    with pytest.raises(Exception):
        w.close()


def test_thread_loader_collates_like_dataloader(tmp_path):
    """irn_amd.step._common.make_loader (thread prefetcher) yields exactly what DataLoader(batch_size=1, shuffle=False)
    yields for the multi-scale dataset, raw and pre-scaled items, with and without worker threads."""
    from PIL import Image
    from torch.utils.data import DataLoader
    from irn_amd.step import _common
    from irn_amd.voc12 import dataloader as vd
    (tmp_path / "JPEGImages").mkdir()
    names, labels = [], {}
    rng = np.random.RandomState(0)
    for i in range(5):
        n = "2008_%06d" % (i + 1)
        names.append(n)
        Image.fromarray((rng.rand(40 + i, 50, 3) * 255).astype(np.uint8)).save(tmp_path / "JPEGImages" / (n + ".jpg"))
        labels[int(n.replace("_", ""))] = np.eye(20, dtype=np.float32)[i]
    (tmp_path / "train.txt").write_text("\n".join(names) + "\n")
    np.save(tmp_path / "cls_labels.npy", labels)
    for raw in (True, False):
        ds = vd.VOC12ClassificationDatasetMSF(str(tmp_path / "train.txt"), voc12_root=str(tmp_path), scales=(1.0, 0.5), raw=raw)
        want = list(DataLoader(ds, shuffle=False, num_workers=0))
        for nw in (0, 3):
            got = list(_common.make_loader(ds, nw))
            assert len(got) == len(want)
            for x, y in zip(want, got):
                assert x["name"] == y["name"] and torch.equal(x["label"], y["label"])
                assert [int(v) for v in x["size"]] == [int(v) for v in y["size"]]
                if raw:
                    assert torch.equal(x["img"], y["img"])
                else:
                    assert all(torch.equal(p, q) for p, q in zip(x["img"], y["img"]))


def test_cam_store_hit_and_file_fallback(tmp_path):
    """step/_common.CamStore: a CAM put by make_cam is handed to the label steps from memory; anything else comes from the
    `.npy` the reference's make_cam writes (step/make_cam.py:55-56) — same values either way.  Entries belong to ONE
    output directory AND to one make_cam run: a later put replaces an earlier one, and an entry of a run the directory
    no longer carries the stamp of (make_cam ran again somewhere else) is never served."""
    from irn_amd.step import _common
    store = _common.CamStore(max_bytes=1 << 20)
    dev = torch.device("cpu")
    keys = torch.tensor([3, 7])
    cam = torch.rand(2, 8, 9)
    np.save(tmp_path / "2008_000001.npy", {"keys": keys, "cam": cam, "high_res": np.zeros((2, 32, 36), np.float32)})
    run1 = _common.new_cam_run(str(tmp_path))
    assert _common.current_cam_run(str(tmp_path)) == run1 and _common.current_cam_run(str(tmp_path / "nowhere")) is None
    store.put("2008_000001", keys, keys.clone(), cam.clone(), cam_out_dir=str(tmp_path), run_id=run1)
    k_cpu, k_dev, c = store.get("2008_000001", str(tmp_path), dev, run1)
    assert store.hits == 1 and store.misses == 0 and torch.equal(k_cpu, keys) and torch.equal(c, cam)
    # keep_cams_on_device off: the store is not consulted
    store.get("2008_000001", str(tmp_path), dev, run1, use_store=False)
    assert store.hits == 1 and store.misses == 1
    # a second run with other weights: same name, new values -> the new ones are served
    cam2 = torch.rand(2, 8, 9)
    store.put("2008_000001", keys, keys.clone(), cam2.clone(), cam_out_dir=str(tmp_path), run_id=run1)
    assert torch.equal(store.get("2008_000001", str(tmp_path), dev, run1)[2], cam2) and len(store) == 1
    assert store._bytes == cam2.numel() * 4
    # make_cam ran again for this directory in ANOTHER process (new stamp, new file): this store's entry is stale
    run2 = _common.new_cam_run(str(tmp_path))
    assert run2 != run1
    cam_new = torch.rand(2, 8, 9)
    np.save(tmp_path / "2008_000001.npy", {"keys": keys, "cam": cam_new, "high_res": np.zeros((2, 32, 36), np.float32)})
    got = store.get("2008_000001", str(tmp_path), dev, _common.current_cam_run(str(tmp_path)))
    assert torch.equal(got[2], cam_new) and store.misses == 2
    # an entry without a stamp (or a directory without one) is never a hit
    assert torch.equal(store.get("2008_000001", str(tmp_path), dev, None)[2], cam_new) and store.misses == 3
    # the same name under another output directory is another entry: served from ITS file
    other = tmp_path / "other"
    other.mkdir()
    cam3 = torch.rand(2, 8, 9)
    np.save(other / "2008_000001.npy", {"keys": keys, "cam": cam3, "high_res": np.zeros((2, 32, 36), np.float32)})
    assert torch.equal(store.get("2008_000001", str(other), dev, run2)[2], cam3) and store.misses == 4
    store.drop_dir(str(tmp_path))
    assert len(store) == 0 and store._bytes == 0
    k_cpu, k_dev, c = store.get("2008_000001", str(tmp_path), dev, run2)
    assert store.misses == 5 and torch.equal(k_cpu, keys) and torch.equal(k_dev, keys) and torch.equal(c, cam_new)
    big = torch.zeros(1, 1024, 1024)                       # 4 MB > the 1 MB cap: not kept, never an error
    store.put("big", keys[:1], keys[:1], big, cam_out_dir=str(tmp_path), run_id=run2)
    assert len(store) == 0
    for i in range(40):                                    # 40 x 36 KB > 1 MB: the oldest entries leave
        store.put("n%d" % i, keys, keys, torch.zeros(1, 96, 96), cam_out_dir=str(tmp_path), run_id=run2)
    assert store._bytes <= 1 << 20 and ("%s" % tmp_path, "n39") in store._items and ("%s" % tmp_path, "n0") not in store._items


def test_split_by_owner_hits_and_balance():
    """Label-step shards that follow make_cam's CAM placement: every image whose CAM a worker holds goes to that worker
    while the shards stay within 25 % of the even share; unknown images fill the lightest shards; every image exactly
    once (the reference's strided split, misc/torchutils.py:66-68, is the fallback)."""
    from irn_amd.step import _common
    rng = np.random.default_rng(0)
    names = ["img%04d" % i for i in range(1000)]
    made = {"img%04d" % i: int(i % 8) for i in rng.permutation(1200)[:900]}      # CAMs of 900 images, strided over 8 workers
    shards = _common.split_by_owner(list(range(1000)), 8, names, made)
    seen = sorted(int(i) for s in shards for i in s.indices)
    assert seen == list(range(1000))
    assert max(len(s) for s in shards) <= int(np.ceil(1000 / 8 * 1.25))
    hits = sum(1 for k, s in enumerate(shards) for i in s.indices if made.get(names[int(i)]) == k)
    known = sum(1 for n in names if n in made)
    assert hits >= 0.97 * known, (hits, known)
    # a pathological placement (everything on worker 0) is capped, not followed
    shards = _common.split_by_owner(list(range(100)), 4, names[:100], {n: 0 for n in names[:100]})
    assert [len(s) for s in shards][0] == 32 and sorted(int(i) for s in shards for i in s.indices) == list(range(100))


def test_model_spec_is_built_once_per_checkpoint_version(tmp_path):
    """step/_common.ModelSpec: what a step's run(args) hands its (persistent) workers instead of a pickled network — built by
    the worker on first use, reused by later steps naming the same checkpoint, rebuilt when the file changes."""
    import os
    from irn_amd.net import weights
    from irn_amd.step import _common, _pool
    path = str(tmp_path / "cam.pth")
    torch.save(weights.random_cam_state(1), path)
    spec = _common.ModelSpec("net.resnet50_cam", "CAM", path, strict=True)
    a = _common.materialise(spec)
    assert _common.materialise(_common.ModelSpec("net.resnet50_cam", "CAM", path, strict=True)) is a     # same key, same object
    assert _common.materialise(a) is a                                                                   # networks pass through
    sd = weights.random_cam_state(7)
    torch.save(sd, path)
    os.utime(path, ns=(os.stat(path).st_atime_ns, os.stat(path).st_mtime_ns + 10 ** 9))
    b = _common.materialise(spec)
    assert b is not a and torch.equal(b.state_dict()["classifier.weight"], sd["classifier.weight"])
    assert sum(1 for k in _pool._MODELS if k[2] == os.path.abspath(path)) == 1                         # the old version was dropped


def test_edge_store_keys_and_cap(tmp_path):
    """step/_common.EdgeStore: the boundary / displacement maps one label step leaves for the other are keyed by network,
    forward geometry and image FILE; another checkpoint, another image under the same name (new mtime / size) or another
    device is a miss; the oldest entries leave when the cap is reached; edges_for fills and uses it."""
    from irn_amd.step import _common, _labels
    root = tmp_path / "voc"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "JPEGImages" / "2008_000001.jpg").write_bytes(b"a" * 100)
    stamp = _common.image_stamp(str(root), "2008_000001")
    assert stamp[0].endswith("2008_000001.jpg") and stamp[2] == 100
    (root / "JPEGImages" / "2008_000001.jpg").write_bytes(b"b" * 101)
    assert _common.image_stamp(str(root), "2008_000001") != stamp and _common.image_stamp(str(root), "missing")[1:] == (-1, -1)

    class _Net:                      # stands in for EdgeDisplacement: counts its forwards
        crop_size, stride, calls = 512, 4, 0

        def forward_batch(self, items):
            _Net.calls += 1
            return [(it[:1, 0, ::4, ::4] + 1.0, it[:, 0, ::4, ::4] * 2.0) for it in items]

    store = _common.EdgeStore(max_bytes=1 << 20)
    net = _Net()
    mk = lambda names: [{"name": n, "img": torch.full((2, 3, 16, 20), float(i)), "stamp": ("/p/" + n, 1, 2)} for i, n in enumerate(names)]
    a = mk(["x", "y", "z"])
    _labels.edges_for(net, a, 2, store=store, model_key=("ckpt", 1))
    assert _Net.calls == 2 and store.misses == 3 and store.hits == 0 and len(store) == 3 and "img" not in a[0]
    b = mk(["x", "y", "z", "w"])
    _labels.edges_for(net, b, 2, store=store, model_key=("ckpt", 1))
    assert _Net.calls == 3 and store.hits == 3                                    # only "w" went through the network
    for p, q in zip(a, b):
        assert torch.equal(p["edge"], q["edge"]) and torch.equal(p["dp"], q["dp"])
    c = mk(["x"])
    _labels.edges_for(net, c, 2, store=store, model_key=("ckpt", 2))   # another checkpoint: computed again
    assert _Net.calls == 4
    d = mk(["x"])
    d[0]["stamp"] = ("/p/x", 9, 2)                                                # the file changed
    _labels.edges_for(net, d, 2, store=store, model_key=("ckpt", 1))
    assert _Net.calls == 5
    e = mk(["x"])
    _labels.edges_for(net, e, 2)                                       # no store: always computed, nothing stored
    assert _Net.calls == 6 and "stamp" in e[0]
    small = _common.EdgeStore(max_bytes=3 * 4 * 60)
    for i in range(5):
        small.put(("k", i), torch.zeros(1, 4, 5), torch.zeros(2, 4, 5))
    assert len(small) == 3 and small.get(("k", 0), torch.device("cpu")) is None and small.get(("k", 4), torch.device("cpu")) is not None


def _stub_label_worker(monkeypatch, packs, fail_cam_at=None):
    """step/_labels.worker() / items() without a GPU: network, loader, writer, walker, device context, CAM store and uploads are
    stand-ins that record what happens to them.  -> (events, args, model); the CAM look-up number `fail_cam_at` raises OSError."""
    import argparse
    import contextlib
    from irn_amd.step import _common, _io, _labels, _pool, _report
    events = []

    class _Model:
        def cuda(self):
            events.append("model.cuda")

    class _Walker:
        fallback_runs, radius = 3, 5

        def __call__(self, edges, cams, **kw):
            events.append(("walk", len(edges)))
            return ["rw"] * len(edges)

        def sync(self):
            return False

        def close(self):
            events.append("walker.close")

    class _Writer:
        def __init__(self, threads):
            pass

        def submit(self, fn, *a, **kw):
            events.append(("submit", os.path.basename(a[0])))

        def close(self):
            events.append("writer.close")

    def cam_get(name, cam_out_dir, dev, run_id=None, use_store=True):
        events.append(("cam", name))
        if fail_cam_at is not None and sum(1 for e in events if e[0] == "cam") > fail_cam_at:
            raise OSError("no CAM file for " + name)
        return torch.tensor([3, 7]), "keys_dev-" + name, "cam-" + name

    monkeypatch.setattr(_pool, "materialise", lambda model: events.append("materialise") or model)
    monkeypatch.setattr(_pool, "worker_device", lambda process_id, args=None: 0)
    monkeypatch.setattr(_io, "make_loader", lambda databin, num_workers, prefetch=4: iter(packs))
    monkeypatch.setattr(_io, "AsyncWriter", _Writer)
    monkeypatch.setattr(_labels, "make_walker", lambda args, radius: _Walker())
    monkeypatch.setattr(_report, "step_summary", lambda rank, walker=None: events.append("summary"))
    monkeypatch.setattr(_io, "progress", lambda pid, n, it, n_items: events.append(("tick", pid, n, it, n_items)))
    monkeypatch.setattr(_io, "device_images", lambda pack, scales: None if pack["img"].numel() == 0 else [pack["img"][0].float()])
    monkeypatch.setattr(_common.CAM_STORE, "get", cam_get)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    args = argparse.Namespace(num_workers=0, voc12_root="/no/such/voc", cam_out_dir="/no/such/cam", sem_seg_out_dir="/no/such/sem",
                              beta=10, exp_times=8, sem_seg_bg_thres=0.25, walk_batch=1)
    return events, args, _Model()


def _label_packs():
    """Two collated loader items: a `str` name with pixels, an integer-encoded name whose pixels the skip predicate emptied."""
    return [{"name": ["2008_000001"], "size": torch.tensor([[6], [4]]), "img": torch.ones(1, 6, 4, 3, dtype=torch.uint8)},
            {"name": torch.tensor([2008000002]), "size": torch.tensor([[5], [7]]), "img": torch.zeros(1, 0, dtype=torch.uint8)}]


def test_label_worker_closes_walker_and_writer_on_both_paths(monkeypatch):
    """step/_labels.worker: leaving the block normally adds the walker's fall-back runs to WALK_STATS once, prints the summary,
    then closes walker and writer; an exception in the block closes both, adds nothing and comes out as it was raised."""
    from irn_amd.step import _common, _labels
    events, args, model = _stub_label_worker(monkeypatch, _label_packs())
    monkeypatch.setitem(_common.WALK_STATS, "fallback_runs", 10)
    with _labels.worker(1, model, [["x"], ["y", "z"]], args) as w:
        assert (w.model, w.databin, w.n_gpus, w.dev) == (model, ["y", "z"], 2, torch.device("cuda", 0))
        assert w.walker.fallback_runs == 3 and hasattr(w.writer, "submit") and len(list(w.loader)) == 2
        assert not torch.is_grad_enabled() and "walker.close" not in events
    assert _common.WALK_STATS["fallback_runs"] == 13 and torch.is_grad_enabled()
    assert events == ["materialise", "model.cuda", "summary", "walker.close", "writer.close"]
    del events[:]
    boom = RuntimeError("a bad CAM file")
    with pytest.raises(RuntimeError) as info:
        with _labels.worker(0, model, [["x"]], args):
            raise boom
    assert info.value is boom and _common.WALK_STATS["fallback_runs"] == 13
    assert events == ["materialise", "model.cuda", "walker.close", "writer.close"]


def test_label_items_yield_what_both_steps_consume(monkeypatch):
    """step/_labels.items: per image the dict both label steps built (name decoded, size as ints, pixels or None, device, CAM,
    keys on the host AND on the device, the image file's stamp), one CAM look-up each, the progress tick after the consumer's turn."""
    from irn_amd.step import _common, _labels
    events, args, model = _stub_label_worker(monkeypatch, _label_packs())
    with _labels.worker(0, model, [["a", "b"]], args) as w:
        got = []
        for p in _labels.items(w, args):
            got.append(p)
            events.append(("consumed", p["name"]))
    a, b = got
    assert set(a) == set(b) == {"name", "size", "img", "dev", "cam", "keys", "keys_dev", "stamp"}
    assert (a["name"], b["name"]) == ("2008_000001", "2008_000002")
    assert a["size"] == (6, 4) and b["size"] == (5, 7) and all(type(v) is int for v in a["size"] + b["size"])
    assert a["img"].shape == (6, 4, 3) and a["img"].dtype == torch.float32 and b["img"] is None
    assert a["dev"] == b["dev"] == torch.device("cuda", 0)
    assert (a["cam"], a["keys_dev"], b["cam"], b["keys_dev"]) == ("cam-2008_000001", "keys_dev-2008_000001", "cam-2008_000002", "keys_dev-2008_000002")
    assert a["keys"].tolist() == [3, 7]
    assert a["stamp"] == _common.image_stamp(args.voc12_root, "2008_000001") and b["stamp"][0].endswith("2008_000002.jpg")
    loop = [e for e in events if e[0] in ("cam", "consumed", "tick")]
    assert loop == [("cam", "2008_000001"), ("consumed", "2008_000001"), ("tick", 0, 1, 0, 2),
                    ("cam", "2008_000002"), ("consumed", "2008_000002"), ("tick", 0, 1, 1, 2)]


def test_semantic_step_hands_its_staging_buffer_back_on_an_exception(monkeypatch):
    """make_sem_seg_labels._work: when the loop dies with a batch in flight (here: the next image's CAM cannot be read), that
    batch's page-locked buffer goes back to _common.PINNED, walker and writer are closed and the error comes out; a run that
    ends well gives every buffer back exactly once."""
    from irn_amd import ops
    from irn_amd.step import _io, _labels, make_sem_seg_labels

    class _Pool:
        def __init__(self):
            self.taken, self.given = [], []

        def take(self, nbytes):
            self.taken.append(torch.zeros(max(int(nbytes), 1), dtype=torch.uint8))
            return self.taken[-1]

        def give(self, buf):
            self.given.append(buf)

    class _Done:
        def synchronize(self):
            pass

    def edges_for(model, pend, irn_batch, **kw):
        for p in pend:
            p["edge"] = "edge-" + p["name"]

    for fail_cam_at, n_taken in ((1, 1), (None, 2)):
        events, args, model = _stub_label_worker(monkeypatch, _label_packs(), fail_cam_at=fail_cam_at)
        pool = _Pool()
        monkeypatch.setattr(_io, "PINNED", pool)
        monkeypatch.setattr(_labels, "edges_for", edges_for)
        monkeypatch.setattr(ops, "label_epilogue", lambda rws, sizes, thres, keys=None, packed=False:
                            {"labels_flat": torch.zeros(sum(h * w for h, w in sizes), dtype=torch.uint8)})
        monkeypatch.setattr(ops, "read_back", lambda src, host, side: _Done())
        if fail_cam_at is None:
            make_sem_seg_labels._work(0, model, [["a", "b"]], args)
            assert [e for e in events if e[0] == "submit"] == [("submit", "2008_000001.png"), ("submit", "2008_000002.png")]
        else:
            with pytest.raises(OSError, match="no CAM file for 2008_000002"):
                make_sem_seg_labels._work(0, model, [["a", "b"]], args)
            assert ("walk", 1) in events and not [e for e in events if e[0] == "submit"]     # the batch was in flight, not collected
        assert len(pool.taken) == n_taken and len(pool.given) == n_taken
        assert all(g is t for g, t in zip(pool.given, pool.taken))
        assert events[-2:] == ["walker.close", "writer.close"]


def test_shard_io_hands_out_the_shard_and_closes_its_writer_however_the_block_ends(monkeypatch):
    events, args, _ = _stub_label_worker(monkeypatch, _label_packs())
    args.num_workers = 5
    seen = []
    monkeypatch.setattr(_io, "make_loader", lambda databin, num_workers, prefetch=4: seen.append((databin, num_workers)) or iter(()))
    monkeypatch.setattr(_io, "writer_threads", lambda args, n: seen.append(("writer_threads", n)) or 4)
    with _io.shard_io(1, [["x"], ["y", "z"]], args) as (databin, n, loader, writer):
        assert (databin, n) == (["y", "z"], 2) and list(loader) == [] and hasattr(writer, "submit")
        assert seen == [(["y", "z"], 5 // 2), ("writer_threads", 2)] and "writer.close" not in events
    assert events == ["writer.close"]
    del events[:]
    boom = RuntimeError("a bad image")
    with pytest.raises(RuntimeError) as info:
        with _io.shard_io(0, [["x"]], args):
            raise boom
    assert info.value is boom and events == ["writer.close"]
