"""One image-to-label chain on the reference's own composition: make_cam -> make_sem_seg_labels -> make_ins_seg_labels of the
product, in-process, on the two images of tests/golden/chain.npz — the pixels, weights and settings the reference itself was run
on (step/make_cam.py:26-56, step/make_sem_seg_labels.py:28-51, the instance branch of step/make_ins_seg_labels.py) — checked stage
by stage against what the reference computed, so that a failure names its stage.  Every stage has its own test on its own inputs;
this one is about the seams between them: scale rounding and the flip pair of the multi-scale item, the strided / strided-up
crops, keys + 1, IRNet's crop on a ragged size, which trunk pass an image of a given size takes (image a: the tuned channels-last
16-row passes at all four scales; image b: NCHW), and the hand-off of CAMs and edge maps in device memory between the steps.

Bars (tests/_chain.py): 1e-4 per stage on CAM / high_res / edge / dp (the project's per-stage bar); delta = 4 * d_rw_up on the
normalised upsampled scores, d_rw_up being the reference's own float32-vs-float64 distance there, measured by the generator;
labels may differ only at ties of the REFERENCE's score stack closer than 2 * delta, and no more of them than it has such ties.

Measured on MI355X with the committed fixture (image a = 281x500, seed 717, three classes, one instance; image b = 101x178, seed
803, one class, two instances; both carry the instance branch), split-precision trunk / fp32 trunk, distance to the reference:
    a  cam 9.2e-6 / 1.3e-5   edge 8.3e-7 / 1.1e-6   dp 7.2e-6 / 8.1e-6   rw_up 4.4e-5 / 4.3e-5 (delta 1.7e-4), instance rw_up the same
    b  cam 2.6e-5 / 2.6e-5   high_res 2.6e-5 / 2.6e-5   edge 1.5e-6 / 2.0e-6   dp 1.4e-5 / 1.1e-5   rw_up 2.8e-5 / 2.8e-5 (delta 1.1e-4),
       instance rw_up 2.9e-5 / 2.9e-5 (delta_ins 1.1e-4)
    (the reference's own float32-vs-float64 distances: a  d_cam 8.6e-6 d_edge 4.4e-7 d_dp 4.4e-6 d_rw_up 4.3e-5;
     b  d_cam 2.5e-5 d_edge 8.6e-7 d_dp 7.7e-6 d_rw_up 2.7e-5 d_rw_up_ins 2.7e-5)
    no label pixel and no instance-class pixel differs in either mode (the reference has 131 / 3 ties at 2 delta, 131 / 1 in the
    instance stacks); centroids, instance maps, detection counts (8 / 3) and classes equal.  The test prints the figures of its run."""
import argparse
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _chain
from _parity import label_mismatches

pytestmark = pytest.mark.gpu

NAMES = {"a": "2009_000001", "b": "2009_000002"}
STAGE_BAR = 1e-4


def _make_voc(tmp, fx):
    """A VOC-shaped tree holding the fixture's two images, written LOSSLESSLY: PNG-encoded bytes at the .jpg path the loader opens
    (PIL detects the format by content), so the pixels the product sees are the fixture's on every machine."""
    root = tmp / "voc"
    (root / "JPEGImages").mkdir(parents=True)
    labels = {}
    for n in _chain.IMAGES:
        img = _chain.photo(fx, n)
        path = root / "JPEGImages" / (NAMES[n] + ".jpg")
        Image.fromarray(img).save(path, format="PNG")
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img)
        labels[int(NAMES[n].replace("_", ""))] = fx[n + "_label"].astype(np.float32)
    (tmp / "lists").mkdir()
    (tmp / "lists" / "train.txt").write_text("\n".join(NAMES[n] for n in _chain.IMAGES) + "\n")
    np.save(tmp / "lists" / "cls_labels.npy", labels)
    return root


class _Capture:
    """Records what the label steps computed between their stages and do not write: the normalised upsampled scores of the
    semantic step (one more `label_epilogue` call on the step's own walk result, with the score output on), the scores and argmax
    maps of the instance step (its own call's outputs), and the centroids / instance maps of the instance front-end."""

    def __init__(self, monkeypatch, ops):
        self.sem, self.ins, self.front = None, None, None
        epilogue, cluster = ops.label_epilogue, ops.cluster_centroids_batch

        def label_epilogue(rws, sizes, bg, **kw):
            out = epilogue(rws, sizes, bg, **kw)
            key = [tuple(int(v) for v in s_) for s_ in sizes]                  # images are told apart by their (distinct) sizes
            if kw.get("want_rw_up"):
                self.ins = {k: {"rw_up": u.clone(), "argmax": a.clone()} for k, u, a in zip(key, out["rw_up"], out["argmax"])}
            else:
                again = epilogue(rws, sizes, bg, keys=kw["keys"], want_rw_up=True)
                self.sem = {k: {"rw_up": u, "labels": l} for k, u, l in zip(key, again["rw_up"], again["labels"])}
            return out

        def cluster_centroids_batch(centroids, dps, **kw):
            cmaps, k = cluster(centroids, dps, **kw)
            self.front = {tuple(m.shape): {"centroids": c.clone(), "cmap": m} for c, m in zip(centroids, cmaps)}
            return cmaps, k

        monkeypatch.setattr(ops, "label_epilogue", label_epilogue)
        monkeypatch.setattr(ops, "cluster_centroids_batch", cluster_centroids_batch)


@pytest.mark.parametrize("trunk", ["split", "fp32"])
def test_chain_matches_the_reference_stage_by_stage(tmp_path, monkeypatch, trunk):
    from irn_amd import ops
    from irn_amd.net import resnet50 as r50, weights
    from irn_amd.step import _common, make_cam, make_ins_seg_labels, make_sem_seg_labels
    from oracle import irn_oracle as O
    fx = _chain.load()
    bg = float(fx["bg"])
    monkeypatch.setattr(r50, "SPLIT_GEMM", trunk == "split")
    root = _make_voc(tmp_path, fx)
    torch.save(weights.random_cam_state(1), tmp_path / "res50_cam.pth")
    torch.save(weights.random_irn_state(2), tmp_path / "res50_irn.pth")
    args = argparse.Namespace(
        num_workers=0, voc12_root=str(root), train_list=str(tmp_path / "lists" / "train.txt"),
        infer_list=str(tmp_path / "lists" / "train.txt"), cam_network="net.resnet50_cam",
        cam_weights_name=str(tmp_path / "res50_cam"), cam_scales=tuple(float(s) for s in fx["scales"]),
        irn_network="net.resnet50_irn", irn_weights_name=str(tmp_path / "res50_irn.pth"),
        beta=10, exp_times=8, sem_seg_bg_thres=bg, ins_seg_bg_thres=bg,
        cam_out_dir=str(tmp_path / "cam"), sem_seg_out_dir=str(tmp_path / "sem"),
        ins_seg_out_dir=str(tmp_path / "ins"), edge_out_dir=str(tmp_path / "edge"))
    for d in (args.cam_out_dir, args.sem_seg_out_dir, args.ins_seg_out_dir):
        os.makedirs(d)

    cap = _Capture(monkeypatch, ops)
    passes, count_pass = {True: set(), False: set()}, r50.count_pass

    def record_pass(x, channels_last):                 # the step reports and resets net/resnet50.PASS_STATS itself: listen in
        passes[bool(channels_last)].add("%dx%d" % (int(x.shape[2]), int(x.shape[3])))
        return count_pass(x, channels_last)
    monkeypatch.setattr(r50, "count_pass", record_pass)
    make_cam.run(args)
    nchw = passes[False]
    hits0 = _common.CAM_STORE.hits
    make_sem_seg_labels.run(args)
    assert _common.CAM_STORE.hits - hits0 == len(NAMES)                    # the CAMs came from device memory, not the files
    e_hits0 = _common.EDGE_STORE.hits
    make_ins_seg_labels.run(args)
    assert _common.EDGE_STORE.hits - e_hits0 == len(NAMES)                 # ... and the edge / displacement maps too
    assert cap.sem is not None and cap.ins is not None and cap.front is not None

    # which trunk pass each image took: a's four scales are sizes the shipped database is tuned for (channels-last, 16 rows a
    # pass) wherever that database is in use; none of b's is
    def scaled(n):
        h, w = _chain.size(fx, n)
        return {"%dx%d" % (int(np.round(h * s)), int(np.round(w * s))) for s in args.cam_scales}
    print("chain [%s]: NCHW trunk passes at %s" % (trunk, sorted(nchw)))
    assert scaled("b") <= nchw, (scaled("b"), nchw)
    if (16,) + _chain.size(fx, "a") in r50.tuned_nhwc_shapes() and os.environ.get("IRN_MIOPEN_DB_SET"):
        assert not (scaled("a") & nchw) and scaled("a") <= passes[True], (scaled("a"), passes)

    problems = []

    def check(ok, msg):
        if not ok:
            problems.append(msg)

    for n in _chain.IMAGES:
        tag = "chain [%s] image %s" % (trunk, n)
        H, W = _chain.size(fx, n)
        keys = fx[n + "_keys"]
        lut = np.concatenate([[0], keys + 1])
        # --- make_cam
        d = np.load(os.path.join(args.cam_out_dir, NAMES[n] + ".npy"), allow_pickle=True).item()
        check(np.array_equal(d["keys"].numpy(), keys), "%s keys: %s, reference %s" % (tag, d["keys"].tolist(), keys.tolist()))
        assert d["cam"].shape == fx[n + "_cam"].shape and d["high_res"].shape == (len(keys), H, W), tag
        dist = {"cam": float(np.abs(d["cam"].numpy() - fx[n + "_cam"]).max())}
        if n + "_high_res" in fx:
            dist["high_res"] = float(np.abs(d["high_res"] - fx[n + "_high_res"]).max())
        # --- IRNet
        e = np.load(os.path.join(args.edge_out_dir, NAMES[n] + ".npy"), allow_pickle=True).item()
        assert e["edge"].shape == fx[n + "_edge"].shape and e["dp"].shape == fx[n + "_dp"].shape, tag
        dist["edge"] = float(np.abs(e["edge"] - fx[n + "_edge"]).max())
        dist["dp"] = float(np.abs(e["dp"] - fx[n + "_dp"]).max())
        for k, v in dist.items():
            check(v <= STAGE_BAR, "%s %s: %.3g from the reference, bar %.0e" % (tag, k, v, STAGE_BAR))
        # --- walk + epilogue: normalised upsampled scores
        delta = _chain.MARGIN * float(fx[n + "_d_rw_up"])
        up_ref, label_ref, _ = O.sem_seg_epilogue(fx[n + "_rw"], (H, W), keys, bg)
        assert np.array_equal(label_ref, fx[n + "_label_map"])
        up = cap.sem[(H, W)]["rw_up"].cpu().numpy()
        d_up = float(np.abs(up - up_ref).max())
        check(d_up <= delta, "%s rw_up: %.3g from the reference, bar delta = 4 d_rw_up = %.3g" % (tag, d_up, delta))
        # --- labels: the step's file
        png = np.asarray(Image.open(os.path.join(args.sem_seg_out_dir, NAMES[n] + ".png")))
        assert png.dtype == np.uint8 and png.shape == (H, W), tag
        check(np.array_equal(png, cap.sem[(H, W)]["labels"].cpu().numpy()), "%s: the label file is not the argmax of the captured scores" % tag)
        ties = _chain.tie_count(up_ref, bg, delta)
        n_diff = -1
        try:
            n_diff, _gap = label_mismatches(png, label_ref, up_ref, bg, lut=lut, what=tag + " labels", tol=2 * delta)
            check(n_diff <= ties, "%s labels: %d pixels differ, the reference has only %d ties at 2 delta" % (tag, n_diff, ties))
        except AssertionError as exc:
            problems.append(str(exc))
        print("%s: cam %.2e%s edge %.2e dp %.2e (bar 1e-4; reference's own d %.1e / %.1e / %.1e); rw_up %.2e (delta %.2e); "
              "%d of %d label pixels differ (%d ties at 2 delta)" % (
                  tag, dist["cam"], " high_res %.2e" % dist["high_res"] if "high_res" in dist else "", dist["edge"], dist["dp"],
                  float(fx[n + "_d_cam"]), float(fx[n + "_d_edge"]), float(fx[n + "_d_dp"]), d_up, delta, int((png != label_ref).sum()), H * W, ties))
        # --- instance branch
        if not _chain.has_instances(fx, n):
            continue
        inst = _chain.instance_map(fx, n)
        front = cap.front[fx[n + "_edge"].shape[1:]]
        cen, cmap = front["centroids"].cpu().numpy(), front["cmap"].cpu().numpy()
        check(np.array_equal(cen, fx[n + "_centroids"]), "%s centroids: %d grid cells differ" % (tag, int((cen != fx[n + "_centroids"]).any(0).sum())))
        same_map = int(cmap.max()) + 1 == inst.shape[0] and np.array_equal(cmap, np.argmax(inst, 0))
        check(same_map, "%s instance map differs (K = %d, reference %d)" % (tag, int(cmap.max()) + 1, inst.shape[0]))
        if not same_map:
            continue                                                        # another channel layout: nothing below is comparable
        delta_i = _chain.MARGIN * float(fx[n + "_d_rw_up_ins"])
        up_i_ref, _, idx_ref = O.sem_seg_epilogue(fx[n + "_rw_ins"], (H, W), np.zeros(fx[n + "_rw_ins"].shape[0], np.int64), bg)
        assert np.array_equal(idx_ref, fx[n + "_argmax"])
        up_i = cap.ins[(H, W)]["rw_up"].cpu().numpy()
        d_up_i = float(np.abs(up_i - up_i_ref).max())
        check(d_up_i <= delta_i, "%s instance rw_up: %.3g from the reference, bar delta_ins = %.3g" % (tag, d_up_i, delta_i))
        want = _chain.detections(fx, n)
        path = os.path.join(args.ins_seg_out_dir, NAMES[n] + ".npy")
        assert os.path.exists(path), tag + ": no instance file"
        det = np.load(path, allow_pickle=True).item()
        chan_class = np.concatenate([[0], np.repeat(keys, inst.shape[0]) + 1])
        ties_i = _chain.tie_count(up_i_ref, bg, delta_i)
        n_diff_i = -1
        try:
            n_diff_i, _gap = label_mismatches(_chain.paint(det), _chain.paint(want), up_i_ref, bg, lut=chan_class,
                                              what=tag + " instance classes", tol=2 * delta_i)
            check(n_diff_i <= ties_i, "%s instance classes: %d pixels differ, the reference has only %d ties" % (tag, n_diff_i, ties_i))
        except AssertionError as exc:
            problems.append(str(exc))
        if len(want["score"]) == len(det["score"]):
            check(np.array_equal(want["class"], det["class"]), "%s detection classes %s, reference %s" % (tag, det["class"], want["class"]))
            d_score = float(np.abs(want["score"] - det["score"]).max())
            check(d_score <= 1e-3, "%s detection scores: %.3g from the reference" % (tag, d_score))
        print("%s: centroids and instance map equal (K = %d); instance rw_up %.2e (delta_ins %.2e); %d instance-class pixels differ "
              "(%d ties); %d detections, reference %d" % (tag, inst.shape[0], d_up_i, delta_i, n_diff_i, ties_i, len(det["score"]), len(want["score"])))
    assert not problems, "\n".join(problems)
