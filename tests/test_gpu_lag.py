"""The batched entry points with the GPU lagging behind the host.

Every other GPU test makes one call on an idle device and reads the result: by the time the host returns, the device is
idle again, and the waits that protect reused host-side state (the descriptor ring of runtime.hip, the walk's tables and
staging slots, the augmentation's page-locked buffers, the deferred read-backs) never have anything to wait for.  Here a
bounded busy kernel (tests/_lag.py) keeps the device behind while a sequence of calls is enqueued, as a step enqueues them
behind the trunk.  Every sequence is run un-stalled first, each call alone between two synchronisations (this warms the
caches and gives the expected bits), then behind a stall: the bits must be the same, at least one call of every sequence
is also held to the CPU reference of the operator's own test module, and the per-call lag records show which calls
returned while the device was still busy and which waited.

Inputs are poison-filled device buffers (NaN, 255 for bytes, 0 for indices) that a copy enqueued BEHIND the stall, on the
stream under test, overwrites with the real data: work the library put on another stream, or ahead of the stall, reads
poison and fails the comparison.

Which guard each "returned only after the stall" assertion observes (it is never removed; the call is entered while the
device is asserted to lag, and returns with the stall over):
    test_descriptor_ring, call 5            runtime.hip scratch_upload: hipEventSynchronize of the slot used four calls ago
    test_label_entries, call 7              the same wait, through label.hip (irn_cam_merge passes its arguments by value and
                                            takes no slot: calls 2 and 5 do not count)
    test_walk_reconfigured, run B           walk.hip irn_walk_configure: hipEventSynchronize(run_done_ev)
    test_walk_reconfigured, run E           walk.hip irn_walk_run: hipEventSynchronize(stage_ev[slot]); two staging slots, so
                                            the third run of a shape (E) meets the slot of the first (C), not the second (D)
    test_augment_staging, call 2            augment.py _augment: staged.synchronize() before the pinned buffers are refilled

Asynchrony contract.  Asserted to return while the device lags (when they are not the fifth user of the ring):
find_centroids_batch, cluster_centroids_batch(k_on_device=True), label4, edge_to_affinity, bn_act_, upsample_bilinear,
stem_pool, msf_pack on cached sizes, a walk run on configured shapes.  Recorded, not asserted (measured on an MI355X):
    label_epilogue, label_sweep_confusion   return lagging (GPU keys, GPU thresholds)
    cam_merge                               returns lagging with a host label (the key list travels from pageable memory
                                            behind the stall: a few bytes, staged by the runtime)
    cam_confusion                           returns lagging with GPU keys and GPU thresholds; host keys or thresholds are a
                                            pageable upload
    augment_batch / augment_pair_batch      the first call returns lagging; every later one waits for the previous call's
                                            uploads (the page-locked staging buffers are reused)
    msf_pack on a new size                  blocks on the legacy default stream (the plan upload is a blocking copy, which that
                                            stream orders behind the stall); returns lagging on another stream
    walk run that reconfigures              blocks until the previous run is done (irn_walk_configure)
    detect_batch_count, and with it detect_instance_batch / _rle_batch / detection_overlap_batch
                                            block: the detection counts are read (the rle form reads the run counts too);
                                            `deferred=True` leaves only the last transfer in flight
    crf_filter, cluster_centroids, detect_instance (single-image forms, not used here) read a count and block
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle import irn_oracle as O
from oracle import msf_oracle as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_pair_ref as P  # noqa: E402
import _augment_ref as A  # noqa: E402
import _cocomask_ref as CR  # noqa: E402
import _detmap_overlap_ref as OR  # noqa: E402
import _label_cases as LC  # noqa: E402
import _label_sweep_ref as S  # noqa: E402
import _lag as L  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-5             # tests/test_gpu_walk.py: the walk against the exact (fp64) operator
GAP_MS = 3.0               # the short stall behind each call: later calls stay queued when earlier ones finish
F32 = np.float32


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


# ---------------------------------------------------------------------------------------------------------------------
# the second stream, and the proof that work on another stream would be seen
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def side_stream():
    """(the module's one extra stream, whether a kernel on the default stream overtakes a stall on it)."""
    dev = _dev()
    side = torch.cuda.Stream(device=dev)
    L.cycles_per_ms()
    canary = torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ev = L.stall(L.STALL_MIN_MS)
    canary.add_(1)                                          # default stream, while `side` is stalled
    done = torch.cuda.Event()
    done.record()
    while L.lagging(ev) and not done.query():               # bounded by the stall
        pass
    overtook = done.query() and L.lagging(ev)
    torch.cuda.synchronize()
    assert float(canary.item()) == 1.0
    print("lag: a kernel on the default stream %s a stall on the side stream" % ("overtakes" if overtook else "does NOT overtake"))
    return side, bool(overtook)


@pytest.fixture(params=["default", "side"])
def on_stream(request):
    """A context manager factory: the sequence runs on the legacy default stream or inside `torch.cuda.stream(side)`."""
    if request.param == "default":
        return contextlib.nullcontext
    side, overtook = request.getfixturevalue("side_stream")
    if not overtook:
        pytest.skip("the two streams share a hardware queue here: work on the wrong stream could not be told apart")
    return lambda: torch.cuda.stream(side)


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------

def _bits(x):
    """The exact content of a result: tensors and arrays as (dtype, shape, bytes), containers element by element."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple((k, _bits(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_bits(v) for v in x)
    if isinstance(x, Exception):
        return (type(x).__name__, str(x))
    return x


def _poison_like(t):
    if t.is_floating_point():
        return torch.full_like(t, float("nan"))
    if t.dtype == torch.uint8:
        return torch.full_like(t, 255)
    return torch.zeros_like(t)                              # indices and keys: in range, and wrong


def _fresh(real):
    return {k: _poison_like(v) for k, v in real.items()}


def _fill(bufs, real):
    for k, v in real.items():
        bufs[k].copy_(v)


def _warm(real, make_thunks):
    """Every call alone between two synchronisations, twice (the first pass fills the caches): -> (the results of the
    second pass as bits, the host time its calls took in ms)."""
    for _ in range(2):
        bufs = _fresh(real)
        _fill(bufs, real)
        want, host_ms = [], 0.0
        for _, thunk in make_thunks(bufs):
            torch.cuda.synchronize()
            out, ms = L.timed(thunk)
            torch.cuda.synchronize()
            want.append(_bits(out))
            host_ms += ms
    return want, host_ms


def _drive(what, real, make_thunks):
    """The sequence un-stalled, then behind a stall with a short stall behind every call.
    -> (results of the stalled run, their bits, the expected bits, the Behind with the lag records)."""
    want, host_ms = _warm(real, make_thunks)
    ms = L.stall_ms_for(host_ms)
    bufs = _fresh(real)
    thunks = make_thunks(bufs)
    torch.cuda.synchronize()
    got = []
    with L.Behind(ms) as b:
        _fill(bufs, real)
        for name, thunk in thunks:
            got.append(b.call(name, thunk))
            b.gap(GAP_MS)
    torch.cuda.synchronize()
    print("lag: %s: warm host time %.3f ms, stall %.0f ms" % (what, host_ms, ms))
    b.report(what)
    return got, [_bits(g) for g in got], want, b


def _assert_lagging(b, names):
    for name in names:
        lag = b.lags[name]
        assert lag.before and lag.after, "%s is documented not to wait for the device, but the stall was over when it %s (%r)" % (
            name, "returned" if lag.before else "was entered: the stall was too short", lag)


def _assert_waited(b, name):
    lag = b.lags[name]
    assert lag.before, "%s was entered with the stall already over: nothing was observed (%r)" % (name, lag)
    assert not lag.after, "%s returned while the device was still behind the stall: the wait that guards it is gone (%r)" % (name, lag)


def _noise_dp(h, w, seed):
    return (np.random.RandomState(seed).randn(2, h, w) * 2.0).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the descriptor ring of runtime.hip
# ---------------------------------------------------------------------------------------------------------------------

def test_descriptor_ring(on_stream):
    """Six users of the four-slot ring behind one stall: calls 1-4 return while the device lags, call 5 needs the slot of
    call 1 and returns only when the stall is over; all six tables reach their own kernels."""
    from irn_amd import ops
    from irn_amd.misc import indexing
    rng = np.random.RandomState(3)
    dps = {"dp_a": _noise_dp(12, 9, 1), "dp_b": _noise_dp(33, 37, 2), "dp_c": _noise_dp(17, 29, 3), "dp_e": _noise_dp(30, 23, 4)}
    mask3 = (rng.rand(3, 33, 37) < 0.55).astype(np.uint8)
    mask1 = (rng.rand(1, 8, 131) < 0.6).astype(np.uint8)
    edge = rng.rand(2, 20 * 27).astype(F32)
    cen_c = O.find_centroids_with_refinement(dps["dp_c"]).astype(np.int32)
    host = dict(dps, mask3=mask3, mask1=mask1, edge=edge, cen_c=cen_c)

    def make_thunks(d):
        return [("1 find_centroids_batch", lambda: ops.find_centroids_batch([d["dp_a"], d["dp_b"]], iterations=20)),
                ("2 label4", lambda: ops.label4(d["mask3"])),
                ("3 edge_to_affinity", lambda: indexing.edge_to_affinity(d["edge"], radius=5, size=(20, 27))),
                ("4 cluster_centroids_batch", lambda: ops.cluster_centroids_batch([d["cen_c"]], [d["dp_c"]], k_on_device=True)),
                ("5 find_centroids_batch", lambda: ops.find_centroids_batch([d["dp_e"]], iterations=20)),
                ("6 label4", lambda: ops.label4(d["mask1"]))]

    with on_stream():
        real = {k: _t(v) for k, v in host.items()}
        got, got_bits, want, b = _drive("descriptor ring", real, make_thunks)
        names = list(b.lags)
        _assert_lagging(b, names[:4])
        _assert_waited(b, names[4])
        for name, g, w in zip(names, got_bits, want):
            assert g == w, "%s: the result behind the stall differs from the un-stalled call" % name
        # the CPU references of tests/test_gpu_labels_instance.py and test_gpu_walk.py::test_edge_to_affinity_exact
        for cen, key in zip(got[0] + got[4], ("dp_a", "dp_b", "dp_e")):
            assert np.array_equal(cen.cpu().numpy(), O.find_centroids_with_refinement(host[key], iterations=20)), key
        for (labels, counts), m in ((got[1], mask3), (got[5], mask1)):
            for i in range(m.shape[0]):
                ref = O.label4(m[i].astype(bool))
                assert np.array_equal(labels[i].cpu().numpy(), ref) and int(counts[i]) == ref.max(), (m.shape, i)
        pio = O.PathIndexOracle(5, (20, 27))
        aff = got[2].cpu().numpy()
        for i in range(2):
            assert np.array_equal(aff[i], O.edge_to_affinity(edge[i], pio.path_indices)), i
        (cmap,), k = got[3]
        k = int(k.cpu()[0])
        ref_oh = O.cluster_centroids(cen_c, dps["dp_c"])
        oh = (cmap[None] == torch.arange(k, device=cmap.device, dtype=torch.int32)[:, None, None]).cpu().numpy()
        assert k >= 3 and oh.shape == ref_oh.shape and np.array_equal(oh, ref_oh.astype(bool))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the three ring users of label.hip
# ---------------------------------------------------------------------------------------------------------------------

def test_label_entries():
    """label_epilogue, cam_merge and label_sweep_confusion on ragged small cases behind one stall.  The epilogue and the
    sweep upload a job table through the ring; irn_cam_merge passes its arguments by value and takes no slot, so the fifth
    ring user is the seventh call."""
    from irn_amd import ops
    cases, merges = dict(LC.label_cases()), dict(LC.merge_cases())
    ep1 = [cases[n] for n in ("corner_5x7_at_0_0", "hot_seed5", "sign_mixed")]            # one threshold (0.25) per call
    ep2 = [c for _, c in LC.align_cases()][:4]                                            # 0.5, packed labels
    ep3 = [cases[n] for n in ("cropped_at_31_5_to_125x128", "corner_2x2_at_1_1")]
    sw = [cases[n] for n in ("plateau_two_equal_peaks", "corner_33x29_at_32_28_crop", "hot_seed6")]
    sw2 = [cases[n] for n in ("hot_seed0", "plateau_constant")]
    mg1, mg2 = merges["src_1xN"], merges["eight_scales"]
    gts = [S.ground_truth(c[1], seed=40 + i) for i, c in enumerate(sw)]
    gts2 = [S.ground_truth(c[1], seed=50 + i) for i, c in enumerate(sw2)]
    th, th2 = S.thresholds(sw[0][0], sw[0][1], 7, seed=1), S.thresholds(sw2[0][0], sw2[0][1], 5, seed=2)
    host = {}
    for tag, group in (("e1", ep1), ("e2", ep2), ("e3", ep3), ("sw", sw), ("s2", sw2)):
        for i, (rw, _, keys, _) in enumerate(group):
            host["%s_rw%d" % (tag, i)], host["%s_k%d" % (tag, i)] = rw, keys
    for tag, maps in (("sw", gts), ("s2", gts2)):
        for i, g in enumerate(maps):
            host["%s_gt%d" % (tag, i)] = g
    for tag, (outs, _, _) in (("m1", mg1), ("m2", mg2)):
        for i, o in enumerate(outs):
            host["%s_o%d" % (tag, i)] = o
    host["sw_th"], host["s2_th"] = th, th2

    def make_thunks(d):
        def epilogue(tag, group, packed):
            n = len(group)
            return lambda: ops.label_epilogue([d["%s_rw%d" % (tag, i)] for i in range(n)], [c[1] for c in group], group[0][3],
                                              keys=[d["%s_k%d" % (tag, i)] for i in range(n)], want_argmax=True, want_rw_up=True,
                                              packed=packed)

        def merge(tag, case):
            return lambda: ops.cam_merge([d["%s_o%d" % (tag, i)] for i in range(len(case[0]))], case[1], torch.from_numpy(case[2]))

        def sweep(tag, group):
            n = len(group)
            return lambda: ops.label_sweep_confusion([d["%s_rw%d" % (tag, i)] for i in range(n)], [c[1] for c in group],
                                                     [d["%s_k%d" % (tag, i)] for i in range(n)], [d["%s_gt%d" % (tag, i)] for i in range(n)],
                                                     d[tag + "_th"])

        return [("1 label_epilogue", epilogue("e1", ep1, False)), ("2 cam_merge", merge("m1", mg1)),
                ("3 label_sweep_confusion", sweep("sw", sw)), ("4 label_epilogue packed", epilogue("e2", ep2, True)),
                ("5 cam_merge", merge("m2", mg2)), ("6 label_sweep_confusion", sweep("s2", sw2)),
                ("7 label_epilogue", epilogue("e3", ep3, False))]

    real = {k: _t(v) for k, v in host.items()}
    got, got_bits, want, b = _drive("label entries", real, make_thunks)
    names = list(b.lags)
    _assert_lagging(b, names[:6])
    _assert_waited(b, names[6])                             # the ring's fifth user needs the slot of call 1
    for name, g, w in zip(names, got_bits, want):
        assert g == w, "%s: the result behind the stall differs from the un-stalled call" % name
    # the oracle of tests/test_gpu_label_epilogue.py, the restatement of tests/_label_sweep_ref.py
    for out, group in ((got[0], ep1), (got[3], ep2), (got[6], ep3)):
        for j, (rw, size, keys, bg) in enumerate(group):
            up, lab, idx = O.sem_seg_epilogue(rw, size, keys, bg)
            assert np.array_equal(out["rw_up"][j].cpu().numpy(), up, equal_nan=True), j
            assert np.array_equal(out["labels"][j].cpu().numpy(), lab) and np.array_equal(out["argmax"][j].cpu().numpy(), idx), j
    for (keys, cam, hi), (outs, size, label) in ((got[1], mg1), (got[4], mg2)):
        ref_keys, ref_cam, ref_hi = O.cam_merge(outs, size, label)
        assert np.array_equal(keys.cpu().numpy(), ref_keys)
        assert np.array_equal(cam.cpu().numpy(), ref_cam) and np.array_equal(hi.cpu().numpy(), ref_hi)
    for (hist, bad), group, maps, t in ((got[2], sw, gts, th), (got[5], sw2, gts2, th2)):
        want_hist, want_bad = 0, 0
        for (rw, size, keys, _), g in zip(group, maps):
            h_i, b_i = S.histogram(rw, size, keys, g, t)
            want_hist, want_bad = want_hist + h_i, want_bad + b_i
        assert int(bad.item()) == want_bad and np.array_equal(hist.cpu().numpy(), want_hist)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the walk, reconfigured under lag
# ---------------------------------------------------------------------------------------------------------------------

SHAPES_A, SHAPES_B = [(33, 37, 2), (20, 20, 1)], [(30, 23, 3)]


def _walk_inputs(shapes, seed0):
    from irn_amd import synth
    return ([synth.edge_field(h, w, seed=seed0 + i) for i, (h, w, c) in enumerate(shapes)],
            [synth.cam_blobs(c, h, w, seed=seed0 + i) for i, (h, w, c) in enumerate(shapes)])


def _walk_reconfigured(r, variant):
    from irn_amd.misc import indexing
    dev = _dev()
    runs = {"A": (SHAPES_A, _walk_inputs(SHAPES_A, 10)), "B": (SHAPES_B, _walk_inputs(SHAPES_B, 20)),
            "C": (SHAPES_B, _walk_inputs(SHAPES_B, 30))}
    runs["D"], runs["E"] = runs["B"], runs["C"]             # D: B again; E: a later run on the same shapes
    real = {n: ([_t(e) for e in es], [_t(c) for c in cs]) for n, (_, (es, cs)) in runs.items() if n in "ABC"}
    real["D"], real["E"] = real["B"], real["C"]
    walker = indexing.RandomWalk(r, dev)
    walker.set_option("variant", variant)

    def buffers(name):
        es, cs = real[name]
        return ([_poison_like(e) for e in es], [_poison_like(c) for c in cs],
                [torch.full((c, 1, h, w), float("nan"), dtype=torch.float32, device=dev) for h, w, c in runs[name][0]])

    def fill(name, bufs):
        for dst, src in zip(bufs[0] + bufs[1], real[name][0] + real[name][1]):
            dst.copy_(src)

    def run(bufs):
        return walker(bufs[0], bufs[1], beta=10, n_sweeps=8, outs=bufs[2])

    # un-stalled, one at a time; A last, so that the walker is configured for A when the stall begins
    want, host_ms = {}, 0.0
    for _ in range(2):
        host_ms = 0.0
        for name in "BCDEA":
            bufs = buffers(name)
            fill(name, bufs)
            torch.cuda.synchronize()
            outs, ms = L.timed(lambda: run(bufs))
            assert walker.sync() is False
            torch.cuda.synchronize()
            want[name] = [o.clone() for o in outs]
            host_ms += ms
    ms = L.stall_ms_for(host_ms)
    bufs = {name: buffers(name) for name in "ABCDE"}
    torch.cuda.synchronize()
    got = {}
    with L.Behind(ms) as b:
        for name in "AB":
            fill(name, bufs[name])
        for name in "AB":
            got[name] = b.call(name, lambda: run(bufs[name]))
        b.restall()
        for name in "CDE":
            fill(name, bufs[name])
        for name in "CDE":
            got[name] = b.call(name, lambda: run(bufs[name]))
    fell = walker.sync()
    torch.cuda.synchronize()
    print("lag: walk r=%d variant=%d: warm host time %.3f ms, stall %.0f ms (twice)" % (r, variant, host_ms, ms))
    b.report("walk r=%d variant=%d" % (r, variant))
    _assert_lagging(b, ["A"])                               # a run on configured shapes waits for nothing
    _assert_waited(b, "B")                                  # irn_walk_configure: the tables are still A's
    _assert_lagging(b, ["C", "D"])                          # no reconfiguration; their staging slots are free
    _assert_waited(b, "E")                                  # irn_walk_run: E's staging slot is C's, and C is behind the stall
    if variant == 2:
        assert fell is False and walker.fallback_runs == 0
    for name in "ABCDE":
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert _bits(g) == _bits(w), "run %s image %d: behind the stall differs from the un-stalled run" % (name, i)
    if variant == 0:
        for name in "AB":
            es, cs = runs[name][1]
            for i, g in enumerate(got[name]):
                st = O.propagate_to_edge_stencil(cs[i], es[i], r, 10, 3)
                err = float(np.abs(g.cpu().numpy() - st).max())
                assert err <= TOL_F64, (name, i, err)
    walker.close()


@pytest.mark.parametrize("variant", [2, 0])
@pytest.mark.parametrize("r", [5, 10])
def test_walk_reconfigured(r, variant):
    _walk_reconfigured(r, variant)


def test_walk_reconfigured_on_a_side_stream(side_stream):
    side, overtook = side_stream
    if not overtook:
        pytest.skip("the two streams share a hardware queue here: work on the wrong stream could not be told apart")
    with torch.cuda.stream(side):
        _walk_reconfigured(10, 2)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the page-locked staging of the augmentation
# ---------------------------------------------------------------------------------------------------------------------

def test_augment_staging():
    """augment_batch twice back to back from host images (the cached pinned `aug_pixels` / `aug_meta` buffers), then
    augment_pair_batch: the second call may refill the buffers only when the first call's uploads have run."""
    from irn_amd import ops
    dev = _dev()
    crop = 32
    rng = np.random.default_rng(9)

    def batch(picks):
        imgs, params = [], []
        for k, (s, target, flip) in enumerate(picks):
            h, w = A.SHAPES[s][:2]
            imgs.append(A.image(h, w, 10 * s + k))
            params.append(A.params_for(h, w, crop, target, flip, "drawn", rng))
        return imgs, params

    b1 = batch([(0, 40, 1), (1, 64, 0)])
    b2 = batch([(2, 60, 0), (3, 100, 1), (0, 20, 0)])
    pc = [P.cases([P.SHAPES[s]])[k] for s, k in ((0, 7), (1, 3), (2, 12))]
    pair_imgs = [P.image(h, w, i) for i, (h, w, _, _) in enumerate(pc)]
    pair_labs = [P.label(h, w, i) for i, (h, w, _, _) in enumerate(pc)]
    pair_params, pair_crop = [c[3] for c in pc], pc[0][2]
    assert len({c[2] for c in pc}) == 1

    def outs():
        g = pair_crop // 4
        return (torch.full((2, 3, crop, crop), float("nan"), device=dev), torch.full((3, 3, crop, crop), float("nan"), device=dev),
                torch.full((3, 3, pair_crop, pair_crop), float("nan"), device=dev), torch.full((3, g, g), 7, dtype=torch.uint8, device=dev))

    def make_thunks(o):
        ti = lambda imgs: [torch.from_numpy(im) for im in imgs]
        return [("1 augment_batch", lambda: ops.augment_batch(ti(b1[0]), b1[1], crop, device=dev, out=o[0])),
                ("2 augment_batch", lambda: ops.augment_batch(ti(b2[0]), b2[1], crop, device=dev, out=o[1])),
                ("3 augment_pair_batch", lambda: ops.augment_pair_batch(ti(pair_imgs), ti(pair_labs), pair_params, pair_crop, reduce=4,
                                                                        device=dev, out=o[2], out_label=o[3]))]

    for _ in range(2):
        want, host_ms = [], 0.0
        for _, thunk in make_thunks(outs()):
            torch.cuda.synchronize()
            out, ms = L.timed(thunk)
            torch.cuda.synchronize()
            want.append(_bits(out))
            host_ms += ms
    ms = L.stall_ms_for(host_ms)
    o = outs()
    torch.cuda.synchronize()
    got, b = L.run_behind(make_thunks(o), ms)
    torch.cuda.synchronize()
    print("lag: augment staging: warm host time %.3f ms, stall %.0f ms" % (host_ms, ms))
    b.report("augment staging")
    _assert_waited(b, "2 augment_batch")                    # augment.py: staged.synchronize()
    for name, g, w in zip(b.lags, got, want):
        assert _bits(g) == w, name
    for out, (imgs, params) in ((got[0], b1), (got[1], b2)):
        ref = np.stack([A.augment_ref(im, p, crop) for im, p in zip(imgs, params)])
        assert _bits(out) == _bits(ref)
    ref_img = np.stack([P.augment_ref(im, p, pair_crop) for im, p in zip(pair_imgs, pair_params)])
    ref_lab = np.stack([P.label_ref(lb, p, pair_crop, 4) for lb, p in zip(pair_labs, pair_params)])
    assert _bits(got[2][0]) == _bits(ref_img) and _bits(got[2][1]) == _bits(ref_lab)


# ---------------------------------------------------------------------------------------------------------------------
# 5. deferred read-backs
# ---------------------------------------------------------------------------------------------------------------------

def _kron(rng, h, w, c, p_bg):
    cls = np.kron(rng.randint(0, c + 1, size=((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), int))[:h, :w]
    cls[rng.rand(h, w) < p_bg] = 0
    return cls.astype(np.int32)


def _det_batch(rng, specs):
    """[(score, class map, class ids, channels, min area)] as tests/test_gpu_labels_instance.py builds its batches."""
    return [(rng.rand(c, h, w).astype(F32), _kron(rng, h, w, c, p_bg), np.arange(50, 50 + c), c, thr) for h, w, c, p_bg, thr in specs]


def _det_oracle(im):
    score, cls, cids, c, thr = im
    one_hot = np.stack([cls == k + 1 for k in range(c)])
    return O.detect_instance(score, one_hot, cids, max_fragment_size=thr)


@pytest.mark.parametrize("kind", ["dense", "rle", "overlap"])
def test_deferred_read_back(kind):
    """Batch A's detections with the last transfer deferred, behind a stall; batch B's labelling enqueued; then A.result()."""
    from irn_amd import ops
    dev = _dev()
    rng = np.random.RandomState(11)
    if kind == "overlap":
        from test_gpu_detmap_overlap import _image
        imgs = [_image(1, 33, 65, 2, 3), _image(2, 17, 65, 2, 4), _image(3, 40, 28, 4, 2)]
        imgs[1]["am"][:] = 0                                # the image without detections
        batch_a = [(im["rw"], im["am"], im["class_ids"], im["n_ch"], im["min_area"]) for im in imgs]
    else:
        batch_a = _det_batch(rng, [(37, 41, 5, 0.4, 0.0), (16, 16, 2, 1.0, 0.0), (24, 30, 12, 0.2, 6.5)])
    batch_b = _det_batch(rng, [(20, 24, 3, 0.3, 0.0), (16, 28, 1, 0.0, 0.0)])
    real = {}
    for tag, batch in (("a", batch_a), ("b", batch_b)):
        for i, im in enumerate(batch):
            real["%s_sc%d" % (tag, i)], real["%s_am%d" % (tag, i)] = _t(im[0]), _t(im[1])
    if kind == "overlap":
        for i, im in enumerate(imgs):
            real["a_in%d" % i] = _t(im["inst"])

    def args(d, tag, batch):
        n = len(batch)
        return ([d["%s_sc%d" % (tag, i)] for i in range(n)], [d["%s_am%d" % (tag, i)] for i in range(n)], [im[2] for im in batch],
                [im[3] for im in batch], [im[4] for im in batch])

    def call_a(d, bad, **kw):
        if kind == "dense":
            return ops.detect_instance_batch(*args(d, "a", batch_a), **kw)
        if kind == "rle":
            return ops.detect_instance_rle_batch(*args(d, "a", batch_a), **kw)
        return ops.detection_overlap_batch(*args(d, "a", batch_a), [d["a_in%d" % i] for i in range(len(imgs))],
                                           [im["g"] for im in imgs], bad, **kw)

    def count_b(d):
        sc, am, _, n_ch, _ = args(d, "b", batch_b)
        return ops.detect_batch_count(sc, am, n_ch).nds

    def new_bad():
        return torch.zeros(1, dtype=torch.int64, device=dev)

    host_ms = 0.0
    for _ in range(2):                                      # blocking, then deferred, un-stalled
        torch.cuda.synchronize()
        want = call_a(real, new_bad())
        torch.cuda.synchronize()
        pending, ms_a = L.timed(lambda: call_a(real, new_bad(), deferred=True))
        want_nds, ms_b = L.timed(lambda: count_b(real))
        warm, ms_r = L.timed(pending.result)
        torch.cuda.synchronize()
        host_ms = ms_a + ms_b + ms_r
    assert _bits(warm) == _bits(want)
    ms = L.stall_ms_for(host_ms)
    bufs, bad = _fresh(real), new_bad()
    torch.cuda.synchronize()
    with L.Behind(ms) as b:
        _fill(bufs, real)
        pending = b.call("A deferred", lambda: call_a(bufs, bad, deferred=True))
        nds_b = b.call("B detect_batch_count", lambda: count_b(bufs))
        got = b.call("A.result()", pending.result)
    torch.cuda.synchronize()
    print("lag: deferred %s: warm host time %.3f ms, stall %.0f ms" % (kind, host_ms, ms))
    b.report("deferred " + kind)
    assert b.lags["A deferred"].before
    assert nds_b == want_nds and sum(nds_b) > 0
    assert _bits(got) == _bits(want), "the deferred result behind the stall differs from the blocking call"
    # the restatements of tests/test_gpu_labels_instance.py, test_gpu_ins_rle.py and test_gpu_detmap_overlap.py
    assert len(got) == len(batch_a)
    if kind == "overlap":
        assert int(bad.item()) == sum(int((im["inst"] > im["g"]).sum()) for im in imgs)
        assert len(got[1]["pred_score"]) == 0 and got[1]["area_gt"].sum() > 0
        for im, rec in zip(imgs, got):
            ref, _ = OR.overlap(im["rw"], im["am"], im["n_ch"], im["min_area"], im["inst"], im["g"])
            ref["pred_class"] = im["class_ids"][ref.pop("channel")]
            assert _bits(rec) == _bits(ref)
        return
    assert isinstance(got[1], ValueError)
    for i in (0, 2):
        ref = _det_oracle(batch_a[i])
        masks = np.asarray(ref["mask"]).astype(bool)
        assert np.array_equal(got[i]["class"], ref["class"]) and np.array_equal(got[i]["score"], np.asarray(ref["score"], F32)), i
        if kind == "dense":
            assert got[i]["mask"].shape == masks.shape and np.array_equal(got[i]["mask"], masks), i
        else:
            counts, offsets, area, bbox = CR.mask_rle(masks)
            assert tuple(got[i]["size"]) == masks.shape[1:]
            for key, ref_v in (("counts", counts), ("offsets", offsets), ("area", area), ("bbox", bbox)):
                assert np.array_equal(got[i][key], ref_v), (i, key)


# ---------------------------------------------------------------------------------------------------------------------
# 6. accumulators and the input pipeline
# ---------------------------------------------------------------------------------------------------------------------

MSF_SCALES = (1.0, 0.5, 1.5)
MSF_NEW = {"default": (15, 19), "side": (13, 22)}           # a size whose plans no earlier call of the process has built


def _want_cam(cams, keys, gt, th):
    """tests/test_gpu_eval.py::_want_cam."""
    conf = np.zeros((len(th), 21, 21), np.int64)
    void = np.zeros((len(th), 21), np.int64)
    keys_pad = np.pad(np.asarray(keys) + 1, (1, 0), mode="constant")
    g = gt.astype(np.int64)
    for i, t in enumerate(th):
        pred = keys_pad[np.argmax(np.pad(cams, ((1, 0), (0, 0), (0, 0)), mode="constant", constant_values=t), axis=0)]
        m = g != 255
        np.add.at(conf[i], (g[m], pred[m]), 1)
        np.add.at(void[i], pred[~m], 1)
    return conf, void


def test_accumulators_and_input_pipeline(on_stream, request):
    from irn_amd import ops
    rng = np.random.RandomState(5)
    g = torch.Generator().manual_seed(31)
    x = torch.randn((3, 5, 7, 9), generator=g).numpy()
    scale, shift = (torch.rand(5, generator=g) * 2 - 0.5).numpy(), torch.randn(5, generator=g).numpy()
    xs = torch.randn((2, 5, 2, 3), generator=g).numpy()
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((11, 14), (9, 23))]
    new_hw = MSF_NEW["side" if "side" in request.node.name else "default"]
    img_new = rng.randint(0, 256, new_hw + (3,)).astype(np.uint8)
    th = np.unique(np.concatenate([F32([0.0, 0.125, 0.25, 0.5, 1.0]), rng.rand(100).astype(F32)]))[:100]
    cam_cases = []
    for h, w, k in ((13, 17, 2), (9, 20, 0), (21, 11, 5)):
        gt = rng.randint(0, 21, (h, w)).astype(np.uint8)
        gt[rng.rand(h, w) < 0.1] = 255
        cams = np.where(rng.rand(k, h, w) < 0.5, rng.choice(th[:6], (k, h, w)), rng.rand(k, h, w)).astype(F32)
        cam_cases.append((cams, np.sort(rng.choice(20, k, replace=False)).astype(np.int64), gt))
    host = {"x": x, "scale": scale, "shift": shift, "xs": xs, "img0": imgs[0], "img1": imgs[1], "th": th}
    for i, (cams, keys, gt) in enumerate(cam_cases):
        host["cam%d" % i], host["key%d" % i], host["gt%d" % i] = cams, keys, gt

    def make_thunks(d):
        st = {}

        def bn():
            st["y"] = ops.bn_act_(d["x"], d["scale"], d["shift"], None, True)
            return st["y"]

        def confusion(i):
            def thunk():
                st["hist"], st["bad"] = ops.cam_confusion(d["cam%d" % i], d["key%d" % i], d["gt%d" % i], d["th"], st.get("hist"), st.get("bad"))
                return st["hist"].clone(), st["bad"].clone()
            return thunk

        return [("bn_act_", bn), ("upsample_bilinear", lambda: ops.upsample_bilinear(st["y"], 2)),
                ("stem_pool", lambda: ops.stem_pool(d["xs"], d["scale"], d["shift"])),
                ("msf_pack cached 0", lambda: ops.msf_pack(d["img0"], MSF_SCALES)),
                ("msf_pack cached 1", lambda: ops.msf_pack(d["img1"], MSF_SCALES)),
                ("cam_confusion 0", confusion(0)), ("cam_confusion 1", confusion(1)), ("cam_confusion 2", confusion(2))]

    with on_stream():
        real = {k: _t(v) for k, v in host.items()}
        new_dev = _t(img_new)
        want, host_ms = _warm(real, make_thunks)
        ms = L.stall_ms_for(host_ms)
        bufs, new_buf = _fresh(real), _poison_like(new_dev)
        thunks = make_thunks(bufs) + [("msf_pack new size", lambda: ops.msf_pack(new_buf, MSF_SCALES))]
        torch.cuda.synchronize()
        got = []
        with L.Behind(ms) as b:
            _fill(bufs, real)
            new_buf.copy_(new_dev)
            for name, thunk in thunks:
                got.append(b.call(name, thunk))
                b.gap(GAP_MS)
        torch.cuda.synchronize()
        print("lag: accumulators and input pipeline: warm host time %.3f ms, stall %.0f ms" % (host_ms, ms))
        b.report("accumulators and input pipeline")
        names = list(b.lags)
        _assert_lagging(b, names[:5])
        for name, gb, w in zip(names, got, want):
            assert _bits(gb) == w, "%s: the result behind the stall differs from the un-stalled call" % name
        # the exact expressions of tests/test_gpu_bn_act.py
        xt, sc, sh = torch.from_numpy(x), torch.from_numpy(scale), torch.from_numpy(shift)
        fma32 = (xt.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float()
        y = torch.clamp_min(fma32, 0)
        assert got[0].data_ptr() == bufs["x"].data_ptr() and torch.equal(got[0].cpu(), y)
        assert _bits(got[1]) == _bits(_upsample_exact(y.numpy(), 2))
        fs = (torch.from_numpy(xs).double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float()
        assert torch.equal(got[2].cpu(), torch.nn.functional.max_pool2d(torch.clamp_min(fs, 0), 3, 2, 1))
        for out, img in ((got[3], imgs[0]), (got[4], imgs[1]), (got[8], img_new)):
            for o, ref in zip(out, M.msf_item(img, MSF_SCALES)):
                assert o.dtype == torch.float32 and np.array_equal(o.cpu().numpy(), ref), img.shape
        want_conf = want_void = 0
        for i, (cams, keys, gt) in enumerate(cam_cases):
            c, v = _want_cam(cams, keys, gt, th)
            want_conf, want_void = want_conf + c, want_void + v
            hist, bad = got[5 + i]
            conf, void = ops.cam_confusion_matrices(hist)
            assert int(bad.item()) == 0
            assert np.array_equal(conf.cpu().numpy(), want_conf) and np.array_equal(void.cpu().numpy(), want_void), i


def _upsample_exact(a, factor):
    """The documented expression of irn_upsample_bilinear, as tests/test_gpu_bn_act.py states it."""
    h, w = a.shape[-2:]
    r = F32(1.0 / factor)

    def axis(n_out, n_in):
        src = np.maximum(r * (np.arange(n_out, dtype=F32) + F32(0.5)) - F32(0.5), F32(0)).astype(F32)
        i0 = src.astype(np.int64)
        return i0, i0 + (i0 < n_in - 1), (src - i0.astype(F32)).astype(F32)

    y0, y1, ly = axis(h * factor, h)
    x0, x1, lx = axis(w * factor, w)
    ly, lx = ly[:, None], lx[None, :]
    one = F32(1)
    top = (one - lx) * a[..., y0[:, None], x0[None, :]] + lx * a[..., y0[:, None], x1[None, :]]
    bot = (one - lx) * a[..., y1[:, None], x0[None, :]] + lx * a[..., y1[:, None], x1[None, :]]
    return ((one - ly) * top + ly * bot).astype(F32)
