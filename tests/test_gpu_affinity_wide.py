"""The walk's weight planes from the unrolled affinity kernel (radius 5 and 10, integer beta: several pixels per lane,
wide LDS reads, wide stores, the planes' pads zeroed in the same launch) against the oracle's weights: bit for bit."""
import numpy as np
import pytest
import torch

from oracle import irn_oracle as O

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-5      # test_gpu_walk.py: the walk vs the exact (fp64) operator; the bound the table-driven path is held to
N_DIRS = {5: 34, 10: 152}

_WALKERS = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def _walker(r, variant):
    from irn_amd.misc import indexing
    if (r, variant) not in _WALKERS:
        wk = indexing.RandomWalk(r, _dev())
        wk.set_option("variant", variant)
        _WALKERS[(r, variant)] = wk
    return _WALKERS[(r, variant)]


def _edge_maps(h, w, seed):
    """The six kinds of edge map, in a fixed order."""
    rng = np.random.default_rng(seed)
    wall = np.zeros((h, w), np.float32)
    wall[:, w // 2] = 1.0
    wall[h // 3, w // 2] = 0.0                                           # the gap
    return [("uniform", rng.random((h, w), dtype=np.float32)),
            ("zeros", np.zeros((h, w), np.float32)),                     # every weight 1
            ("ones", np.ones((h, w), np.float32)),                       # every weight 0
            ("bernoulli", (rng.random((h, w)) < 0.3).astype(np.float32)),
            ("wall", wall),
            ("quantised", (np.floor(rng.random((h, w)) * 8) / 7).astype(np.float32))]   # 8 levels: many paths tie


def _planes(wk, r, edges, beta):
    """Weight planes of every image of one batched run."""
    dev = _dev()
    cams = [torch.ones((1,) + e.shape, device=dev) for e in edges]
    wk([torch.from_numpy(e).to(dev) for e in edges], cams, beta=beta, n_sweeps=1)
    wk.check()
    return [wk.export_weights(i, N_DIRS[r])[0].cpu().numpy() for i in range(len(edges))]


def _check(r, named_edges, beta, variant):
    got = _planes(_walker(r, variant), r, [e for _, e in named_edges], beta)
    for (name, e), g in zip(named_edges, got):
        _, want = O.stencil_weights(e, r, beta)
        assert g.shape == want.shape
        assert np.array_equal(g, want), (name, e.shape, r, beta, int((g != want).sum()))


# 20x20: smaller than a tile, narrower than 2R (streaming sweeps: the persistent kernel's planner refuses it);
# 33x37: odd height, width = 1 mod 4;  8x131: one tile row, three pixels past a multiple of 32 and of 128;  128x128: the launch shape
@pytest.mark.parametrize("r", [10, 5])
@pytest.mark.parametrize("h,w,variant", [(20, 20, 0), (33, 37, 2), (8, 131, 2), (128, 128, 2)])
def test_planes_equal_oracle(r, h, w, variant):
    _check(r, _edge_maps(h, w, 1000 + h), 10, variant)


@pytest.mark.parametrize("r", [10, 5])
@pytest.mark.parametrize("beta", [1, 7])
def test_other_bit_patterns_of_the_power_loop(r, beta):
    _check(r, _edge_maps(33, 37, 77), beta, 2)


@pytest.mark.parametrize("r", [10, 5])
def test_ragged_batch_every_image(r):
    """Three images in one call: plane_stride and front_pad differ per image, odd widths put rows on 4-byte boundaries."""
    kinds = ("uniform", "quantised", "bernoulli")
    named = []
    for i, (h, w) in enumerate([(94, 125), (125, 94), (30, 23)]):
        named.append([(n, e) for n, e in _edge_maps(h, w, 2000 + i) if n == kinds[i]][0])
    _check(r, named, 10, 2)


@pytest.mark.parametrize("r", [10, 5])
@pytest.mark.parametrize("variant", [0, 2])
def test_nan_workspace_changes_nothing(r, variant):
    """Pads and plane cells are all written on every call: a workspace full of NaN bytes gives the output of a zeroed one."""
    from irn_amd import synth
    dev = _dev()
    shapes = [(94, 125, 2), (125, 94, 1), (30, 23, 3)]
    edges = [torch.from_numpy(synth.edge_field(h, w, seed=60 + i)).to(dev) for i, (h, w, c) in enumerate(shapes)]
    cams = [torch.from_numpy(synth.cam_blobs(c, h, w, seed=60 + i)).to(dev) for i, (h, w, c) in enumerate(shapes)]
    wk = _walker(r, variant)
    outs = []
    for fill in (0, 0xFF):
        wk.configure(shapes)
        wk._ws.fill_(fill)
        o = wk(edges, cams, beta=10, n_sweeps=24)
        wk.check()
        outs.append([t.cpu().numpy() for t in o])
    for a, b in zip(*outs):
        assert np.isfinite(b).all()
        assert np.array_equal(a, b)


def test_non_integer_beta_keeps_the_table_driven_kernel():
    """beta = 2.5 at radius 10 goes to affinity_kernel<true> and zero_pad_kernel as before: the walk against the fp64 oracle,
    within the bound test_gpu_walk.py holds that path to."""
    from irn_amd import synth
    dev = _dev()
    h, w, c = 33, 37, 2
    edge = synth.edge_field(h, w, seed=5)
    cam = synth.cam_blobs(c, h, w, seed=5)
    wk = _walker(10, 2)
    wk.configure([(h, w, c)])
    wk._ws.fill_(0xFF)
    rw = wk([torch.from_numpy(edge).to(dev)], [torch.from_numpy(cam).to(dev)], beta=2.5, exp_times=4)[0]
    wk.check()
    st = O.propagate_to_edge_stencil(cam, edge, 10, 2.5, 4)
    assert np.abs(rw.cpu().numpy() - st).max() <= TOL_F64
