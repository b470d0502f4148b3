"""bench.py --dump-outputs on the host: the files it writes from a step's per-image outputs (no GPU involved)."""
import numpy as np

import bench


def _outputs(n, seed=0):
    rng = np.random.RandomState(seed)
    return {"labels": [rng.randint(0, 21, (64, 48)).astype(np.uint8) for _ in range(n)],
            "rw": [rng.rand(1 + i % 3, 1, 16, 12).astype(np.float32) for i in range(n)],
            "score": [rng.rand(i % 2).astype(np.float64) for i in range(n)]}


def test_whole_batch_stacked_or_concatenated(tmp_path):
    out = _outputs(5)
    written = bench.dump_outputs(str(tmp_path), out)
    assert sorted(written) == sorted(["index.npy", "labels.npy", "rw.npy", "rw_shapes.npy", "score.npy", "score_shapes.npy"])
    assert list(np.load(tmp_path / "index.npy")) == [0, 1, 2, 3, 4]
    labels = np.load(tmp_path / "labels.npy")
    assert labels.dtype == np.float32 and labels.shape == (5, 64, 48)
    assert np.array_equal(labels, np.stack(out["labels"]).astype(np.float32))
    rw, shapes = np.load(tmp_path / "rw.npy"), np.load(tmp_path / "rw_shapes.npy")
    assert rw.dtype == np.float32 and shapes.dtype == np.float64
    assert [tuple(int(v) for v in s) for s in shapes] == [a.shape for a in out["rw"]]
    assert np.array_equal(rw, np.concatenate([a.ravel() for a in out["rw"]]))
    assert np.load(tmp_path / "score.npy").dtype == np.float64


def test_over_budget_a_fixed_sample_of_the_same_images(tmp_path):
    out = _outputs(40)
    one = 64 * 48 * 4
    budget = 10 * one + 40 * 3 * 16 * 12 * 4                 # room for about ten images
    bench.dump_outputs(str(tmp_path / "a"), out, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), _outputs(40), budget=budget)
    idx = np.load(tmp_path / "a" / "index.npy")
    assert 0 < len(idx) < 40 and list(idx) == sorted(idx)
    total = sum(np.load(tmp_path / "a" / (k + ".npy")).nbytes for k in ("labels", "rw", "score"))
    assert total <= budget
    labels = np.load(tmp_path / "a" / "labels.npy")
    assert np.array_equal(labels, np.stack([out["labels"][int(i)] for i in idx]).astype(np.float32))
    for name in ("index", "labels", "rw", "rw_shapes", "score"):          # same inputs, same files
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy")))
