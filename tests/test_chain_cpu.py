"""The `chain` fixture holds its own conditions (tests/golden/make_golden.py gen_chain asserts them when it writes the file; here
they are checked on the stored arrays, without a GPU and without the reference): the stored label map IS the reference's epilogue
of the stored walk result, the stored detections paint the stored argmax map, few pixels are ties at the bar the GPU test uses, every
present class appears, and the reference's float32-vs-float64 distances that the bars are built from are real numbers."""
import numpy as np
import pytest

import _chain
from oracle import irn_oracle as O


@pytest.fixture(scope="module")
def fx():
    return _chain.load()


def test_fixture_names_two_images_and_one_carries_the_instance_branch(fx):
    assert tuple(float(s) for s in fx["scales"]) == (1.0, 0.5, 1.5, 2.0)
    a, b = _chain.size(fx, "a"), _chain.size(fx, "b")
    assert int(fx["a_label"].sum()) == 3 and int(fx["b_label"].sum()) == 1
    assert b[0] % 4 and b[1] % 16 and b[0] * b[1] <= 141 * 250
    assert "b_high_res" in fx and "a_high_res" not in fx
    assert "a_rw_up" not in fx and "b_rw_up" not in fx                    # rebuilt from rw by the tests
    assert any(_chain.has_instances(fx, n) for n in _chain.IMAGES)
    for n, (h, w) in (("a", a), ("b", b)):
        gh, gw = (h - 1) // 4 + 1, (w - 1) // 4 + 1
        k = int(fx[n + "_label"].sum())
        assert np.array_equal(fx[n + "_keys"], np.nonzero(fx[n + "_label"])[0])
        assert fx[n + "_cam"].shape == (k, gh, gw) and fx[n + "_edge"].shape == (1, gh, gw) and fx[n + "_dp"].shape == (2, gh, gw)
        assert fx[n + "_rw"].shape == (k, 1, gh, gw) and fx[n + "_label_map"].shape == (h, w) and fx[n + "_label_map"].dtype == np.uint8


@pytest.mark.parametrize("name", _chain.IMAGES)
def test_reference_distances_are_finite_and_positive(fx, name):
    keys = ["d_cam", "d_edge", "d_dp", "d_rw_up"] + (["d_rw_up_ins"] if _chain.has_instances(fx, name) else [])
    for k in keys:
        v = float(fx["%s_%s" % (name, k)])
        assert np.isfinite(v) and 0 < v < 1e-3, (name, k, v)


@pytest.mark.parametrize("name", _chain.IMAGES)
def test_label_map_is_the_epilogue_of_the_stored_walk(fx, name):
    bg = float(fx["bg"])
    up, label, _ = O.sem_seg_epilogue(fx[name + "_rw"], _chain.size(fx, name), fx[name + "_keys"], bg)
    assert np.array_equal(label, fx[name + "_label_map"])
    # every present class appears: the walk and the argmax are not trivial
    present = set((fx[name + "_keys"] + 1).tolist())
    assert present <= set(np.unique(label).tolist()), (present, np.unique(label))
    # tie share at the GPU test's bar
    ties = _chain.tie_count(up, bg, _chain.MARGIN * float(fx[name + "_d_rw_up"]))
    assert ties == int(fx[name + "_ties"])
    assert ties <= _chain.TIE_SHARE * label.size, (ties, label.size)


@pytest.mark.parametrize("name", _chain.IMAGES)
def test_detections_paint_the_stored_argmax(fx, name):
    if not _chain.has_instances(fx, name):
        assert name + "_centroids" not in fx and name + "_det_score" not in fx     # the instance-less form is all or nothing
        return
    bg = float(fx["bg"])
    h, w = _chain.size(fx, name)
    inst = _chain.instance_map(fx, name)
    keys = fx[name + "_keys"]
    rw_i = fx[name + "_rw_ins"]
    assert inst.sum(0).min() == 1 and inst.sum(0).max() == 1 and rw_i.shape[0] == len(keys) * inst.shape[0]
    up, _, idx = O.sem_seg_epilogue(rw_i, (h, w), np.zeros(rw_i.shape[0], np.int64), bg)
    assert np.array_equal(idx, fx[name + "_argmax"])
    det = _chain.detections(fx, name)
    chan_class = np.concatenate([[0], np.repeat(keys, inst.shape[0]) + 1])
    assert det["mask"].sum(0).max() <= 1
    assert np.array_equal(_chain.paint(det), chan_class[idx])
    # scores: the channel's maximum over the fragment, 0 for fragments under 1 % of the image (step/make_ins_seg_labels.py:96-99)
    for s, m, c in zip(det["score"], det["mask"], det["class"]):
        ch = np.unique(idx[m])
        assert len(ch) == 1 and chan_class[ch[0]] == c + 1
        assert s == (0 if m.sum() < 0.01 * h * w else up[ch[0] - 1][m].max())
    ties = _chain.tie_count(up, bg, _chain.MARGIN * float(fx[name + "_d_rw_up_ins"]))
    assert ties == int(fx[name + "_ties_ins"])
    assert ties <= _chain.TIE_SHARE * h * w, (ties, h * w)
