"""The training steps' shared parts (irn_amd/step/_train.py) apart from any network: the loop's report cadence and hooks on a
two-parameter model and ten in-memory items on the CPU, the loader's contract, the length check, the initial state's
re-keying and the saving.  None of it needs a GPU."""
import re

import pytest
import torch
from torch import nn
from torch.utils.data import Dataset

from irn_amd.step import _train

CPU = torch.device("cpu")


class Items(Dataset):
    """n items {x: [1], idx}, raw (not pinned) unless told otherwise, and the epochs it was told about."""

    def __init__(self, n=10, raw=True):
        self.n, self.raw, self.epochs = n, raw, []

    def set_epoch(self, ep):
        self.epochs.append(ep)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {"x": torch.tensor([float(i + 1)]), "idx": i}


def _order(dataset, seed, batch_size=2):
    return [int(i) for pack in _train.loader(dataset, batch_size, 0, True, seed) for i in pack["idx"]]


@pytest.mark.parametrize("k", (None, 3))
def test_reports_fire_every_print_every_steps_over_the_losses_since_the_last_one(capsys, k):
    torch.manual_seed(0)
    model = nn.Linear(1, 1)
    dataset = Items(10)
    optimizer = _train.two_rate_optimizer([model.weight], [model.bias], 0.01, 0.0, _train.max_steps("t", "train_list", dataset, 2, 2))
    assert optimizer.max_step == 10 and [g["lr"] for g in optimizer.param_groups] == [0.01, 0.1]
    losses, reports, epochs, seeds = [], [], [], []

    def step(pack):
        loss = (model(pack["x"]) ** 2).mean()
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        losses.append(loss.detach() if k is None else loss.detach() * torch.arange(1.0, k + 1))
        return losses[-1]

    def make_loader(seed):
        seeds.append(seed)
        return _train.loader(dataset, 2, 0, True, seed)

    first = _train.fit(model, optimizer, dataset, make_loader, CPU, 2, 2, 40, 2, step, "loss:" + " ".join(["%.6f"] * (k or 1)),
                       on_report=lambda: reports.append(len(losses)), after_epoch=epochs.append)
    assert len(losses) == 10 and optimizer.global_step == 10
    assert torch.equal(first, losses[0]) and first.device == CPU
    assert reports == [1, 3, 5, 7, 9]                            # once per report, behind global steps 1, 3, 5, 7, 9
    assert epochs == [0, 1] and dataset.epochs == [0, 1] and seeds == [40, 41]
    assert model.training
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step:")]
    assert [ln.split(" loss:")[0] for ln in lines] == ["step:%5d/%5d" % (s, 10) for s in (0, 2, 4, 6, 8)]
    since = [losses[0:1], losses[1:3], losses[3:5], losses[5:7], losses[7:9]]
    for ln, chunk in zip(lines, since):
        assert re.fullmatch(r"step:.* loss:.* imps:\d+\.\d lr: 0\.\d{4} etc:.+", ln), ln
        want = torch.stack(chunk).mean(0).reshape(-1)
        assert ln.split(" imps:")[0].split("loss:")[1].split() == ["%.6f" % float(v) for v in want]


def test_loader_clamps_workers_pins_host_items_drops_the_tail_and_follows_the_seed():
    for asked, got in ((-3, 0), (0, 0), (5, 5), (99, 8)):
        assert _train.loader(Items(), 2, asked, True, 0).num_workers == got
    assert _train.MAX_LOADER_WORKERS == 8
    assert _train.loader(Items(raw=True), 2, 0, True, 0).pin_memory is False
    assert _train.loader(Items(raw=False), 2, 0, True, 0).pin_memory is True
    assert _train.loader([0, 1, 2, 3], 2, 0, False, 0).pin_memory is True          # (a dataset without the attribute)
    a, b, c = _order(Items(), 7), _order(Items(), 7), _order(Items(), 8)
    assert a == b and sorted(a) == list(range(10)) and a != c
    assert _order(Items(), 7) != list(range(10))
    assert [int(i) for p in _train.loader(Items(), 2, 0, False, 7) for i in p["idx"]] == list(range(10))
    eleven = _order(Items(11), 7)
    assert len(eleven) == 10 and len(set(eleven)) == 10                               # drop_last: the eleventh is left out
    assert len(_order(Items(11), 7, batch_size=4)) == 8
    marks = []
    _train.loader(Items(), 2, 0, False, 0, collate_fn=lambda items: marks.append(len(items))).__iter__().__next__()
    assert marks == [2]


def test_max_steps_counts_whole_batches_and_names_the_step_the_list_and_the_batch():
    assert _train.max_steps("train_cam", "train_list", Items(10), 2, 3) == 15
    assert _train.max_steps("train_cam", "train_list", Items(11), 4, 3) == 6
    assert _train.max_steps("train_cam", "val_list", Items(4), 4, 1) == 1
    with pytest.raises(RuntimeError) as err:
        _train.max_steps("train_irn", "infer_list", Items(3), 4, 5)
    assert str(err.value) == "train_irn: infer_list holds fewer images than one batch of 4"


def test_init_state_rekeys_a_bare_trunk_and_drops_what_it_is_told_to(tmp_path):
    def saved(state):
        path = str(tmp_path / ("s%d.pth" % len(list(tmp_path.iterdir()))))
        torch.save(state, path)
        return path

    bare = {"conv1.weight": torch.ones(2), "layer1.0.conv1.weight": torch.zeros(3), "fc.weight": torch.ones(4)}
    got = _train.init_state(saved(bare))
    assert list(got) == ["resnet50.conv1.weight", "resnet50.layer1.0.conv1.weight"]
    assert torch.equal(got["resnet50.conv1.weight"], bare["conv1.weight"]) and got["resnet50.conv1.weight"].device == CPU
    full = {"resnet50.conv1.weight": torch.ones(2), "resnet50.fc.weight": torch.ones(1), "classifier.weight": torch.ones(5)}
    got = _train.init_state(saved(full))
    assert list(got) == list(full) and all(torch.equal(got[k], full[k]) for k in full)
    assert list(_train.init_state(saved(full), drop=("classifier.",))) == ["resnet50.conv1.weight", "resnet50.fc.weight"]
    assert list(_train.init_state(saved(bare), drop=("classifier.",))) == ["resnet50.conv1.weight", "resnet50.layer1.0.conv1.weight"]


def test_save_state_makes_the_directory_and_writes_a_plain_state_dict(tmp_path, monkeypatch):
    torch.manual_seed(1)
    model = nn.Linear(1, 1)
    path = str(tmp_path / "a" / "b" / "model.pth")
    _train.save_state(model, path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert list(state) == ["weight", "bias"] and all(torch.equal(state[k], v) for k, v in model.state_dict().items())
    _train.save_state(model, str(tmp_path / "a" / "again.pth"))                        # an existing directory is fine
    monkeypatch.chdir(tmp_path)
    _train.save_state(model, "here.pth")                                               # no directory part
    assert (tmp_path / "here.pth").exists()
