"""CPU: the epoch and checkpoint loop of the four training drivers (`computervision_codes_amd/trainloop.py`) with a fake trainer and a
fake validation: dealing of batches to ranks, validation cadence, best / latest checkpoints, atomic writes, rank-0-only output, lr."""
import argparse
import os

import pytest
import torch

from computervision_codes_amd import trainloop
from computervision_codes_amd.trainloop import add_schedule_flags, deal, lr_at_epoch, run_epochs


class FakeTrainer:
    def __init__(self):
        self.lr, self.epoch = None, -1

    def state_dict(self):
        return {"epoch": torch.tensor(self.epoch)}


def _flags(*argv):
    p = argparse.ArgumentParser()
    add_schedule_flags(p)
    return p.parse_args(list(argv))


def _run(tmp_path, F, scores=None, rank=0, latest_every_epoch=False):
    """run_epochs with one fake step per epoch; -> (validated epochs, lr per epoch, the log text or None, the result)"""
    tr, validated, lrs = FakeTrainer(), [], []

    def train_epoch(epoch):
        tr.epoch = epoch
        lrs.append(tr.lr)
        return 2.0 * epoch, 2

    def validate(state):
        assert int(state["epoch"]) == tr.epoch
        validated.append(tr.epoch)
        score = scores[tr.epoch] if scores else 0.5
        return score, f"ivt: [{score:.5f}]"

    log = tmp_path / "run" / "m.log"
    res = run_epochs(F, tr, rank, train_epoch, validate, str(log), str(tmp_path / "run" / "m_latest.pth"), str(tmp_path / "run" / "m.pth"),
                     latest_every_epoch=latest_every_epoch)
    return validated, lrs, log.read_text() if log.exists() else None, res


def test_deal_is_the_round_robin_of_the_drivers():
    for nb in range(1, 10):
        for world in range(1, 5):
            for rank in range(world):
                old = [(s * world + rank) % nb for s in range((nb + world - 1) // world)]
                assert deal(list(range(nb)), 1, world, rank) == [[i] for i in old], (nb, world, rank)
                items = list(range(3 * nb - 1))                      # batches of 3, the last one short (drop_last False)
                assert deal(items, 3, world, rank) == [items[i * 3:(i + 1) * 3] for i in old], (nb, world, rank)


@pytest.mark.parametrize("epochs,val_interval,want", [(5, 1, [0, 1, 2, 3, 4]), (5, 2, [0, 2, 4]), (5, -1, [0, 4]), (5, 0, [0, 1, 2, 3, 4]),
                                                      (1, 1, [0]), (1, 2, [0]), (1, -1, [0]), (1, 0, [0])])
def test_validation_cadence(tmp_path, epochs, val_interval, want):
    validated, _, log, res = _run(tmp_path, _flags("--epochs", str(epochs), "--val_interval", str(val_interval)))
    assert validated == want
    assert log.count("Traning | lr:") == epochs and log.count("mAP => ivt: [0.50000]") == len(want)
    assert res["loss"] == epochs - 1 and ("val_mAP" in res) == (epochs - 1 in want)


def test_best_checkpoint_follows_the_score(tmp_path):
    _, _, log, res = _run(tmp_path, _flags("--epochs", "3"), scores=[0.2, 0.1, 0.3])
    assert log.count(">>> Saving checkpoint") == 2
    assert ">>> Saving checkpoint for epoch 1 at " in log and ">>> Saving checkpoint for epoch 3 at " in log
    assert int(torch.load(tmp_path / "run" / "m.pth")["epoch"]) == 2
    assert res["val_mAP"] == 0.3
    assert not [f for f in os.listdir(tmp_path / "run") if f.endswith(".tmp")]


@pytest.mark.parametrize("every", [False, True])
def test_latest_cadence(tmp_path, monkeypatch, every):
    writes = []
    save = trainloop.save_atomic
    monkeypatch.setattr(trainloop, "save_atomic", lambda state, path: (writes.append((os.path.basename(path), int(state["epoch"]))), save(state, path)))
    _run(tmp_path, _flags("--epochs", "4", "--val_interval", "2"), scores=[0.1, 0.2, 0.3, 0.4], latest_every_epoch=every)
    assert [e for f, e in writes if f == "m_latest.pth"] == ([0, 1, 2, 3] if every else [0, 2])
    assert [e for f, e in writes if f == "m.pth"] == [0, 2]
    assert int(torch.load(tmp_path / "run" / "m_latest.pth")["epoch"]) == (3 if every else 2)
    assert sorted(os.listdir(tmp_path / "run")) == ["m.log", "m.pth", "m_latest.pth"]


def test_interrupted_write_keeps_the_previous_checkpoint(tmp_path, monkeypatch):
    _run(tmp_path, _flags("--epochs", "1"))
    real = torch.save

    def torn(obj, f):                                        # the process dies halfway through the write
        with open(f, "wb") as fh:
            fh.write(b"PK\x03\x04 truncated")
        raise KeyboardInterrupt

    monkeypatch.setattr(torch, "save", torn)
    with pytest.raises(KeyboardInterrupt):
        _run(tmp_path, _flags("--epochs", "2"))
    monkeypatch.setattr(torch, "save", real)
    for name in ("m_latest.pth", "m.pth"):
        assert int(torch.load(tmp_path / "run" / name)["epoch"]) == 0
    assert sorted(os.listdir(tmp_path / "run")) == ["m.log", "m.pth", "m_latest.pth"]


def test_other_ranks_write_and_log_nothing(tmp_path, capsys):
    validated, lrs, log, res = _run(tmp_path, _flags("--epochs", "3"), rank=1)
    assert validated == [] and log is None and not (tmp_path / "run").exists() and capsys.readouterr().out == ""
    assert len(lrs) == 3 and res == {"loss": 2.0, "lr": lrs[-1]}


def test_lr_follows_the_schedule(tmp_path):
    F = _flags("--epochs", "8", "-w", "1", "2", "3", "-l", "0.1", "0.2", "0.05", "--power", "0.2", "--decay_rate", "0.9")
    _, lrs, log, _ = _run(tmp_path, F)
    assert lrs == [lr_at_epoch(e, 0.05, 0.2, 3, 0.9) for e in range(8)]
    assert f"Traning | lr: {lrs[5]:.6f} | epoch 5 | loss 5.0000 | " in log
