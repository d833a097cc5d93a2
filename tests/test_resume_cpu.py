"""CPU: --resume of the epoch loop the four trainers share (`trainloop.run_epochs`, `trainloop.load_resume`) with the fake trainer of
tests/test_trainloop_cpu.py: an interrupted-and-resumed run draws, schedules, validates, logs and checkpoints what the uninterrupted run
does; a kill at any point of the two-file write is either continued from the older pair or refused; a checkpoint without matching resume
state is refused; ranks > 0 keep their own generators' states."""
import argparse
import json
import os
import random
import re

import pytest
import torch

from computervision_codes_amd import drivers, trainloop
from computervision_codes_amd.trainloop import add_schedule_flags, lr_at_epoch, run_epochs

SCHEDULE = ["-w", "1", "2", "3", "-l", "0.1", "0.2", "0.05", "--power", "0.2", "--decay_rate", "0.9"]      # warm-up to epoch 3, decay after


class FakeTrainer:
    """its 'weights' are the last epoch and a running sum of every draw: a resumed run ends with the same bytes only if it drew the same"""

    def __init__(self):
        self.lr, self.epoch, self.acc = None, -1, 0.0

    def state_dict(self):
        return {"epoch": torch.tensor(self.epoch), "acc": torch.tensor(self.acc, dtype=torch.float64)}

    def load_state_dict(self, sd):
        self.epoch, self.acc = int(sd["epoch"]), float(sd["acc"])
        return self


def _flags(*argv, resume=True):
    p = argparse.ArgumentParser()
    add_schedule_flags(p)
    F = p.parse_args(list(argv) + SCHEDULE)
    F.resume = resume
    return F


class Run:
    """one process of a driver: fresh generators from the seed, the trainer started from `_latest` as the drivers do, `run_epochs`"""

    def __init__(self, tmp_path, F, scores=None, rank=0, world=1, die_in=None, every=True):
        d = tmp_path / "run"
        self.latest, self.best, self.log = str(d / "m_latest.pth"), str(d / "m.pth"), d / "m.log"
        self.draws, self.lrs, self.validated = {}, {}, []
        tr = FakeTrainer()
        py, tg = random.Random(5), torch.Generator().manual_seed(5 + rank)
        resume = trainloop.load_resume(self.latest, rank, world) if F.resume else None
        state = drivers._latest_state(self.latest, resume)
        if state is not None:
            tr.load_state_dict(state)

        def train_epoch(epoch):
            if epoch == die_in:
                raise KeyboardInterrupt
            a, b = py.random(), float(torch.rand((), generator=tg))
            py.shuffle(list(range(7)))
            self.draws[epoch], self.lrs[epoch] = (a, b), tr.lr
            tr.epoch, tr.acc = epoch, tr.acc + a + b * tr.lr
            return tr.acc, 2

        def validate(state):
            assert int(state["epoch"]) == tr.epoch
            self.validated.append(tr.epoch)
            score = scores[tr.epoch] if scores else 0.1 + 0.1 * (tr.epoch % 3)
            return score, f"ivt: [{score:.5f}]"

        self.result = run_epochs(F, tr, rank, train_epoch, validate, str(self.log), self.latest, self.best, latest_every_epoch=every,
                                 generators={"py": py, "tg": tg}, resume=resume, world=world)
        self.logged = self.log.read_text() if self.log.exists() else None

    def text(self):
        """the log file as this run left it"""
        return self.logged


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _epoch_lines(log, epochs):
    """the lines of `epochs` (the `Traning |` line up to the next one) that the last process wrote into the log -- everything behind the last
    `Resuming` line; a killed process may have logged some of these epochs before -- without the `secs` fields and the save line's wall-clock time"""
    out, keep = [], False
    lines = log.splitlines()
    start = max([i for i, ln in enumerate(lines) if ln.startswith("Resuming")], default=-1) + 1
    for ln in lines[start:]:
        m = re.match(r"Traning \| lr: .* \| epoch (\d+) \|", ln)
        if m:
            keep = int(m.group(1)) in epochs
        if keep and not ln.startswith("Resuming"):
            out.append(re.sub(r"^(>>> Saving checkpoint for epoch \d+) at .*$", r"\1", re.sub(r"[0-9.]+ secs", "secs", ln)))     # (the tree's path, the time)
    return out


def _assert_equals_straight(straight, parts, tmp_s, tmp_r, epochs=range(3, 6)):
    """`parts`: the runs of the interrupted tree in order; the last one against the straight run over `epochs`, the files of both trees"""
    last = parts[-1]
    for e in epochs:
        assert last.draws[e] == straight.draws[e] and last.lrs[e] == straight.lrs[e] == lr_at_epoch(e, 0.05, 0.2, 3, 0.9), e
    assert sorted(last.draws) == list(epochs)
    assert last.validated == [e for e in straight.validated if e in epochs]
    assert last.result == straight.result
    for name in ("m_latest.pth", "m.pth"):
        assert _bytes(tmp_s / "run" / name) == _bytes(tmp_r / "run" / name), name
    assert int(torch.load(tmp_r / "run" / "m.pth")["epoch"]) == int(torch.load(tmp_s / "run" / "m.pth")["epoch"])
    lines = _epoch_lines(last.text(), epochs)
    assert lines == _epoch_lines(straight.text(), epochs) and sum(ln.startswith("Traning | lr:") for ln in lines) == len(epochs)
    assert sorted(os.listdir(tmp_r / "run")) == sorted(os.listdir(tmp_s / "run")) == ["m.log", "m.pth", "m_latest.pth", "m_latest.pth.resume"]


@pytest.mark.parametrize("every", [True, False], ids=["latest_every_epoch", "latest_at_validation"])
def test_three_epochs_then_resume_equals_six_straight(tmp_path, every):
    s, r = tmp_path / "s", tmp_path / "r"
    extra = [] if every else ["--val_interval", "2"]
    straight = Run(s, _flags("--epochs", "6", *extra), every=every)
    first = Run(r, _flags("--epochs", "3", *extra), every=every)
    second = Run(r, _flags("--epochs", "6", *extra), every=every)
    assert "Resuming" not in first.text() and sorted(first.draws) == [0, 1, 2]
    assert second.text().count("Resuming at epoch 3 (best so far 0.30000)") == 1
    _assert_equals_straight(straight, [first, second], s, r)
    assert straight.validated == ([0, 1, 2, 3, 4, 5] if every else [0, 2, 4])
    assert int(torch.load(r / "run" / "m.pth")["epoch"]) == 2            # scores 0.1 0.2 0.3 0.1 0.2 0.3: the first 0.3 stays the best


def test_a_run_killed_in_epoch_four_and_resumed_equals_the_straight_run(tmp_path):
    """`_latest` only at validation epochs (0, 2, 4): the kill in epoch 4 leaves the pair of epoch 2, so epoch 3 is run again"""
    s, r = tmp_path / "s", tmp_path / "r"
    F = lambda: _flags("--epochs", "6", "--val_interval", "2")
    straight = Run(s, F(), every=False)
    with pytest.raises(KeyboardInterrupt):
        Run(r, F(), every=False, die_in=4)
    second = Run(r, F(), every=False)
    assert second.text().count("Resuming at epoch 3 ") == 1
    _assert_equals_straight(straight, [second], s, r)


RISING = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]                       # every epoch is the best so far: best `.pth`, sidecar, `_latest` per epoch


@pytest.mark.parametrize("scores,fail_at", [(None, n) for n in range(1, 7)] + [(RISING, n) for n in range(1, 7)])
def test_a_kill_between_the_file_writes_is_continued_or_refused(tmp_path, monkeypatch, scores, fail_at):
    """the `fail_at`-th os.replace of the run that continues after epoch 2 dies (2: the second); the next --resume ends equal to the straight
    run from the older consistent pair, or refuses with the ValueError of a mismatch -- nothing else"""
    s, r = tmp_path / "s", tmp_path / "r"
    straight = Run(s, _flags("--epochs", "6"), scores=scores)
    Run(r, _flags("--epochs", "3"), scores=scores)
    real, calls = os.replace, []

    def replace(a, b):
        calls.append(os.path.basename(b))
        if len(calls) == fail_at:
            raise KeyboardInterrupt
        return real(a, b)
    monkeypatch.setattr(os, "replace", replace)
    with pytest.raises(KeyboardInterrupt):
        Run(r, _flags("--epochs", "6"), scores=scores)
    monkeypatch.setattr(os, "replace", real)
    per_epoch = (["m.pth"] if scores else []) + ["m_latest.pth.resume", "m_latest.pth"]      # the sidecar is replaced first, then `_latest`
    assert calls == (per_epoch * 3)[:fail_at]
    assert not [f for f in os.listdir(r / "run") if f.endswith(".tmp")]
    try:
        again = Run(r, _flags("--epochs", "6"), scores=scores)
    except ValueError as e:
        assert "--resume" in str(e) and "m_latest.pth" in str(e)
        return
    first = min(again.draws)
    assert first in (3, 4, 5) and f"Resuming at epoch {first} " in again.text()
    _assert_equals_straight(straight, [again], s, r, epochs=range(first, 6))


def test_best_score_is_kept_across_the_restart(tmp_path):
    Run(tmp_path, _flags("--epochs", "1"), scores=[0.9, 0.1, 0.2])
    before = _bytes(tmp_path / "run" / "m.pth")
    second = Run(tmp_path, _flags("--epochs", "3"), scores=[0.9, 0.1, 0.2])
    assert second.validated == [1, 2] and "Resuming at epoch 1 (best so far 0.90000)" in second.text()
    assert second.text().count(">>> Saving checkpoint") == 1              # epoch 0's; none for the lower scores
    assert _bytes(tmp_path / "run" / "m.pth") == before and int(torch.load(tmp_path / "run" / "m.pth")["epoch"]) == 0
    assert int(torch.load(tmp_path / "run" / "m_latest.pth")["epoch"]) == 2


def test_latest_without_resume_state_is_refused_before_anything_is_touched(tmp_path):
    Run(tmp_path, _flags("--epochs", "2", resume=False))
    assert sorted(os.listdir(tmp_path / "run")) == ["m.log", "m.pth", "m_latest.pth"]          # flag off: no sidecar
    before = {f: _bytes(tmp_path / "run" / f) for f in os.listdir(tmp_path / "run")}
    with pytest.raises(ValueError, match=r"--resume: .*m_latest\.pth has no resume state .*m_latest\.pth\.resume is missing.*Drop --resume"):
        Run(tmp_path, _flags("--epochs", "4"))
    assert {f: _bytes(tmp_path / "run" / f) for f in os.listdir(tmp_path / "run")} == before
    with pytest.raises(ValueError, match="has no resume state"):          # `run_epochs` on its own refuses as well
        run_epochs(_flags("--epochs", "4"), FakeTrainer(), 0, None, None, str(tmp_path / "run" / "m.log"), str(tmp_path / "run" / "m_latest.pth"),
                   str(tmp_path / "run" / "m.pth"))


def test_another_world_size_is_refused(tmp_path):
    Run(tmp_path, _flags("--epochs", "2"))
    with pytest.raises(ValueError, match=r"--resume: .*m_latest\.pth\.resume was written by a run of 1 rank\(s\) and this one has 2"):
        Run(tmp_path, _flags("--epochs", "4"), world=2)


def test_a_replaced_latest_is_refused(tmp_path):
    Run(tmp_path, _flags("--epochs", "2"))
    trainloop.save_atomic({"epoch": torch.tensor(1), "acc": torch.tensor(7.0, dtype=torch.float64)}, str(tmp_path / "run" / "m_latest.pth"))
    with pytest.raises(ValueError, match=r"--resume: .*m_latest\.pth \(sha256:.*is not the checkpoint .*m_latest\.pth\.resume was written for"):
        Run(tmp_path, _flags("--epochs", "4"))


def test_the_loaded_weights_are_the_digested_bytes(tmp_path):
    """the state dict a resumed trainer loads comes from the bytes whose digest was checked, not from a second read of the file"""
    Run(tmp_path, _flags("--epochs", "2"))
    latest = str(tmp_path / "run" / "m_latest.pth")
    res = trainloop.load_resume(latest)
    want = torch.load(latest)
    os.remove(latest)
    got = drivers._latest_state(latest, res)
    assert res.epoch == 1 and got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in want)
    side = json.load(open(latest + trainloop.RESUME_SUFFIX))
    assert side["world"] == 1 and [r["epoch"] for r in side["records"]] == [1, 0] and set(side["records"][0]) == {"epoch", "top", "digest", "generators"}
    assert trainloop.resume_file(latest) == latest + ".resume" and trainloop.resume_file(latest, 3) == latest + ".resume.rank3"


def test_a_finished_run_trains_nothing(tmp_path, capsys):
    n = len(Run(tmp_path, _flags("--epochs", "3")).text().splitlines())
    before = {f: _bytes(tmp_path / "run" / f) for f in os.listdir(tmp_path / "run") if not f.endswith(".log")}
    capsys.readouterr()
    again = Run(tmp_path, _flags("--epochs", "3"), die_in=2)
    assert again.result == {} and again.draws == {} and again.validated == []
    lines = again.text().splitlines()
    assert len(lines) == n + 1 and lines[-1] == "Resuming: epoch 2 was the last of --epochs 3 (best so far 0.30000); nothing left to train"
    assert capsys.readouterr().out.splitlines() == lines[-1:]             # one line, printed and logged
    assert {f: _bytes(tmp_path / "run" / f) for f in os.listdir(tmp_path / "run") if not f.endswith(".log")} == before


def test_a_rank_above_zero_keeps_and_restores_its_own_generators(tmp_path, capsys):
    """rank 1 of 2 beside rank 0 in one directory: it writes `<latest>.resume.rank1` and nothing else, restores ITS torch generator (seeded by
    rank) and continues the straight run's draws"""
    s, r = tmp_path / "s", tmp_path / "r"
    straight = Run(s, _flags("--epochs", "6"), rank=1, world=2)
    assert sorted(os.listdir(s / "run")) == ["m_latest.pth.resume.rank1"] and capsys.readouterr().out == ""
    first = Run(r, _flags("--epochs", "3"), rank=1, world=2)             # (one after the other here: rank 1 starts before rank 0 has written)
    Run(r, _flags("--epochs", "3"), rank=0, world=2)
    assert sorted(os.listdir(r / "run")) == ["m.log", "m.pth", "m_latest.pth", "m_latest.pth.resume", "m_latest.pth.resume.rank1"]
    rank0 = {f: _bytes(r / "run" / f) for f in os.listdir(r / "run") if not f.endswith("rank1")}
    second = Run(r, _flags("--epochs", "6"), rank=1, world=2)
    assert sorted(second.draws) == [3, 4, 5] and all(second.draws[e] == straight.draws[e] for e in (3, 4, 5))
    assert all(second.lrs[e] == straight.lrs[e] for e in (3, 4, 5)) and first.draws[2] == straight.draws[2]
    assert {f: _bytes(r / "run" / f) for f in os.listdir(r / "run") if not f.endswith("rank1")} == rank0          # rank 1 touched none of them
    rank0_draws = Run(tmp_path / "z", _flags("--epochs", "3"), rank=0, world=2).draws
    assert rank0_draws[2][0] == first.draws[2][0] and rank0_draws[2][1] != first.draws[2][1]                       # shared python stream, own torch stream
    os.remove(r / "run" / "m_latest.pth.resume.rank1")
    with pytest.raises(ValueError, match=r"--resume: rank 1 has no resume state .*m_latest\.pth\.resume\.rank1 is missing"):
        Run(r, _flags("--epochs", "6"), rank=1, world=2)


def test_flag_off_is_unchanged_and_the_flag_is_declared_on_every_trainer(tmp_path):
    for stage in ("spatial_cnn", "spatial_transformer", "mstct", "tenco"):
        p = drivers._parser(stage, True)
        assert p.parse_known_args([])[0].resume is False
        F, rest = p.parse_known_args(["--resume"])
        assert F.resume is True and rest == []
    off = Run(tmp_path, _flags("--epochs", "3", resume=False))
    assert sorted(os.listdir(tmp_path / "run")) == ["m.log", "m.pth", "m_latest.pth"] and "Resuming" not in off.text()
    again = Run(tmp_path, _flags("--epochs", "3", resume=False))           # as always: from `_latest`'s weights at epoch 0
    assert sorted(again.draws) == [0, 1, 2] and again.draws == off.draws
