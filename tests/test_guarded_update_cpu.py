"""CPU: the host side of --clip_grad_norm / --skip_nonfinite -- the flags on the four trainers' parsers, the host restatement of the guarded update
(`ops.guarded_sgd_host`) against torch's clip_grad_norm_ + SGD, the plan query, the refusals of the C entry points (no device is touched) and the
epoch loop's note, loss mean and all-skipped stop with a fake trainer."""
import argparse
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from computervision_codes_amd import _lib, drivers, ops, trainloop
from computervision_codes_amd.trainloop import LossMean, add_schedule_flags, run_epochs

STAGES = ["spatial_cnn", "spatial_transformer", "mstct", "tenco"]


# ------------------------------------------------------------------------------------------------ the flags
@pytest.mark.parametrize("stage", STAGES)
def test_flags_are_declared_and_off_by_default(stage, capsys):
    p = drivers._parser(stage, True)
    F, rest = p.parse_known_args([])
    assert F.clip_grad_norm == 0.0 and F.skip_nonfinite is False and rest == []
    assert drivers._guard(F) == {"clip_grad_norm": 0.0, "skip_nonfinite": False} and capsys.readouterr().out == ""     # off: not a word
    F, rest = p.parse_known_args(["--clip_grad_norm", "2.5", "--skip_nonfinite"])
    assert F.clip_grad_norm == 2.5 and F.skip_nonfinite is True and rest == []     # declared: not among the flags parse_known_args drops in silence
    assert drivers._guard(F) == {"clip_grad_norm": 2.5, "skip_nonfinite": True}
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "--clip_grad_norm 2.5" in out and "--skip_nonfinite" in out                        # said once at start
    with pytest.raises(ValueError, match="--clip_grad_norm"):
        drivers._guard(p.parse_known_args(["--clip_grad_norm", "-1"])[0])
    with pytest.raises(ValueError, match="--clip_grad_norm"):
        drivers._guard(p.parse_known_args(["--clip_grad_norm", "nan"])[0])


def test_a_negative_norm_is_refused_before_any_model_is_built():
    """no GPU and no dataset here: anything past the refusal would fail differently"""
    bad = ["-t", "--clip_grad_norm", "-0.5", "--data_dir", "/nonexistent"]
    with pytest.raises(ValueError, match="--clip_grad_norm -0.5"):
        drivers.spatial_cnn_train(bad)
    with pytest.raises(ValueError, match="--clip_grad_norm -0.5"):
        drivers.spatial_transformer_train(bad + ["--loss_type", "i"])
    with pytest.raises(ValueError, match="--clip_grad_norm -0.5"):
        drivers._mstct_train(drivers._parser("mstct", True).parse_known_args(bad + ["--loss_type", "i"])[0])
    with pytest.raises(ValueError, match="--clip_grad_norm -0.5"):
        drivers._tenco_train(drivers._parser("tenco", True).parse_known_args(bad + ["--fpn"])[0])


# ------------------------------------------------------------------------------------------------ the host restatement
def _torch_step(p, g, lr, wd, max_norm):
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_([q], max_norm)
    torch.optim.SGD([q], lr=lr, weight_decay=wd).step()
    return q.detach()


@pytest.mark.parametrize("n,seed,gmag", [(1, 0, 1.0), (5, 1, 3.0), (1000, 2, 0.01), (4099, 3, 50.0)])
def test_host_restatement_against_torch_clip_and_sgd(n, seed, gmag):
    gen = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * gmag
    lr, wd = 0.05, 1e-3
    norm = float(g.double().norm())
    for max_norm in (0.0, 0.3 * norm, 0.9 * norm):
        got, info = ops.guarded_sgd_host(p, g, lr, wd, 1.0, max_norm, False)
        want = _torch_step(p, g, lr, wd, max_norm)
        assert got.dtype == torch.float32 and float((got - want).abs().max()) <= 1e-6 * float(want.abs().max()), (n, max_norm)      # (torch: fp32 norm)
        assert info["skip"] == 0 and info["nonfinite"] == 0 and abs(info["norm"] - norm) <= 1e-12 * norm
        assert (info["coef"] < 1.0) == (max_norm > 0)
    # a clip that does not bite: coef is exactly 1 and the step is the unclipped one, bit for bit
    plain, _ = ops.guarded_sgd_host(p, g, lr, wd, 1.0, 0.0, False)
    loose, info = ops.guarded_sgd_host(p, g, lr, wd, 1.0, 10.0 * norm, False)
    assert info["coef"] == 1.0 and torch.equal(loose, plain)
    # grad_scale (the data-parallel mean) scales the norm the clip sees
    _, half = ops.guarded_sgd_host(p, g, lr, wd, 0.5, 0.0, False)
    assert abs(half["norm"] - 0.5 * norm) <= 1e-12 * norm


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("where", [0, 7, 99])
def test_host_restatement_skips_a_nonfinite_gradient(bad, where):
    gen = torch.Generator().manual_seed(5)
    p, g = torch.randn(100, generator=gen), torch.randn(100, generator=gen)
    g[where] = bad
    got, info = ops.guarded_sgd_host(p, g, 0.1, 1e-4, 1.0, 1.0, True)
    assert info["skip"] == 1 and info["nonfinite"] == 1 and info["coef"] == 1.0
    assert torch.equal(got.view(torch.int32), p.view(torch.int32))                                   # bit-identical to before
    # without the flag: applied as today (coef 1: the clip is not evaluated on a non-finite norm)
    got, info = ops.guarded_sgd_host(p, g, 0.1, 1e-4, 1.0, 1.0, False)
    want = _torch_step(p, g, 0.1, 1e-4, 0.0)
    assert info["skip"] == 0 and info["nonfinite"] == 1 and info["coef"] == 1.0
    ok = torch.arange(100) != where
    assert not math.isfinite(float(got[where])) and torch.allclose(got[ok], want[ok], rtol=1e-6, atol=1e-7)


def test_host_restatement_takes_the_norm_in_float64():
    g = torch.full((64,), 1e30)                                                                      # the fp32 norm overflows, float64's does not
    got, info = ops.guarded_sgd_host(torch.zeros(64), g, 1.0, 0.0, 1.0, 1.0, True)
    assert info["skip"] == 0 and math.isfinite(info["norm"]) and abs(info["norm"] - 8e30) <= 1e-6 * 8e30
    assert bool(torch.isfinite(got).all()) and abs(float(got.double().norm()) - 1.0) < 1e-5          # clipped to norm 1, not zeroed


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_is_a_function_of_n_alone_and_monotone():
    one = ops.grad_norm_plan(1)
    assert one.nparts == 1 and one.part_elems > 0 and one.part_elems % 4 == 0 and one.bytes == 16
    pe, last = one.part_elems, one
    for n in [1, 2, 3, 4, 5, 1023, pe - 1, pe, pe + 1, 3 * pe, 3 * pe + 4, (1 << 20) + 4, 25_600_000, 200_000_000, (1 << 31) + 5]:
        q = ops.grad_norm_plan(n)
        assert q == ops.grad_norm_plan(n)                                                            # the same answer twice
        assert q.part_elems == pe and q.nparts == -(-n // pe) and q.bytes == 16 * q.nparts
        assert q.nparts >= last.nparts and q.bytes >= last.bytes
        last = q
    for n in (0, -3):
        with pytest.raises(_lib.Mt4Error):
            ops.grad_norm_plan(n)


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_bad_arguments_without_a_device():
    """the C entry points return before any launch (no GPU here: a launch would fail differently)"""
    lib, buf = _lib.lib, ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    EINVAL = -1
    n = 3 * ops.grad_norm_plan(1).part_elems + 4
    need = ops.grad_norm_plan(n).bytes
    assert lib.mt4_grad_norm_plan(0, None, None, None) == EINVAL and lib.mt4_grad_norm_plan(5, None, None, None) == 0
    assert lib.mt4_grad_norm_parts_f32(None, n, p, need, None) == EINVAL and lib.mt4_grad_norm_parts_f32(p, n, None, need, None) == EINVAL
    assert lib.mt4_grad_norm_parts_f32(p, 0, p, need, None) == EINVAL
    assert lib.mt4_grad_norm_parts_f32(p, n, p, need - 4, None) == EINVAL                            # four bytes short
    assert lib.mt4_grad_norm_parts_f32(p + 4, n, p, need, None) not in (0, EINVAL)                   # misaligned: its own code
    assert lib.mt4_grad_norm_parts_f32(p, n, p + 8, need, None) == lib.mt4_grad_norm_parts_f32(p + 4, n, p, need, None)
    fin = lib.mt4_grad_guard_finalize
    assert fin(None, 4, 1.0, 1.0, 1, p, p, None) == EINVAL and fin(p, 4, 1.0, 1.0, 1, None, p, None) == EINVAL
    assert fin(p, 4, 1.0, 1.0, 1, p, None, None) == EINVAL and fin(p, 0, 1.0, 1.0, 1, p, p, None) == EINVAL
    assert fin(p, 4, 1.0, -1.0, 1, p, p, None) == EINVAL and fin(p, 4, 1.0, float("nan"), 1, p, p, None) == EINVAL
    assert fin(p + 8, 4, 1.0, 1.0, 1, p, p, None) not in (0, EINVAL) and fin(p, 4, 1.0, 1.0, 1, p + 4, p, None) not in (0, EINVAL)
    sgd = lib.mt4_sgd_step_guarded_f32
    assert sgd(None, p, 8, 0.1, 0.0, 1.0, p, None) == EINVAL and sgd(p, None, 8, 0.1, 0.0, 1.0, p, None) == EINVAL
    assert sgd(p, p, 8, 0.1, 0.0, 1.0, None, None) == EINVAL and sgd(p, p, 0, 0.1, 0.0, 1.0, p, None) == EINVAL
    assert sgd(p + 4, p, 8, 0.1, 0.0, 1.0, p, None) not in (0, EINVAL)
    rst = lib.mt4_restore_if_skipped_f32
    assert rst(None, p, 8, p, None) == EINVAL and rst(p, None, 8, p, None) == EINVAL and rst(p, p, 8, None, None) == EINVAL
    assert rst(p, p, 0, p, None) == EINVAL and rst(p, p + 4, 8, p, None) not in (0, EINVAL)


def test_wrappers_refuse_before_any_launch():
    plan = ops.grad_norm_plan(100000)
    ws, rec = torch.empty(plan.nparts * 2 - 1, dtype=torch.float64), torch.zeros(5, dtype=torch.float64)
    with pytest.raises(_lib.Mt4Error):
        ops.grad_guard(torch.zeros(100000), 1.0, 0.0, True, ws, rec, rec)                            # not on the device
    with pytest.raises(_lib.Mt4Error):
        ops.sgd_step_guarded(torch.zeros(8), torch.zeros(8), 0.1, 0.0, 1.0, rec)
    with pytest.raises(_lib.Mt4Error):
        ops.restore_if_skipped(torch.zeros(8), torch.zeros(8), rec)


# ------------------------------------------------------------------------------------------------ the epoch loop
class FakeTrainer:
    """steps = [(loss, skipped, norm)] per epoch; `guard_stats` answers like `FlatTrainer.guard_stats`"""

    def __init__(self):
        self.lr, self.epoch, self.seen, self.reads = None, -1, [], 0

    def state_dict(self):
        return {"epoch": torch.tensor(self.epoch)}

    def guard_stats(self, reset=False):
        self.reads += 1
        applied = [n for _, s, n in self.seen if not s]
        out = {"steps": len(self.seen), "skipped": len(self.seen) - len(applied), "clipped": sum(n > 1.0 for n in applied),
               "norm_sum": sum(applied), "norm_max": max(applied, default=0.0), "norm_mean": sum(applied) / len(applied) if applied else 0.0}
        if reset:
            self.seen = []
        return out


def _loop(tmp_path, script, *argv, note=None):
    p = argparse.ArgumentParser()
    add_schedule_flags(p)
    p.add_argument("--clip_grad_norm", type=float, default=0.0)
    p.add_argument("--skip_nonfinite", action="store_true")
    F = p.parse_args(["--epochs", str(len(script))] + list(argv))
    tr = FakeTrainer()

    def train_epoch(epoch):
        tr.epoch = epoch
        tot = LossMean(F.skip_nonfinite)
        for step in script[epoch]:
            tr.seen.append(step)
            tot.add(step[0])
        return tot.total, tot.steps

    log = tmp_path / "run" / "m.log"
    res = run_epochs(F, tr, 0, train_epoch, lambda state: (0.5, "ivt: [0.50000]"), str(log), str(tmp_path / "run" / "m_latest.pth"),
                     str(tmp_path / "run" / "m.pth"), latest_every_epoch=True, epoch_note=note)
    return tr, log.read_text(), res


NAN = float("nan")


def test_epoch_note_appears_only_with_a_flag(tmp_path):
    script = [[(1.0, False, 0.5), (3.0, False, 2.0)], [(2.0, False, 4.0)]]
    tr, log, res = _loop(tmp_path / "off", script)
    assert "gnorm" not in log and "skipped" not in log and tr.reads == 0 and res["loss"] == 2.0
    assert "| epoch 0 | loss 2.0000 | " in log
    tr, log, res = _loop(tmp_path / "clip", script, "--clip_grad_norm", "1.0", note=lambda: " | cache 1/2")
    lines = [ln for ln in log.splitlines() if ln.startswith("Traning")]
    assert lines[0].endswith(" secs | cache 1/2 | gnorm mean 1.25 max 2 | clipped 1 | skipped 0")
    assert lines[1].endswith(" secs | cache 1/2 | gnorm mean 4 max 4 | clipped 1 | skipped 0")          # counters are per epoch
    assert tr.reads == 2                                                                             # one read per epoch
    tr, log, _ = _loop(tmp_path / "skip", script, "--skip_nonfinite")
    assert log.count("| clipped ") == 2 and log.count("| skipped 0") == 2


def test_mean_loss_leaves_out_nonfinite_steps(tmp_path):
    script = [[(1.0, False, 1.0), (NAN, True, 0.0), (4.0, False, 1.0), (float("inf"), True, 0.0)]]
    _, log, res = _loop(tmp_path / "on", script, "--skip_nonfinite")
    assert res["loss"] == 2.5 and "| loss 2.5000 |" in log and log.rstrip().splitlines()[0].endswith("| skipped 2")
    _, log, res = _loop(tmp_path / "off", script, "--clip_grad_norm", "5")                           # without the flag: the plain mean, as today
    assert math.isnan(res["loss"]) and "| loss nan |" in log
    acc = LossMean(False)
    for v in (1.0, 2.0, 4.5):
        acc.add(v)
    assert (acc.total, acc.steps) == (0.0 + 1.0 + 2.0 + 4.5, 3)


def test_an_all_skipped_epoch_raises_before_anything_is_replaced(tmp_path, monkeypatch):
    script = [[(1.0, False, 1.0)], [(NAN, True, 0.0), (NAN, True, 0.0)], [(1.0, False, 1.0)]]
    replaced = []
    real = os.replace
    monkeypatch.setattr(os, "replace", lambda a, b: (replaced.append(os.path.basename(b)), real(a, b))[1])
    with pytest.raises(RuntimeError) as e:
        _loop(tmp_path, script, "--skip_nonfinite")
    assert "epoch 1" in str(e.value) and "--skip_nonfinite" in str(e.value) and "all 2 steps" in str(e.value)
    assert replaced == ["m_latest.pth", "m.pth"]                                                     # epoch 0's; nothing of epoch 1
    assert int(torch.load(tmp_path / "run" / "m_latest.pth")["epoch"]) == 0
    log = (tmp_path / "run" / "m.log").read_text()
    assert log.count("Traning | lr:") == 1                                                           # the epoch that could not learn logs no line


def test_an_all_skipped_first_epoch_writes_nothing(tmp_path, monkeypatch):
    script = [[(NAN, True, 0.0)]]
    replaced = []
    real = os.replace
    monkeypatch.setattr(os, "replace", lambda a, b: (replaced.append(b), real(a, b))[1])
    with pytest.raises(RuntimeError, match="--skip_nonfinite"):
        _loop(tmp_path, script, "--skip_nonfinite")
    assert replaced == [] and not (tmp_path / "run").exists()
