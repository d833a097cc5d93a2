"""GPU: the weight average through the four trainers (`FlatTrainer(ema=Ema(...))`, `_ema_update`): after every `apply_update` each tensor of
`ema_state_dict()` is the host restatement applied to the previous one and the new `state_dict()` tensor, bit for bit (the student's averaged
running statistics included); the default construction allocates nothing and leaves P's bits alone; hipGraph replay gives the eager bits; a
skipped step leaves the average and its count alone and no trace in the next one; twins agree; the export round-trips; two data-parallel ranks
hold the same average without exchanging it.  The smallest configurations of the trainers' own step tests (`Rig`).  Non-finite numbers here are
DATA fed to correct kernels."""
import math
import os
import subprocess
import sys

import pytest
import torch

from computervision_codes_amd.flatparams import Ema
from test_gpu_guarded_train import DETERMINISTIC, IDS, KINDS, Rig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
FRESH = {"t": 0, "decay": 0.0, "comp": 1.0}
FP32_KINDS = [(k, d) for k, d in KINDS if d == F32]
FP32_IDS = [k for k, _ in FP32_KINDS]


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    """equal bit for bit"""
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), k


def _averaged(tr):
    """what of the trainer is averaged, as device clones: E (and the student's averaged running statistics)"""
    out = {"E": tr.fp.S["ema"].clone()}
    if getattr(tr, "_rstats_ema", None) is not None:
        out["rstats"] = tr._rstats_ema.clone()
    return out


@pytest.mark.parametrize("kind,operands", KINDS, ids=IDS)
def test_every_step_is_the_host_restatement_of_the_exported_tensors(cuda, kind, operands):
    from computervision_codes_amd import ops
    r = Rig(kind, operands, cuda, ema=Ema(0.9))
    tr = r.tr
    prev, rec = tr.ema_state_dict(), dict(FRESH)
    _same(prev, tr.state_dict())                                 # the average starts as a copy of the loaded weights
    assert tr.ema_record() == rec and tr.ema_config() == {"decay": 0.9, "warmup": False}
    verbatim = set(getattr(tr, "_extra", {}))
    for step in range(3):
        assert math.isfinite(r.step())
        rec = ops.ema_advance_host(rec, 0.9, False)
        assert tr.ema_record() == rec, step
        new, now = tr.state_dict(), tr.ema_state_dict()
        assert list(now.keys()) == list(new.keys())
        moved = 0
        for k in now:
            assert now[k].dtype == new[k].dtype and now[k].shape == new[k].shape, k
            if k.endswith("num_batches_tracked") or k in verbatim:   # the trainer's own integer; parameters it keeps verbatim
                assert torch.equal(now[k], new[k]), k
                continue
            want = ops.ema_step_host(prev[k], new[k], rec)
            assert torch.equal(_bits(now[k]), _bits(want)), (step, k)
            moved += int(not torch.equal(_bits(now[k]), _bits(new[k])))
        assert moved > len(now) // 2                             # the average lags the weights
        if kind == "student":
            assert any(k.endswith("running_mean") for k in now) and any(k.endswith("running_var") for k in now)
        # padding columns, padding rows and reserved slots: exact zeros wherever P and G are
        E, quiet = tr.fp.S["ema"], (tr.P == 0) & (tr.G == 0)
        assert bool(quiet.any()) and bool((E[quiet].view(torch.int32) == 0).all())
        prev = now


@pytest.mark.parametrize("kind,operands", KINDS, ids=IDS)
def test_default_construction_keeps_nothing_and_the_average_leaves_p_alone(cuda, kind, operands):
    rigs = [Rig(kind, operands, cuda), Rig(kind, operands, cuda, ema=Ema()), Rig(kind, operands, cuda, ema=Ema(0.9, True))]
    for r in rigs[:2]:
        assert r.tr.ema is None and r.tr._estate is None and "ema" not in r.tr.fp.S and r.tr.ema_config() is None and r.tr.ema_record() == {}
        with pytest.raises(ValueError):
            r.tr.ema_state_dict()
    assert "ema" in rigs[2].tr.fp.S
    for r in rigs:
        for _ in range(2):
            r.step()
    for r in rigs[:2]:
        assert "ema" not in r.tr.fp.S and r.tr._estate is None   # nothing was allocated on the way
    if kind in DETERMINISTIC:                                    # twins agree bit for bit there: today's trainer, Ema(), and one that averages
        for r in rigs[1:]:
            assert torch.equal(rigs[0].tr.P.view(torch.int32), r.tr.P.view(torch.int32))
            _same(rigs[0].tr.state_dict(), r.tr.state_dict())


@pytest.mark.parametrize("kind", ["tenco", "student"])
def test_graph_replay_gives_the_bits_of_eager(cuda, kind):
    e, g = Rig(kind, F32, cuda, ema=Ema(0.9, True)), Rig(kind, F32, cuda, ema=Ema(0.9, True))
    kw = (lambda i: dict(draws=(41, i))) if kind == "tenco" else (lambda i: {})
    for i in range(3):
        le, lg = e.step(**kw(i)), g.step(use_graph=True, **kw(i))
        assert le == lg, (i, le, lg)
        assert torch.equal(e.tr.P.view(torch.int32), g.tr.P.view(torch.int32)), i
        a, b = _averaged(e.tr), _averaged(g.tr)
        assert a.keys() == b.keys() and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a), i
        assert e.tr.ema_record() == g.tr.ema_record() and e.tr.ema_record()["t"] == i + 1
    assert len(g.tr._graphs) >= 1 and not torch.equal(e.tr.fp.S["ema"], e.tr.P)


@pytest.mark.parametrize("kind,operands", KINDS, ids=IDS)
def test_skipped_step_stays_out_of_the_average_and_leaves_no_trace(cuda, kind, operands):
    a = Rig(kind, operands, cuda, skip_nonfinite=True, ema=Ema(0.9))
    a.step()                                                     # one clean step first: the average differs from the weights
    before, rec = _averaged(a.tr), a.tr.ema_record()
    assert rec["t"] == 1
    loss = a.step(bad=True)
    assert not math.isfinite(loss) and a.tr.guard_state()["skip"] == 1
    now = _averaged(a.tr)
    assert all(torch.equal(now[k].view(torch.int32), before[k].view(torch.int32)) for k in before)   # E and the averaged statistics
    assert a.tr.ema_record() == rec                                                                   # ... and t
    assert math.isfinite(a.step()) and a.tr.guard_state()["skip"] == 0 and a.tr.ema_record()["t"] == 2
    after = _averaged(a.tr)
    assert all(bool(torch.isfinite(v).all()) for v in after.values()) and not torch.equal(after["E"], before["E"])
    if kind in DETERMINISTIC:                                    # ... equals that of a twin that never saw the poisoned one, bit for bit
        b = Rig(kind, operands, cuda, skip_nonfinite=True, ema=Ema(0.9))
        b.step()
        b.step()
        twin = _averaged(b.tr)
        assert all(torch.equal(after[k].view(torch.int32), twin[k].view(torch.int32)) for k in after)
        assert b.tr.ema_record() == a.tr.ema_record()
    # without the guard the same input enters the average and stays there
    a.tr.skip_nonfinite = False
    a.tr.clip_grad_norm = 1.0
    a.step(bad=True)
    assert a.tr.ema_record()["t"] == 3 and not bool(torch.isfinite(a.tr.fp.S["ema"]).all())


@pytest.mark.parametrize("kind", DETERMINISTIC)
def test_twins_agree_in_every_bit_of_the_average(cuda, kind):
    a, b = Rig(kind, F32, cuda, ema=Ema(0.99, True)), Rig(kind, F32, cuda, ema=Ema(0.99, True))
    for _ in range(3):
        assert a.step() == b.step()
    x, y = _averaged(a.tr), _averaged(b.tr)
    assert all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in x) and a.tr.ema_record() == b.tr.ema_record()
    _same(a.tr.ema_state_dict(), b.tr.ema_state_dict())


@pytest.mark.parametrize("kind,operands", FP32_KINDS, ids=FP32_IDS)
def test_export_round_trip_restores_buffer_and_record(cuda, kind, operands):
    from computervision_codes_amd import ops
    r = Rig(kind, operands, cuda, ema=Ema(0.9, True))
    tr = r.tr
    for _ in range(2):
        r.step()
    exp, kept, rec = tr.ema_export(), _averaged(tr), tr.ema_record()
    assert exp["ema"] == {"decay": 0.9, "warmup": True} and exp["t"] == rec["t"] == 2 and sorted(exp) == ["ema", "state", "t"]
    _same(exp["state"], tr.ema_state_dict())
    tr.fp.S["ema"].fill_(3.0)                                    # both are overwritten ...
    if "rstats" in kept:
        tr._rstats_ema.fill_(-2.0)
    ops.write_ema_state(tr._estate, 7, 0.25, 0.75)
    tr.load_ema_export(exp)                                      # ... and come back bit for bit, padding zeros included
    now = _averaged(tr)
    assert all(torch.equal(now[k].view(torch.int32), kept[k].view(torch.int32)) for k in kept) and tr.ema_record() == rec
    with pytest.raises(ValueError, match="does not belong"):
        tr.load_ema_export(dict(exp, ema={"decay": 0.9, "warmup": False}))
    with pytest.raises(ValueError, match="other tensors"):
        tr.load_ema_export(dict(exp, state={k: v for k, v in list(exp["state"].items())[1:]}))
    now = _averaged(tr)
    assert all(torch.equal(now[k].view(torch.int32), kept[k].view(torch.int32)) for k in kept)       # a refused load changed nothing
    with pytest.raises(ValueError):
        Rig(kind, operands, cuda).tr.load_ema_export(exp)        # a trainer without an average takes none


def test_two_ranks_hold_the_same_average_without_exchanging_it(cuda, tmp_path):
    """... and it is the average a one-rank trainer takes from the same exchanged gradient: the all-reduce leaves the SUM in G, the mean is
    G x 1/2 -- an exact scaling, so the one-rank update from G / 2 has the two-rank update's bits"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    from ddp_ema_worker import EMA
    from ddp_guarded_worker import trainer
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29551", os.path.join(ROOT, "tests", "helpers", "ddp_ema_worker.py"), str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    got = [torch.load(tmp_path / f"ddp_ema_rank{rank}.pth", map_location="cpu") for rank in (0, 1)]
    one = trainer(deterministic=True, ema=EMA)
    for a, b in zip(got[0]["snaps"], got[1]["snaps"]):
        assert torch.equal(_bits(a["E"]), _bits(b["E"])) and torch.equal(_bits(a["P"]), _bits(b["P"])) and a["record"] == b["record"]
        one.G.copy_((a["G"] * 0.5).to(cuda))
        one.apply_update()
        assert torch.equal(_bits(one.P), _bits(a["P"])) and torch.equal(_bits(one.fp.S["ema"]), _bits(a["E"])) and one.ema_record() == a["record"]
    assert got[0]["snaps"][-1]["record"]["t"] == 2 and not torch.equal(got[0]["snaps"][-1]["E"], got[0]["snaps"][-1]["P"])
    _same(got[0]["ema_state_dict"], got[1]["ema_state_dict"])
    _same(got[0]["ema_state_dict"], one.ema_state_dict())
