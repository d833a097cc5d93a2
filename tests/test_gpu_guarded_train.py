"""GPU: --clip_grad_norm / --skip_nonfinite through the four trainers (`FlatTrainer.apply_update`): the norm over the flat gradient buffer is the
norm over the reference-shaped gradients (row padding, zero K columns and reserved slots hold exact zeros), a step on a poisoned input changes
nothing and leaves no trace in the next one, a clip that bites is the host restatement's update and one that does not is the plain update's
bits, hipGraph replay and two data-parallel ranks decide alike, and `Temporal_tenco/run.py -t` logs the note.  The smallest configurations of
the trainers' own step tests.  Non-finite numbers here are DATA fed to correct kernels."""
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

import test_gpu_deterministic_train as tdet
import test_gpu_mstct_train as tm
import test_gpu_q2l_train as tq
import test_gpu_train as tg
import test_gpu_train2d as t2
from computervision_codes_amd import shapes, synth
from conftest import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32
INF, NAN = float("inf"), float("nan")
Q2L_CFG = dict(backbone="swin_T_224_1k", img=224, hidden=768, loss_type="v", B=2, seed=811, lr=0.05)
CNN_CFG = dict(network="resnet18", B=4, H=64, W=96, seed=77, lr=0.05, rates=(1.0, 0.5, 2.0))
KINDS = [("tenco", F32), ("mstct", F32), ("mstct", BF), ("q2l", F32), ("q2l", BF), ("student", F32), ("student", BF)]
IDS = [f"{k}_{'bf16' if d == BF else 'fp32'}" for k, d in KINDS]
DETERMINISTIC = ("tenco", "student")                       # the trainers with the mode: twins agree bit for bit


class Rig:
    """a trainer of `kind` with the smallest configuration of its own step test, and `step(bad, **kw)`: one train_step on the clean inputs or on
    inputs with one +Inf (NaN labels where the frames are uint8); -> the loss"""

    def __init__(self, kind, operands, cuda, **kw):
        self.kind = kind
        if kind == "tenco":
            from computervision_codes_amd.tenco_train import TencoTrainer
            _, c = load_golden("tenco_train_small")
            sd = synth.fill_from_shapes(shapes.tenco_shapes(c["num_layers_PG"], c["num_layers_R"], c["num_R"], c["num_f_maps"], c["dim"], 100, fpn=True),
                                        seed=c["seed"])
            self.tr = TencoTrainer(c["num_layers_PG"], c["num_layers_R"], c["num_R"], c["num_f_maps"], c["dim"], lr=c["lr"], weight_decay=1e-5,
                                   deterministic=True, **kw).load_state_dict(sd)
            x = synth.synthetic_features(c["T"], c["dim"], seed=c["seed"]).to(cuda)
            z = self.tr.prepare_labels(tg._labels(c["seed"], c["T"]))
            self.args, self.bad = (x, z), (self._poison(x), z)
        elif kind == "mstct":
            from computervision_codes_amd.mstct_train import MstctTrainer
            _, c = load_golden("mstct_train_tiny")
            sd = synth.fill_from_shapes(shapes.mstct_shapes(c["D"], c["inter"], 2, 8, c["final"], c["loss_type"]), seed=c["seed"])
            self.tr = MstctTrainer(c["inter"], 2, 8, 8, c["D"], c["final"], c["loss_type"], lr=c["lr"], weight_decay=1e-5, operand_dtype=operands,
                                   **kw).load_state_dict(sd)
            x, y = tm._inputs(c)
            x = x.to(cuda)
            self.args, self.bad = (x, y), (self._poison(x), y)
        elif kind == "q2l":
            from computervision_codes_amd.q2l_train import Q2LTrainer
            c = Q2L_CFG
            sd = synth.fill_from_shapes(shapes.q2l_param_shapes(c["backbone"], c["img"], c["hidden"], c["loss_type"]), seed=c["seed"])
            self.tr = Q2LTrainer(c["backbone"], c["img"], c["hidden"], c["loss_type"], lr=c["lr"], weight_decay=1e-5, operand_dtype=operands,
                                 **kw).load_state_dict(sd)
            img, y = tq._inputs(c)
            img = img.to(cuda)
            self.args, self.bad = (img, y), (self._poison(img), y)
        else:
            from computervision_codes_amd.spatial_cnn_train import SpatialCnnTrainer
            c = CNN_CFG
            sd = synth.fill_from_shapes(shapes.spatial_cnn_shapes(c["network"]), seed=c["seed"])
            self.tr = SpatialCnnTrainer(c["network"], lr=c["lr"], weight_decay=1e-5, rates=c["rates"], temp=4.0, operand_dtype=operands,
                                        deterministic=True, **kw).load_state_dict(sd)
            _, labels, tpred, tfeat = t2._inputs(c)
            frames = synth.synthetic_frames(c["B"], c["H"], c["W"], seed=c["seed"]).to(cuda)
            assert frames.dtype == torch.uint8
            z = torch.cat([l.float() for l in labels], 1).contiguous().to(cuda)
            zb = z.clone()
            zb[1, 3] = NAN                                   # the frames are uint8: the poison is a NaN label
            self.args, self.bad = (frames, z, tpred, tfeat), (frames, zb, tpred, tfeat)

    @staticmethod
    def _poison(x):
        x = x.clone()
        x.view(-1)[x.numel() // 3] = INF
        return x

    def step(self, bad=False, **kw):
        out = self.tr.train_step(*(self.bad if bad else self.args), **kw)
        return out[0] if isinstance(out, tuple) else out["loss"] if isinstance(out, dict) else out

    def state(self):
        """state_dict() without `num_batches_tracked` (a host integer: it counts a skipped step too)"""
        return {k: v for k, v in self.tr.state_dict().items() if not k.endswith("num_batches_tracked")}


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    """equal bit for bit"""
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(_bytes(a[k]), _bytes(b[k])), k


@pytest.mark.parametrize("kind,operands", KINDS, ids=IDS)
def test_flat_norm_clip_and_loose_clip(cuda, kind, operands):
    from computervision_codes_amd import ops
    r = Rig(kind, operands, cuda, clip_grad_norm=1e9)
    tr = r.tr
    loss = r.step(apply_update=False)
    assert math.isfinite(loss)
    # --- the norm over flat G (padding rows, zero K columns, reserved slots included) == the norm over the reference-shaped gradients
    n = tr.G.numel()
    ws, state, stats = ops.guard_buffers(n, cuda)
    ops.grad_guard(tr.G, 1.0, 0.0, False, ws, state, stats)
    st = ops.read_guard_state(state)
    shaped = math.fsum(float((g.double() ** 2).sum()) for g in tr.grads().values())
    print(f"{kind}: n={n} flat sumsq {st['sumsq']!r} reference-shaped {shaped!r} rel {abs(st['sumsq'] - shaped) / shaped:.3e}")
    # the device: (n - 1) 2^-53 (additions of exact squares); torch's float64 sums over the shaped tensors: the same bound again, and fsum over them exact
    assert abs(st["sumsq"] - shaped) <= 2 * (n - 1) * 2.0 ** -53 * shaped and st["nonfinite"] == 0
    norm = math.sqrt(shaped)
    # --- max_norm 1e9: the bits of the plain update
    P0, G = tr.P.clone(), tr.G.clone()
    tr.apply_update()
    want = P0.clone()
    ops.sgd_step(want, G, tr.lr, tr.wd, 1.0)
    assert torch.equal(tr.P.view(torch.int32), want.view(torch.int32)) and torch.equal(tr.G, G)
    gs = tr.guard_state()
    assert gs["coef"] == 1.0 and gs["skip"] == 0 and abs(gs["norm"] - norm) <= 1e-9 * norm
    assert tr.guard_stats() == {"steps": 1, "skipped": 0, "clipped": 0, "norm_sum": gs["norm"], "norm_max": gs["norm"], "norm_mean": gs["norm"]}
    # --- max_norm = half the measured norm: the host restatement applied to G / P, within fp32 rounding of the update
    r.step(apply_update=False)
    P0, G = tr.P.clone(), tr.G.clone()
    tr.clip_grad_norm = 0.5 * float(G.double().norm())
    tr.apply_update()
    host, info = ops.guarded_sgd_host(P0, G, tr.lr, tr.wd, 1.0, tr.clip_grad_norm, False)
    gs = tr.guard_state()
    assert gs["coef"] < 1.0 and abs(gs["coef"] - info["coef"]) <= 2.0 ** -23 * info["coef"] and tr.guard_stats(reset=True)["clipped"] == 1
    bound = 2.0 ** -22 * (P0.cpu().abs() + tr.lr * G.cpu().abs())
    d = (tr.P.cpu() - host).abs()
    assert bool((d <= bound).all()), float((d - bound).max())
    assert tr.guard_stats()["steps"] == 0                    # reset


@pytest.mark.parametrize("kind,operands", KINDS, ids=IDS)
def test_skipped_step_changes_nothing_and_leaves_no_trace(cuda, kind, operands):
    a = Rig(kind, operands, cuda, skip_nonfinite=True)
    before = a.state()
    stats0 = a.tr.running_stats() if kind == "student" else None
    loss = a.step(bad=True)
    assert not math.isfinite(loss)
    gs = a.tr.guard_state()
    assert gs["skip"] == 1 and gs["nonfinite"] >= 1 and gs["coef"] == 1.0
    _same(a.state(), before)
    if kind == "student":
        now = a.tr.running_stats()
        for k in now:
            if k.endswith("num_batches_tracked"):
                assert int(now[k]) == int(stats0[k]) + 1, k  # advances for a skipped step too, as torch's under GradScaler
            else:
                assert torch.equal(now[k].view(torch.int32), stats0[k].view(torch.int32)), k
    assert a.tr.guard_stats()["skipped"] == 1 and a.tr.guard_stats()["steps"] == 1
    # the next clean step
    loss = a.step()
    assert math.isfinite(loss) and a.tr.guard_state()["skip"] == 0 and a.tr.guard_stats()["skipped"] == 1 and a.tr.guard_stats()["steps"] == 2
    after = a.state()
    assert all(bool(torch.isfinite(v.float()).all()) for v in after.values())
    assert any(not torch.equal(after[k], before[k]) for k in after)
    if kind in DETERMINISTIC:                                # ... gives the parameters of a twin that never saw the bad batch, bit for bit
        b = Rig(kind, operands, cuda, skip_nonfinite=True)
        b.step()
        _same(after, b.state())
        assert torch.equal(a.tr.P.view(torch.int32), b.tr.P.view(torch.int32))
    # the same input without the flag: applied as today
    a.tr.skip_nonfinite = False
    a.tr.clip_grad_norm = 1.0
    a.step(bad=True)
    gs = a.tr.guard_state()
    assert gs["skip"] == 0 and gs["nonfinite"] >= 1 and gs["coef"] == 1.0 and not bool(torch.isfinite(a.tr.P).all())


@pytest.mark.parametrize("clip,skip", [(True, False), (False, True), (True, True)], ids=["clip", "skip", "both"])
def test_graph_replay_gives_the_bits_of_eager(cuda, clip, skip):
    plain = Rig("tenco", F32, cuda, clip_grad_norm=1e9)
    plain.step(apply_update=False, draws=(41, 0))
    flags = dict(clip_grad_norm=0.25 * float(plain.tr.G.double().norm()) if clip else 0.0, skip_nonfinite=skip)     # a quarter of the first norm: bites
    e, g = Rig("tenco", F32, cuda, **flags), Rig("tenco", F32, cuda, **flags)
    seq = [False, True, False] if skip else [False, False]
    for i, bad in enumerate(seq):
        le, lg = e.step(bad=bad, draws=(41, i)), g.step(bad=bad, draws=(41, i), use_graph=True)
        assert (le == lg) or (math.isnan(le) and math.isnan(lg)), (i, le, lg)
        assert torch.equal(e.tr.P.view(torch.int32), g.tr.P.view(torch.int32)), i
        assert torch.equal(e.tr._guard[1].view(torch.int64), g.tr._guard[1].view(torch.int64)), i    # the same decisions, bit for bit
        assert e.tr.guard_state()["skip"] == int(bad)
    assert len(g.tr._graphs) == 1 and e.tr.guard_stats() == g.tr.guard_stats()
    assert e.tr.guard_stats()["skipped"] == sum(seq) and (e.tr.guard_stats()["clipped"] >= 1) == clip
    # a twin without the flags in effect (max_norm 1e9) against one without the flags at all: bit for bit
    from computervision_codes_amd.tenco_train import TencoTrainer
    none = Rig("tenco", F32, cuda)
    assert isinstance(none.tr, TencoTrainer) and not none.tr.guarded and plain.tr.guarded
    for i in range(2):
        assert plain.step(draws=(41, i)) == none.step(draws=(41, i))
    _same(plain.state(), none.state())
    assert none.tr._guard is None                            # nothing allocated on the default path


def test_two_ranks_skip_alike(cuda, tmp_path):
    """rank 1's video holds one +Inf: NaN and Inf survive the sum all-reduce, so both ranks skip without another collective; the clean step
    behind it is sgd of the mean gradient"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    from ddp_guarded_worker import trainer, video
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29541", os.path.join(ROOT, "tests", "helpers", "ddp_guarded_worker.py"), str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    got = [torch.load(tmp_path / f"ddp_guarded_rank{rank}.pth", map_location="cpu") for rank in (0, 1)]
    for rank in (0, 1):
        assert got[rank]["stats_bad"]["skipped"] == 1 and got[rank]["stats_bad"]["steps"] == 1, rank
        assert got[rank]["state_bad"]["skip"] == 1 and got[rank]["state_bad"]["nonfinite"] >= 1
        _same(got[rank]["after_bad"], got[rank]["before"])                                           # unchanged
        assert got[rank]["stats"]["skipped"] == 1 and got[rank]["stats"]["steps"] == 2
    _same(got[0]["after_bad"], got[1]["after_bad"])
    _same(got[0]["after_clean"], got[1]["after_clean"])                                              # identical on both ranks
    assert got[0]["stats"] == got[1]["stats"]
    trs = []
    for rank in (0, 1):
        tr = trainer()
        x, labels = video(rank)
        tr.train_step(x.to(cuda), labels, apply_update=False)
        trs.append(tr)
    trs[0].G.add_(trs[1].G).mul_(0.5)
    trs[0].apply_update()
    want = trs[0].state_dict()
    for k in want:
        assert (got[0]["after_clean"][k].float() - want[k].float()).abs().max().item() <= 2e-6 * max(1.0, want[k].float().abs().max().item()), k


# ------------------------------------------------------------------------------------------------ the driver
def _tenco_run(top, extra):
    tree, data = top / "MT4MTLKD", str(top / "CholecT45")
    shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
    tdet._make_temporal_dataset(tree, data, 300)
    r = subprocess.run([sys.executable, "run.py", "-t", "--fpn", "--mask", "--mask_draw", "device", "--deterministic", "--num_layers_PG", "3",
                        "--num_layers_R", "2", "--input_dim", "512", "--loss_type", "all", "--epochs", "2", "-l", "1e-2", "5e-3", "1e-2",
                        "-w", "9", "18", "200", "--version", "S_TCN", "--version1", "S", "--data_dir", data, "--kfold", "1", "--seed", "7"] + extra,
                       cwd=tree / "Temporal_tenco", env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    ck = tree / "Temporal_tenco" / "__checkpoint__" / "run_S_TCN" / "rendezvous_l8_cholectcholect45-crossval_k1_batchnorm_lowres_latest.pth"
    return r.stdout, open(str(ck).replace("_latest.pth", ".log")).read(), open(ck, "rb").read()


def test_driver_runs_with_a_biting_clip_repeat_and_log_the_note(cuda, tmp_path):
    flags = ["--clip_grad_norm", "0.01", "--skip_nonfinite"]
    (out_a, log_a, ck_a), (out_b, log_b, ck_b) = _tenco_run(tmp_path / "a", flags), _tenco_run(tmp_path / "b", flags)
    out_c, log_c, ck_c = _tenco_run(tmp_path / "c", [])
    lines = lambda log: [ln.split(" secs")[0].rsplit(" | ", 1)[0] + ln.split(" secs", 1)[1] for ln in log.splitlines() if ln.startswith("Traning | lr:")]
    la, lb, lc = lines(log_a), lines(log_b), lines(log_c)
    assert len(la) == 2 and la == lb, (la, lb)                                                       # the same lines (but the seconds)
    assert ck_a == ck_b                                                                              # the same `_latest.pth` bytes
    assert out_a.count("guarded update:") == 1 and "--clip_grad_norm 0.01" in out_a and "--skip_nonfinite" in out_a
    for ln in la:
        assert " | gnorm mean " in ln and " max " in ln and ln.endswith(" | skipped 0"), ln
        clipped = int(ln.split("| clipped ")[1].split(" |")[0])
        assert clipped > 0, ln                                                                       # 0.01 bites
    assert "guarded update" not in out_c and all("gnorm" not in ln and "skipped" not in ln for ln in log_c.splitlines())
    assert len(lc) == 2 and ck_c != ck_a
