"""CPU: optimizer state of the flat trainers (--momentum, --nesterov, --optimizer adamw).  The five flags on all four trainer parsers and the
refusals of `drivers._optim` before any model is built; the host restatement `ops.optim_step_host` (the contract the kernels are held to bit for
bit on the GPU) against torch.optim.SGD / torch.optim.AdamW run in float64, one step at a time, within a per-element bound derived from the
stated operation order; and the --resume plumbing of `trainloop` with a fake trainer that keeps optimizer state."""
import argparse
import json
import os
import random

import numpy as np
import pytest
import torch

from computervision_codes_amd import drivers, ops, trainloop
from computervision_codes_amd.flatparams import Optim
from computervision_codes_amd.trainloop import add_schedule_flags, run_epochs

STAGES = ("spatial_cnn", "spatial_transformer", "mstct", "tenco")
U = 2.0 ** -24                                                     # one float32 rounding, relative


# ------------------------------------------------------------------------------------------------ flags
@pytest.mark.parametrize("stage", STAGES)
def test_flags_are_declared_on_every_trainer_parser_with_their_defaults(stage):
    F = drivers._parser(stage, True).parse_known_args(["-t"])[0]
    assert (F.momentum, F.nesterov, F.optimizer, F.adam_betas, F.adam_eps) == (0.0, False, "sgd", [0.9, 0.999], 1e-8)
    assert drivers._optim(F) == {"optim": None}                    # the defaults: the existing update, no state
    F = drivers._parser(stage, True).parse_known_args(["-t", "--momentum", "0.9", "--nesterov"])[0]
    assert drivers._optim(F) == {"optim": Optim("sgd", 0.9, True)}
    F = drivers._parser(stage, True).parse_known_args(["-t", "--optimizer", "adamw", "--adam_betas", "0.8", "0.95", "--adam_eps", "1e-6"])[0]
    assert drivers._optim(F) == {"optim": Optim("adamw", 0.0, False, 0.8, 0.95, 1e-6)}
    with pytest.raises(SystemExit):
        drivers._parser(stage, True).parse_known_args(["-t", "--optimizer", "lion"])
    assert "--momentum" not in drivers._parser(stage, False).format_help()       # trainer flags only


def test_the_help_text_cites_the_reference_and_names_the_poisoning():
    text = " ".join(drivers._parser("tenco", True).format_help().split())
    for cite in ("Spatial_cnn/run.py:72", "Spatial_transformer/run.py:72", "Temporal_mstct/run.py:73", "Temporal_tenco/run.py:66", "0.95"):
        assert cite in text, cite
    assert text.count("poisons") == 2


def test_the_rule_is_said_once_unless_it_is_plain_sgd(capsys):
    drivers._optim(drivers._parser("mstct", True).parse_known_args([])[0])
    assert capsys.readouterr().out == ""
    drivers._optim(drivers._parser("mstct", True).parse_known_args(["--momentum", "0.9", "--nesterov"])[0])
    out = capsys.readouterr().out
    assert out.count("update rule:") == 1 and "momentum 0.9 nesterov" in out
    drivers._optim(drivers._parser("mstct", True).parse_known_args(["--optimizer", "adamw"])[0])
    assert "update rule: adamw betas (0.9, 0.999) eps 1e-08" in capsys.readouterr().out


BAD = [(["--nesterov"], "--nesterov"), (["--momentum", "1.0"], "--momentum"), (["--momentum", "-0.1"], "--momentum"),
       (["--momentum", "nan"], "--momentum"), (["--optimizer", "adamw", "--momentum", "0.9"], "--momentum"),
       (["--optimizer", "adamw", "--nesterov"], "--nesterov"), (["--optimizer", "adamw", "--adam_betas", "1.0", "0.999"], "--adam_betas"),
       (["--optimizer", "adamw", "--adam_betas", "0.9", "-0.1"], "--adam_betas"), (["--optimizer", "adamw", "--adam_eps", "0"], "--adam_eps")]


@pytest.mark.parametrize("flags,word", BAD, ids=[" ".join(f) for f, _ in BAD])
def test_every_trainer_refuses_before_any_model_is_built(flags, word):
    """no GPU and no dataset here: anything past the refusal would fail differently"""
    argv = ["-t", "--fpn", "--data_dir", "/nonexistent"] + flags
    with pytest.raises(ValueError, match=word):
        drivers.spatial_cnn_train(argv)
    with pytest.raises(ValueError, match=word):
        drivers.spatial_transformer_train(argv)
    with pytest.raises(ValueError, match=word):
        drivers._mstct_train(drivers._parser("mstct", True).parse_known_args(argv)[0])
    with pytest.raises(ValueError, match=word):
        drivers._tenco_train(drivers._parser("tenco", True).parse_known_args(argv)[0])


def test_optim_tuple_checks_and_config():
    assert not Optim().stateful and Optim().buffers == () and Optim("sgd", 0.5).buffers == ("momentum_buffer",)
    assert Optim("adamw").stateful and Optim("adamw").buffers == ("exp_avg", "exp_avg_sq")
    assert Optim("sgd", 0.9, True).config() == {"kind": "sgd", "momentum": 0.9, "nesterov": True}
    assert Optim("adamw").config() == {"kind": "adamw", "beta1": 0.9, "beta2": 0.999, "eps": 1e-8}
    for bad in (Optim("sgd", 1.0), Optim("sgd", 0.0, True), Optim("adamw", 0.9), Optim("adamw", 0.0, False, 1.0), Optim("adamw", eps=0.0), Optim("rms")):
        with pytest.raises(ValueError):
            bad.check()


# ------------------------------------------------------------------------------------------------ the host model against torch in float64
N_EXP = 25                                                         # exponents -12 .. 12
LR, GS, COEF = 0.01, 1.0, 0.75


def _ramps(step):
    """per-element powers of two 2^-12 .. 2^12: g's exponent walks the ramp from step to step (its sign stays: m and g never cancel), p's
    exponent takes five values, the four sign pairs all occur"""
    i = np.arange(N_EXP * 5 * 4)
    ge = (i % N_EXP + 5 * step) % N_EXP - 12
    pe = (i // N_EXP % 5) * 6 - 12
    gs, ps = np.where(i // (N_EXP * 5) % 2 == 0, 1.0, -1.0), np.where(i // (N_EXP * 10) % 2 == 0, 1.0, -1.0)
    return (ps * 2.0 ** pe).astype(np.float32), (gs * 2.0 ** ge).astype(np.float32)


def _all_zero_or_normal(trace):
    tiny = float(np.finfo(np.float32).tiny)
    for k, a in trace.items():
        a = np.abs(np.asarray(a, dtype=np.float64))
        assert np.all(np.isfinite(a)) and np.all((a == 0) | (a >= tiny)), k


def _f(x):
    return float(np.float32(x))


def _torch_step(opt_cls, kw, p, g, state):
    """one step of the float64 optimizer loaded with the fp32 state -> (p, state tensors)"""
    w = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = opt_cls([w], **kw)
    if state is not None:
        opt.load_state_dict({"state": {0: state}, "param_groups": opt.state_dict()["param_groups"]})
    w.grad = torch.from_numpy(g.astype(np.float64))
    opt.step()
    return w.detach().numpy(), opt.state[w]


@pytest.mark.parametrize("momentum", [0.9, 0.5])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_sgd_host_model_against_torch_float64(momentum, nesterov, wd):
    """Rounding count from the stated order (u = 2^-24; D = |g s| + |wd p|, M = |mom m|):
      d = g s + wd p: a rounding per product and one of the sum                                  -> 2u D
      m' = mom m + d: the product, d's error, the sum                                            -> u (2M + 3D) <= 3u (M + D); asserted with k = 4
      plain:    lr m' adds one                                                                   -> 4u lr (M + D);             asserted with k = 5
      nesterov: t = mom m' (4u mom (M + D)), d + t (one more on each), lr (.) one more           -> 6u lr (D + mom (M + D));   asserted with k = 7
      p' = p - lr (.): one rounding of the result                                                -> + u |p'|
    (k + 1: room for the second-order terms).  torch runs with the float32 values of lr, wd and momentum as float64 and the gradient g s."""
    mom32, lr32, wd32, s = _f(momentum), _f(LR), _f(wd), _f(np.float32(GS) * np.float32(COEF))
    kw = dict(lr=lr32, momentum=mom32, dampening=0.0, weight_decay=wd32, nesterov=nesterov)
    p, _ = _ramps(0)
    m = np.zeros_like(p)
    for step in range(6):
        g = _ramps(step)[1]
        trace = {}
        got = ops.optim_step_host("sgd", p, g, m, lr=LR, weight_decay=wd, grad_scale=GS, coef=COEF, momentum=momentum, nesterov=nesterov, trace=trace)
        _all_zero_or_normal(trace)
        # a zeroed m is torch's first step (its buffer starts as d): step 0 runs torch WITHOUT any state
        state = None if step == 0 else {"momentum_buffer": torch.from_numpy(m.astype(np.float64))}
        p_ref, st = _torch_step(torch.optim.SGD, kw, p, g.astype(np.float64) * s, state)
        m_ref = st["momentum_buffer"].numpy()
        p64, D = p.astype(np.float64), np.abs(g.astype(np.float64) * s) + np.abs(wd32 * p.astype(np.float64))
        M = np.abs(mom32 * m.astype(np.float64))
        dm, dp = np.abs(got["m"].numpy() - m_ref), np.abs(got["p"].numpy() - p_ref)
        bm = 4 * U * (M + D)
        bp = (7 * U * lr32 * (D + mom32 * (M + D)) if nesterov else 5 * U * lr32 * (M + D)) + U * np.abs(p_ref)
        assert np.all(dm <= bm) and np.all(dp <= bp), (step, float((dm / bm).max()), float((dp / bp).max()))
        assert np.any(dp > 0) and not np.array_equal(p64, p_ref)
        p, m = got["p"].numpy(), got["m"].numpy()                   # the fp32 state goes on: errors do not compound in the check


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.95)])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adamw_host_model_against_torch_float64(betas, wd):
    """Rounding count (u = 2^-24; h = g s; nothing cancels: m and g keep one sign per element, v and h^2 are positive):
      m' = b1 m + c1 h: h, c1, their product, the sum (b1 m: b1, the product, the sum)           -> 4u (|b1 m| + |c1 h|);  asserted with k = 5
      v' = b2 v + c2 (h h): h twice, h h, c2, the product, the sum                               -> 6u (|b2 v| + |c2 h^2|); asserted with k = 7
      sqrt(v'): half of 6u and its own rounding (4u); / r2: r2's rounding and the quotient's (6u); + eps: the sum (7u, relative to den)
      m' / den: 4u + 7u + the quotient's (12u); step's rounding and the product's                -> 14u |update|;          asserted with k = 15
      q = p - lw p: lw, the product (2u |lw p|; asserted with 3), the difference (u |q|);  p' = q - update: one rounding of the result (u |p'|)
    The double-precision scalars (1 - beta^t from t repeated multiplies against torch's pow) differ by parts in 10^13: nothing at this scale."""
    b1, b2 = betas
    lr32, wd32, eps32, s = _f(LR), _f(wd), _f(1e-8), _f(np.float32(GS) * np.float32(COEF))
    kw = dict(lr=lr32, betas=betas, eps=eps32, weight_decay=wd32, amsgrad=False)
    p, _ = _ramps(0)
    m, v = np.zeros_like(p), np.zeros_like(p)
    rec = {"t": 0, "beta1_pow": 1.0, "beta2_pow": 1.0}
    for step in range(6):
        g = _ramps(step)[1]
        rec = ops.optim_advance_host(rec, b1, b2)
        assert rec["t"] == step + 1 and abs(rec["beta1_pow"] - b1 ** rec["t"]) <= 1e-15 and abs(rec["beta2_pow"] - b2 ** rec["t"]) <= 1e-15
        trace = {}
        got = ops.optim_step_host("adamw", p, g, m, v, lr=LR, weight_decay=wd, grad_scale=GS, coef=COEF, beta1=b1, beta2=b2, eps=1e-8, record=rec,
                                  trace=trace)
        _all_zero_or_normal(trace)
        state = None if step == 0 else {"step": torch.tensor(float(step)), "exp_avg": torch.from_numpy(m.astype(np.float64)),
                                        "exp_avg_sq": torch.from_numpy(v.astype(np.float64))}
        p_ref, st = _torch_step(torch.optim.AdamW, kw, p, g.astype(np.float64) * s, state)
        assert float(st["step"]) == rec["t"]
        m_ref, v_ref = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        p64, h = p.astype(np.float64), g.astype(np.float64) * s
        bm = 5 * U * (np.abs(b1 * m.astype(np.float64)) + np.abs((1 - b1) * h))
        bv = 7 * U * (np.abs(b2 * v.astype(np.float64)) + np.abs((1 - b2) * h * h))
        q = p64 - lr32 * wd32 * p64
        update = np.abs(q - p_ref)                                  # the float64 update term step m' / den
        bp = 15 * U * update + 3 * U * np.abs(lr32 * wd32 * p64) + U * np.abs(q) + U * np.abs(p_ref)
        dm, dv, dp = np.abs(got["m"].numpy() - m_ref), np.abs(got["v"].numpy() - v_ref), np.abs(got["p"].numpy() - p_ref)
        assert np.all(dm <= bm) and np.all(dv <= bv) and np.all(dp <= bp), (step, float((dm / bm).max()), float((dv / bv).max()), float((dp / bp).max()))
        assert np.all(update > 0)
        p, m, v = got["p"].numpy(), got["m"].numpy(), got["v"].numpy()


def test_host_model_skip_and_guard_coefficient():
    p, g = _ramps(0)
    m = np.full_like(p, 0.5)
    out = ops.optim_step_host("sgd", p, g, m, lr=LR, weight_decay=1e-2, momentum=0.9, skip=True)
    assert np.array_equal(out["p"].numpy(), p) and np.array_equal(out["m"].numpy(), m)
    a = ops.optim_step_host("sgd", p, g, m, lr=LR, weight_decay=0.0, momentum=0.9, grad_scale=0.5, coef=0.5)
    b = ops.optim_step_host("sgd", p, g, m, lr=LR, weight_decay=0.0, momentum=0.9, grad_scale=0.25)
    assert np.array_equal(a["p"].numpy(), b["p"].numpy())           # powers of two: the clip scales the gradient ahead of the state
    assert ops.optim_advance_host({"t": 3, "beta1_pow": 0.5, "beta2_pow": 0.25}, 0.9, 0.999, skip=True) == {"t": 3, "beta1_pow": 0.5, "beta2_pow": 0.25}
    with pytest.raises(ValueError):
        ops.optim_step_host("rms", p, g, m, lr=LR, weight_decay=0.0)


# ------------------------------------------------------------------------------------------------ --resume plumbing
SCHEDULE = ["-w", "1", "2", "3", "-l", "0.1", "0.2", "0.05", "--power", "0.2", "--decay_rate", "0.9"]
SGD_CFG, ADAM_CFG = Optim("sgd", 0.9, False).config(), Optim("adamw").config()


class FakeTrainer:
    """weights = the last epoch and a running sum; with `cfg` it also keeps a 'momentum' the sum depends on, so a resumed run ends with the
    same bytes only if the optimizer state came back"""

    def __init__(self, cfg=None):
        self.lr, self.epoch, self.acc, self.cfg, self.mom = None, -1, 0.0, cfg, 0.0

    def state_dict(self):
        return {"epoch": torch.tensor(self.epoch), "acc": torch.tensor(self.acc, dtype=torch.float64)}

    def load_state_dict(self, sd):
        self.epoch, self.acc = int(sd["epoch"]), float(sd["acc"])
        return self

    def optim_config(self):
        return self.cfg

    def optimizer_state_dict(self):
        return None if self.cfg is None else {"optim": self.cfg, "step": self.epoch + 1, "state": {"w": {"momentum_buffer": torch.tensor(self.mom, dtype=torch.float64)}}}

    def load_optimizer_state_dict(self, osd):
        assert osd["optim"] == self.cfg
        self.mom = float(osd["state"]["w"]["momentum_buffer"])


def _flags(*argv, resume=True):
    p = argparse.ArgumentParser()
    add_schedule_flags(p)
    F = p.parse_args(list(argv) + SCHEDULE)
    F.resume = resume
    return F


class Run:
    def __init__(self, tmp_path, F, cfg=None, die_in=None, load=True):
        d = tmp_path / "run"
        self.dir, self.latest, self.best, self.log = d, str(d / "m_latest.pth"), str(d / "m.pth"), d / "m.log"
        tr = self.tr = FakeTrainer(cfg)
        py = random.Random(5)
        resume = trainloop.load_resume(self.latest, 0, 1, optim=cfg) if F.resume else None
        state = drivers._latest_state(self.latest, resume)
        if state is not None:
            tr.load_state_dict(state)
        if load:
            drivers._load_optim(tr, resume)

        def train_epoch(epoch):
            if epoch == die_in:
                raise KeyboardInterrupt
            tr.mom = 0.9 * tr.mom + py.random()
            tr.epoch, tr.acc = epoch, tr.acc + tr.mom * tr.lr
            return tr.acc, 1

        self.result = run_epochs(F, tr, 0, train_epoch, lambda state: (0.5, "ivt: [0.50000]"), str(self.log), self.latest, self.best,
                                 latest_every_epoch=True, generators={"py": py}, resume=resume, world=1)

    def files(self):
        return sorted(os.listdir(self.dir))

    def sidecar(self):
        with open(trainloop.resume_file(self.latest)) as f:
            return json.load(f)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_optimizer_file_is_named_digested_and_two_generations_are_kept(tmp_path):
    r = Run(tmp_path, _flags("--epochs", "1"), SGD_CFG)
    assert r.files() == ["m.log", "m.pth", "m_latest.pth", "m_latest.pth.optim.e0", "m_latest.pth.resume"]
    rec = r.sidecar()["records"][0]
    path = trainloop.optim_file(r.latest, 0)
    assert rec["optim"] == {"file": "m_latest.pth.optim.e0", "digest": trainloop._file_digest(path), "config": SGD_CFG}
    assert torch.load(path)["state"]["w"]["momentum_buffer"] == torch.tensor(r.tr.mom, dtype=torch.float64)
    r = Run(tmp_path, _flags("--epochs", "2"), SGD_CFG)
    assert [x["optim"]["file"] for x in r.sidecar()["records"]] == ["m_latest.pth.optim.e1", "m_latest.pth.optim.e0"]
    assert [f for f in r.files() if ".optim." in f] == ["m_latest.pth.optim.e0", "m_latest.pth.optim.e1"]
    r = Run(tmp_path, _flags("--epochs", "4"), SGD_CFG)             # ... and every older one is removed behind the pair
    assert [f for f in r.files() if ".optim." in f] == ["m_latest.pth.optim.e2", "m_latest.pth.optim.e3"]
    for x in r.sidecar()["records"]:
        assert trainloop._file_digest(os.path.join(r.dir, x["optim"]["file"])) == x["optim"]["digest"]
    assert not [f for f in r.files() if f.endswith(".tmp")]


@pytest.mark.parametrize("cfg", [SGD_CFG, ADAM_CFG], ids=["sgd", "adamw"])
def test_two_plus_two_epochs_end_like_four_and_a_kill_keeps_a_loadable_pair(tmp_path, cfg):
    straight = Run(tmp_path / "a", _flags("--epochs", "4"), cfg)
    Run(tmp_path / "b", _flags("--epochs", "2"), cfg)
    with pytest.raises(KeyboardInterrupt):
        Run(tmp_path / "b", _flags("--epochs", "4"), cfg, die_in=3)
    resumed = Run(tmp_path / "b", _flags("--epochs", "4"), cfg)
    assert _bytes(resumed.latest) == _bytes(straight.latest) and straight.tr.mom == resumed.tr.mom
    assert _bytes(trainloop.optim_file(resumed.latest, 3)) == _bytes(trainloop.optim_file(straight.latest, 3))
    # without the persisted state the momentum restarts at zero and the run ends elsewhere: what the file is for
    Run(tmp_path / "c", _flags("--epochs", "2"), cfg)
    lost = Run(tmp_path / "c", _flags("--epochs", "4"), cfg, load=False)
    assert _bytes(lost.latest) != _bytes(straight.latest)


def test_resume_refusals_name_the_file_and_the_way_out(tmp_path):
    r = Run(tmp_path, _flags("--epochs", "2"), SGD_CFG)
    opt = trainloop.optim_file(r.latest, 1)
    # a record with optimizer state resumed without the flags, or with another rule's
    with pytest.raises(ValueError, match="no optimizer flags.*drop --resume"):
        trainloop.load_resume(r.latest, 0, 1)
    with pytest.raises(ValueError, match="changing the update rule.*drop --resume"):
        trainloop.load_resume(r.latest, 0, 1, optim=ADAM_CFG)
    with pytest.raises(ValueError, match="changing the update rule"):
        trainloop.load_resume(r.latest, 0, 1, optim=Optim("sgd", 0.5).config())
    assert trainloop.load_resume(r.latest, 0, 1, optim=SGD_CFG).optim_state()["step"] == 2
    # its bytes have another digest
    data = _bytes(opt)
    with open(opt, "wb") as f:
        f.write(data[:-1] + bytes([data[-1] ^ 1]))
    with pytest.raises(ValueError, match=r"optim\.e1.*replaced or its write was torn.*drop --resume"):
        trainloop.load_resume(r.latest, 0, 1, optim=SGD_CFG)
    # it is missing
    os.remove(opt)
    with pytest.raises(ValueError, match=r"optim\.e1.*is missing.*drop --resume"):
        trainloop.load_resume(r.latest, 0, 1, optim=SGD_CFG)
    # optimizer flags on a record without "optim"
    plain = Run(tmp_path / "plain", _flags("--epochs", "1"), None)
    with pytest.raises(ValueError, match="holds no optimizer state.*Drop --momentum"):
        trainloop.load_resume(plain.latest, 0, 1, optim=SGD_CFG)
    assert trainloop.load_resume(plain.latest, 0, 1).optim_state is None


def test_runs_without_optimizer_state_or_without_resume_write_what_they_wrote(tmp_path):
    """a trainer that keeps no state (None) and one that has never heard of optimizer state write byte-identical sidecars in today's format:
    records of exactly epoch, top, digest, generators"""
    class Old:                                                      # the fake trainer of tests/test_resume_cpu.py: no optimizer methods at all
        def __init__(self):
            self.lr, self.epoch, self.acc = None, -1, 0.0
        state_dict, load_state_dict = FakeTrainer.state_dict, FakeTrainer.load_state_dict

    def run(d, tr):
        py = random.Random(5)

        def train_epoch(epoch):
            tr.epoch, tr.acc = epoch, tr.acc + py.random() * tr.lr
            return tr.acc, 1
        run_epochs(_flags("--epochs", "3"), tr, 0, train_epoch, lambda s: (0.5, "ivt: [0.50000]"), str(d / "m.log"), str(d / "m_latest.pth"),
                   str(d / "m.pth"), latest_every_epoch=True, generators={"py": py}, world=1)
        return _bytes(str(d / "m_latest.pth.resume")), sorted(os.listdir(d))
    a, files_a = run(tmp_path / "a", Old())
    b, files_b = run(tmp_path / "b", FakeTrainer(None))
    assert a == b and files_a == files_b == ["m.log", "m.pth", "m_latest.pth", "m_latest.pth.resume"]
    obj = json.loads(a)
    assert sorted(obj) == ["format", "records", "world"] and obj["format"] == 1
    assert all(sorted(r) == ["digest", "epoch", "generators", "top"] for r in obj["records"]) and len(obj["records"]) == 2
    # without --resume: no optimizer file, no sidecar, though the trainer has state
    r = Run(tmp_path / "c", _flags("--epochs", "2", resume=False), SGD_CFG)
    assert r.files() == ["m.log", "m.pth", "m_latest.pth"]
