"""CPU: the weight average of the flat trainers (--ema_decay, --ema_warmup, --ema_eval).  The three flags on all four trainer parsers and the
refusals of `drivers._ema` before any model is built; the host restatements `ops.ema_advance_host` / `ops.ema_step_host` (the contract the
kernels are held to bit for bit on the GPU) against the definition in float64; the argument checks of the two entry points, which run before any
launch; and the plumbing of `trainloop.run_epochs` with a fake trainer that keeps an average."""
import argparse
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from computervision_codes_amd import _lib, drivers, ops, trainloop
from computervision_codes_amd.flatparams import Ema
from computervision_codes_amd.trainloop import add_schedule_flags, run_epochs
from test_optimizer_state_cpu import _all_zero_or_normal, _ramps

STAGES = ("spatial_cnn", "spatial_transformer", "mstct", "tenco")
U = 2.0 ** -24                                                     # one float32 rounding, relative
FRESH = {"t": 0, "decay": 0.0, "comp": 1.0}


# ------------------------------------------------------------------------------------------------ flags
@pytest.mark.parametrize("stage", STAGES)
def test_flags_are_declared_on_every_trainer_parser_with_their_defaults(stage, capsys):
    F = drivers._parser(stage, True).parse_known_args(["-t"])[0]
    assert (F.ema_decay, F.ema_warmup, F.ema_eval) == (0.0, False, "ema")
    assert drivers._ema(F) == {"ema": None} and capsys.readouterr().out == ""      # the defaults: no average, nothing said
    F = drivers._parser(stage, True).parse_known_args(["-t", "--ema_decay", "0.999", "--ema_warmup", "--ema_eval", "both"])[0]
    assert drivers._ema(F) == {"ema": Ema(0.999, True)} and F.ema_eval == "both"
    assert capsys.readouterr().out == "weight average: decay 0.999 warmup\n"       # exactly one line
    F = drivers._parser(stage, True).parse_known_args(["-t", "--ema_decay", "0.9"])[0]
    assert drivers._ema(F) == {"ema": Ema(0.9, False)}
    assert capsys.readouterr().out == "weight average: decay 0.9\n"
    with pytest.raises(SystemExit):
        drivers._parser(stage, True).parse_known_args(["-t", "--ema_eval", "raw"])
    text = drivers._parser(stage, False).format_help()                             # trainer flags only
    assert "--ema_decay" not in text and "--ema_warmup" not in text and "--ema_eval" not in text
    assert "--ema_decay" not in drivers._predict_parser().format_help()


BAD = [(["--ema_decay", "1.0"], "--ema_decay"), (["--ema_decay", "-0.1"], "--ema_decay"), (["--ema_decay", "nan"], "--ema_decay"),
       (["--ema_decay", "1.5", "--ema_warmup"], "--ema_decay"), (["--ema_warmup"], "--ema_warmup"), (["--ema_eval", "both"], "--ema_eval")]


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


def test_ema_tuple_checks_and_config():
    assert not Ema().active and Ema(0.5).active and Ema(0.5, True).active
    assert Ema(0.999, True).config() == {"decay": 0.999, "warmup": True} and Ema().config() == {"decay": 0.0, "warmup": False}
    assert Ema(0.0).check() == Ema() and Ema(0.25, True).check() == Ema(0.25, True)
    for bad in (Ema(1.0), Ema(-0.5), Ema(float("nan")), Ema(0.0, True), Ema(2.0, True)):
        with pytest.raises(ValueError):
            bad.check()


# ------------------------------------------------------------------------------------------------ the record
def test_advance_host_follows_the_tensorflow_schedule_and_crosses_over():
    """30 steps with warmup at D = 0.999, every step against min(D, (1 + t) / (10 + t)) in Python doubles.  At 0.999 the ramp crosses the decay only
    at t = 8990, so the crossover step cannot lie inside 30 steps; the same 30 steps at D = 0.7 (crossed at t = 20: 21 / 30) put it there."""
    D, rec, ds = 0.999, dict(FRESH), []
    for step in range(1, 31):
        rec = ops.ema_advance_host(rec, D, warmup=True)
        d = min(D, (1 + step) / (10 + step))                       # Python doubles
        assert rec == {"t": step, "decay": float(np.float32(d)), "comp": float(np.float32(1.0 - d))}, step
        ds.append(d)
    assert ds[0] == 2 / 11 and ds[0] < D                           # the ramp ...
    assert all(a < b for a, b in zip(ds, ds[1:]))                  # ... (30 steps are too few for 0.999: (1 + t) / (10 + t) reaches it at t = 8990)
    # a decay the ramp does reach inside the sequence: the crossover step is present, both sides of it are
    D, rec, ds = 0.7, dict(FRESH), []
    for step in range(1, 31):
        rec = ops.ema_advance_host(rec, D, warmup=True)
        d = min(D, (1 + step) / (10 + step))
        assert rec["decay"] == float(np.float32(d)) and rec["comp"] == float(np.float32(1.0 - d)) and rec["t"] == step
        ds.append(d)
    first = next(i for i, d in enumerate(ds) if d == D)            # t = 20: 21 / 30 = 0.7
    assert 0 < first < 29 and all(d < D for d in ds[:first]) and all(d == D for d in ds[first:])
    assert (1 + first) / (10 + first) < D <= (2 + first) / (11 + first)


def test_advance_host_skip_and_constant_decay():
    rec = {"t": 3, "decay": 0.5, "comp": 0.5}
    assert ops.ema_advance_host(rec, 0.9, True, skip=True) == rec and ops.ema_advance_host(rec, 0.9, True, skip=True) is not rec
    r, seen = dict(FRESH), []
    for step in range(1, 6):
        r = ops.ema_advance_host(r, 0.999)
        seen.append((r["decay"], r["comp"]))
        assert r["t"] == step
    assert set(seen) == {(float(np.float32(0.999)), float(np.float32(1.0 - 0.999)))}     # constant from t = 1
    # comp is the ROUNDED DOUBLE difference, not 1 - float32(decay)
    assert float(np.float32(1.0 - 0.999)) != float(np.float32(1.0) - np.float32(0.999))


# ------------------------------------------------------------------------------------------------ the step against float64
@pytest.mark.parametrize("decay,warmup", [(0.999, False), (0.9, False), (0.999, True)], ids=["0.999", "0.9", "0.999-warmup"])
def test_step_host_against_float64(decay, warmup):
    """e' = fl(fl(d32 e) + fl(c32 p)) against d e + (1 - d) p in float64, d the step's double decay: the two rounded scalars and the three roundings
    give |e' - (d e + (1 - d) p)| <= 3 x 2^-24 x (|d e| + |c p|) x (1 + 2^-20) (second-order terms are 2^-24 of the first).  A product of a float32
    scalar and a POWER OF TWO is exact, so step 0 on the ramp rounds only in the sum; from step 1 on e is a general float32 and all three round."""
    f32 = np.float32
    e, _ = _ramps(0)
    rec, differs = dict(FRESH), 0
    for step in range(5):
        p = _ramps(step)[1]
        rec = ops.ema_advance_host(rec, decay, warmup)
        d = min(decay, (1.0 + rec["t"]) / (10.0 + rec["t"])) if warmup else decay
        got = ops.ema_step_host(e, p, rec).numpy()
        de, cp = f32(rec["decay"]) * e, f32(rec["comp"]) * p
        _all_zero_or_normal({"de": de, "cp": cp, "e": got})
        assert np.array_equal(got, de + cp) and got.dtype == np.float32
        e64, p64 = e.astype(np.float64), p.astype(np.float64)
        want = d * e64 + (1.0 - d) * p64
        bound = 3 * U * (np.abs(d * e64) + np.abs(rec["comp"] * p64)) * (1 + 2.0 ** -20)
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= bound), (step, float((err / bound).max()))
        # a deliberately WRONG order -- the first product fused into the add (one rounding for d e + cp), emulated in float64 (the product of two
        # float32 values is exact there) -- must not give the restatement's bits everywhere
        fused = (f32(rec["decay"]).astype(np.float64) * e64 + cp.astype(np.float64)).astype(f32)
        differs += int(np.count_nonzero(fused != got))
        e = got
    assert differs > 0
    # signs: all four pairs occurred
    e0, p0 = _ramps(0)
    assert {(a, b) for a, b in zip(np.sign(e0), np.sign(p0))} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}


def test_step_host_skip_and_data_nan():
    e, p = _ramps(0)
    rec = ops.ema_advance_host(dict(FRESH), 0.9)
    out = ops.ema_step_host(e, p, rec, skip=True)
    assert np.array_equal(out.numpy(), e) and out.dtype == torch.float32
    p = p.copy()
    p[7] = np.nan
    out = ops.ema_step_host(torch.from_numpy(e), torch.from_numpy(p), rec).numpy()
    assert np.isnan(out[7]) and np.count_nonzero(np.isnan(out)) == 1
    z = np.zeros(8, dtype=np.float32)
    assert np.array_equal(ops.ema_step_host(z, z, rec).numpy().view(np.int32), z.view(np.int32))     # padding: d 0 + c 0 = +0


# ------------------------------------------------------------------------------------------------ the entry points refuse before any launch
def test_abi_refusals_without_a_device():
    lib = _lib.lib
    EINVAL, EALIGN = -1, -2
    E, P, S, G = 0x10000, 0x20000, 0x30000, 0x40000                # never dereferenced: every call below returns before a launch
    assert lib.mt4_ema_step_f32(None, P, 8, S, None, None) == EINVAL
    assert lib.mt4_ema_step_f32(E, None, 8, S, None, None) == EINVAL
    assert lib.mt4_ema_step_f32(E, P, 8, None, None, None) == EINVAL
    assert lib.mt4_ema_step_f32(E, P, 0, S, None, None) == EINVAL
    assert lib.mt4_ema_step_f32(E, P, -4, S, G, None) == EINVAL
    assert lib.mt4_ema_step_f32(E + 4, P, 8, S, None, None) == EALIGN
    assert lib.mt4_ema_step_f32(E, P + 8, 8, S, None, None) == EALIGN
    assert lib.mt4_ema_step_f32(E, P, 8, S + 4, None, None) == EALIGN
    assert lib.mt4_ema_step_f32(E, P, 8, S, G + 4, None) == EALIGN
    assert lib.mt4_ema_advance(None, 0.9, 0, None, None) == EINVAL
    for bad in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        assert lib.mt4_ema_advance(S, bad, 1, None, None) == EINVAL, bad
    assert lib.mt4_ema_advance(S + 4, 0.9, 0, None, None) == EALIGN
    assert ops.EMA_STATE_BYTES == 16
    with pytest.raises(_lib.Mt4Error):
        ops.ema_step(torch.zeros(4), torch.zeros(4), torch.zeros(2, dtype=torch.float64))             # CPU tensors are refused


# ------------------------------------------------------------------------------------------------ run_epochs
SCHEDULE = ["-w", "1", "2", "3", "-l", "0.1", "0.2", "0.05", "--power", "0.2", "--decay_rate", "0.9"]
CFG = Ema(0.9, True).config()


class FakeTrainer:
    """weights = the last epoch and a running sum; with `cfg` it also keeps an average of the sum, advanced once per epoch with the host
    restatements, so a resumed run ends with the same average bytes only if the average came back"""

    def __init__(self, cfg=None):
        self.lr, self.epoch, self.acc, self.cfg = None, -1, 0.0, cfg
        self.avg, self.rec = None, dict(FRESH)

    def state_dict(self):
        return {"epoch": torch.tensor(self.epoch), "acc": torch.tensor(self.acc, dtype=torch.float64)}

    def load_state_dict(self, sd):
        self.epoch, self.acc = int(sd["epoch"]), float(sd["acc"])
        if self.cfg is not None:
            self.avg = self.acc                                     # a copy of the loaded weights
        return self

    def step(self, epoch, acc):
        self.epoch, self.acc = epoch, acc
        if self.cfg is not None:
            self.rec = ops.ema_advance_host(self.rec, self.cfg["decay"], self.cfg["warmup"])
            self.avg = self.rec["decay"] * (self.acc if self.avg is None else self.avg) + self.rec["comp"] * self.acc

    def ema_config(self):
        return self.cfg

    def ema_record(self):
        return dict(self.rec) if self.cfg is not None else {}

    def ema_state_dict(self):
        return {"epoch": torch.tensor(self.epoch), "acc": torch.tensor(self.avg, dtype=torch.float64)}

    def ema_export(self):
        return {"ema": self.cfg, "t": self.rec["t"], "state": self.ema_state_dict()}

    def load_ema_export(self, exp):
        if exp["ema"] != self.cfg:
            raise ValueError("another config")
        self.avg = float(exp["state"]["acc"])
        self.rec = dict(FRESH)
        for _ in range(exp["t"]):
            self.rec = ops.ema_advance_host(self.rec, self.cfg["decay"], self.cfg["warmup"])


def _flags(*argv, resume=True, ema_eval=None):
    p = argparse.ArgumentParser()
    add_schedule_flags(p)
    F = p.parse_args(list(argv) + SCHEDULE)
    F.resume = resume
    if ema_eval is not None:
        F.ema_eval = ema_eval
    return F


class Run:
    def __init__(self, tmp_path, F, cfg=None, die_in=None, load=True, hook=None):
        d = tmp_path / "run"
        self.dir, self.latest, self.best, self.log = d, str(d / "m_latest.pth"), str(d / "m.pth"), d / "m.log"
        tr = self.tr = FakeTrainer(cfg)
        py = random.Random(5)
        resume = trainloop.load_resume(self.latest, 0, 1, ema=cfg) if F.resume else None
        state = drivers._latest_state(self.latest, resume)
        if state is not None:
            tr.load_state_dict(state)
        if load:
            drivers._load_optim(tr, resume)                         # (the driver's one loader of what lies beside the checkpoint)
        self.validated = []

        def train_epoch(epoch):
            if epoch == die_in:
                raise KeyboardInterrupt
            tr.step(epoch, tr.acc + py.random() * tr.lr)
            return tr.acc, 1

        def validate(state):
            self.validated.append({k: v.clone() for k, v in state.items()})
            if hook:
                hook(self)
            return float(state["acc"]), f"ivt: [{float(state['acc']):.5f}]"

        self.result = run_epochs(F, tr, 0, train_epoch, validate, str(self.log), self.latest, self.best,
                                 latest_every_epoch=True, generators={"py": py}, resume=resume, world=1)

    def files(self):
        return sorted(os.listdir(self.dir))

    def sidecar(self):
        with open(trainloop.resume_file(self.latest)) as f:
            return json.load(f)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_validate_scores_the_average_and_the_best_checkpoint_holds_it(tmp_path):
    r = Run(tmp_path, _flags("--epochs", "3", resume=False), CFG)
    assert len(r.validated) == 3
    assert float(r.validated[-1]["acc"]) == r.tr.avg != r.tr.acc                                     # validate received the EMA dict
    best, latest = torch.load(r.best), torch.load(r.latest)
    assert float(best["acc"]) == r.tr.avg and float(latest["acc"]) == r.tr.acc                       # best: the average; `_latest`: the raw weights
    assert list(best) == list(latest) and r.result["val_mAP"] == r.tr.avg
    assert r.files() == ["m.log", "m.pth", "m_latest.pth"]                                           # no --resume: no file beside them
    lines = [ln for ln in r.log.read_text().splitlines() if ln.startswith("Traning | lr:")]
    assert len(lines) == 3
    rec = dict(FRESH)
    for i, ln in enumerate(lines):
        rec = ops.ema_advance_host(rec, 0.9, True)
        assert ln.endswith(f" | ema t {i + 1} decay {rec['decay']:.6g}"), ln
    assert "raw =>" not in r.log.read_text()


def test_ema_eval_both_validates_twice_and_logs_the_raw_score(tmp_path):
    r = Run(tmp_path, _flags("--epochs", "2", resume=False, ema_eval="both"), CFG)
    assert len(r.validated) == 4
    assert [float(v["acc"]) for v in r.validated[2:]] == [r.tr.avg, r.tr.acc]                        # the average first (it decides), then the raw weights
    vw = [ln for ln in r.log.read_text().splitlines() if "video-wise |" in ln]
    assert len(vw) == 2 and vw[-1].endswith(f"mAP => ivt: [{r.tr.avg:.5f}] | raw => ivt: [{r.tr.acc:.5f}] "), vw
    assert float(torch.load(r.best)["acc"]) == r.tr.avg and r.result["val_mAP"] == r.tr.avg          # the raw score decides nothing
    # the flag without an average on the trainer changes nothing
    plain = Run(tmp_path / "p", _flags("--epochs", "2", resume=False, ema_eval="both"), None)
    assert len(plain.validated) == 2 and "raw =>" not in plain.log.read_text() and " ema t " not in plain.log.read_text()


def test_ema_file_is_written_before_the_sidecar_named_digested_and_two_generations_are_kept(tmp_path):
    seen = []

    def hook(run):                                                  # during epoch e's validation: the files of epoch e - 1 and no sidecar of e yet
        seen.append((sorted(f for f in os.listdir(run.dir) if ".ema." in f),
                     [x["epoch"] for x in run.sidecar()["records"]] if os.path.exists(trainloop.resume_file(run.latest)) else []))
    r = Run(tmp_path, _flags("--epochs", "1"), CFG, hook=hook)
    assert seen == [([], [])]                                       # nothing beside the checkpoint until the epoch's pair is written
    assert r.files() == ["m.log", "m.pth", "m_latest.pth", "m_latest.pth.ema.e0", "m_latest.pth.resume"]
    rec = r.sidecar()["records"][0]
    path = trainloop.ema_file(r.latest, 0)
    assert rec["ema"] == {"file": "m_latest.pth.ema.e0", "digest": trainloop._file_digest(path), "config": CFG}
    exp = torch.load(path)
    assert exp["ema"] == CFG and exp["t"] == 1 and float(exp["state"]["acc"]) == r.tr.avg == float(torch.load(r.best)["acc"])
    r = Run(tmp_path, _flags("--epochs", "2"), CFG)
    assert [x["ema"]["file"] for x in r.sidecar()["records"]] == ["m_latest.pth.ema.e1", "m_latest.pth.ema.e0"]
    r = Run(tmp_path, _flags("--epochs", "4"), CFG)                  # ... and every older one is removed behind the pair
    assert [f for f in r.files() if ".ema." in f] == ["m_latest.pth.ema.e2", "m_latest.pth.ema.e3"]
    for x in r.sidecar()["records"]:
        assert trainloop._file_digest(os.path.join(r.dir, x["ema"]["file"])) == x["ema"]["digest"]
    assert not [f for f in r.files() if f.endswith(".tmp")]
    # order of the writes: the sidecar never names a file that is not there
    order = []
    real_json, real_named = trainloop._write_json_atomic, trainloop._save_named
    try:
        trainloop._save_named = lambda obj, path: (order.append(("ema", os.path.basename(path))), real_named(obj, path))[1]
        trainloop._write_json_atomic = lambda obj, path: (order.append(("side", os.path.exists(os.path.join(os.path.dirname(path), obj["records"][0]["ema"]["file"])))),
                                                          real_json(obj, path))[1]
        Run(tmp_path / "o", _flags("--epochs", "2"), CFG)
    finally:
        trainloop._write_json_atomic, trainloop._save_named = real_json, real_named
    assert order == [("ema", "m_latest.pth.ema.e0"), ("side", True), ("ema", "m_latest.pth.ema.e1"), ("side", True)]


def test_two_plus_two_epochs_end_like_four_and_a_kill_between_the_writes_keeps_a_consistent_pair(tmp_path):
    straight = Run(tmp_path / "a", _flags("--epochs", "4"), CFG)
    Run(tmp_path / "b", _flags("--epochs", "2"), CFG)
    with pytest.raises(KeyboardInterrupt):
        Run(tmp_path / "b", _flags("--epochs", "4"), CFG, die_in=3)
    # a kill between the EMA file of epoch 3 and the sidecar that would name it: the sidecar on disk still names files that exist
    real = trainloop._write_json_atomic

    def dying(obj, path):
        raise KeyboardInterrupt
    trainloop._write_json_atomic = dying
    try:
        with pytest.raises(KeyboardInterrupt):
            Run(tmp_path / "b", _flags("--epochs", "4"), CFG)
    finally:
        trainloop._write_json_atomic = real
    d = tmp_path / "b" / "run"
    side = json.load(open(d / "m_latest.pth.resume"))
    assert [x["epoch"] for x in side["records"]] == [2, 1] and all(os.path.exists(d / x["ema"]["file"]) for x in side["records"])
    assert os.path.exists(d / "m_latest.pth.ema.e3") and not [f for f in os.listdir(d) if f.endswith(".tmp")]    # the orphan is replaced by the next run
    assert trainloop.load_resume(str(d / "m_latest.pth"), 0, 1, ema=CFG).epoch == 2
    resumed = Run(tmp_path / "b", _flags("--epochs", "4"), CFG)
    assert _bytes(resumed.latest) == _bytes(straight.latest) and _bytes(resumed.best) == _bytes(straight.best)
    assert _bytes(trainloop.ema_file(resumed.latest, 3)) == _bytes(trainloop.ema_file(straight.latest, 3))
    assert resumed.tr.avg == straight.tr.avg and resumed.tr.rec == straight.tr.rec and resumed.tr.rec["t"] == 4
    # without the persisted average it restarts from the weights and ends elsewhere: what the file is for
    Run(tmp_path / "c", _flags("--epochs", "2"), CFG)
    lost = Run(tmp_path / "c", _flags("--epochs", "4"), CFG, load=False)
    assert _bytes(lost.latest) == _bytes(straight.latest) and lost.tr.avg != straight.tr.avg


def test_resume_refusals_name_the_file_and_the_way_out(tmp_path):
    r = Run(tmp_path, _flags("--epochs", "2"), CFG)
    path = trainloop.ema_file(r.latest, 1)
    # a record with an average resumed without the flag, or with another config
    with pytest.raises(ValueError, match=r"ema\.e1.*no --ema_decay.*drop --resume"):
        trainloop.load_resume(r.latest, 0, 1)
    with pytest.raises(ValueError, match=r"ema\.e1.*changing the average.*drop --resume"):
        trainloop.load_resume(r.latest, 0, 1, ema=Ema(0.9, False).config())
    with pytest.raises(ValueError, match="changing the average"):
        trainloop.load_resume(r.latest, 0, 1, ema=Ema(0.99, True).config())
    got = trainloop.load_resume(r.latest, 0, 1, ema=CFG)
    assert got.ema_state()["t"] == 2 and got.optim_state is None
    # its bytes have another digest
    data = _bytes(path)
    with open(path, "wb") as f:
        f.write(data[:-1] + bytes([data[-1] ^ 1]))
    with pytest.raises(ValueError, match=r"ema\.e1.*replaced or its write was torn.*drop --resume"):
        trainloop.load_resume(r.latest, 0, 1, ema=CFG)
    # it is missing
    os.remove(path)
    with pytest.raises(ValueError, match=r"ema\.e1.*is missing.*drop --resume"):
        trainloop.load_resume(r.latest, 0, 1, ema=CFG)
    # the flag on a record without "ema"
    plain = Run(tmp_path / "plain", _flags("--epochs", "1"), None)
    with pytest.raises(ValueError, match=r"m_latest\.pth\.resume.*holds no weight average.*Drop --ema_decay"):
        trainloop.load_resume(plain.latest, 0, 1, ema=CFG)
    assert trainloop.load_resume(plain.latest, 0, 1).ema_state is None


def test_runs_without_an_average_write_what_they_wrote(tmp_path):
    """a trainer whose average is off (None) and one that has never heard of it write byte-identical sidecars, checkpoints and log lines in
    today's format: records of exactly epoch, top, digest, generators"""
    class Old:                                                      # the fake trainer of tests/test_resume_cpu.py: no average methods at all
        def __init__(self):
            self.lr, self.epoch, self.acc = None, -1, 0.0
        state_dict = FakeTrainer.state_dict

    def run(d, tr):
        py = random.Random(5)

        def train_epoch(epoch):
            tr.epoch, tr.acc = epoch, tr.acc + py.random() * tr.lr
            return tr.acc, 1
        run_epochs(_flags("--epochs", "3"), tr, 0, train_epoch, lambda s: (0.5, "ivt: [0.50000]"), str(d / "m.log"), str(d / "m_latest.pth"),
                   str(d / "m.pth"), latest_every_epoch=True, generators={"py": py}, world=1)
        strip = lambda ln: ln.split(" secs")[0].rsplit(" | ", 1)[0] + ln.split(" secs", 1)[1] if " secs" in ln else ln.split(", time ")[0]
        return (_bytes(str(d / "m_latest.pth.resume")), _bytes(str(d / "m_latest.pth")), _bytes(str(d / "m.pth")),
                [strip(ln).replace(str(d), "") for ln in open(d / "m.log").read().splitlines()]), sorted(os.listdir(d))
    a, files_a = run(tmp_path / "a", Old())
    b, files_b = run(tmp_path / "b", FakeTrainer(None))
    assert a == b and files_a == files_b == ["m.log", "m.pth", "m_latest.pth", "m_latest.pth.resume"]
    obj = json.loads(a[0])
    assert sorted(obj) == ["format", "records", "world"] and obj["format"] == 1
    assert all(sorted(r) == ["digest", "epoch", "generators", "top"] for r in obj["records"]) and len(obj["records"]) == 2
    assert all(" ema t " not in ln and "raw =>" not in ln for ln in a[3])
    assert math.isfinite(float(torch.load(tmp_path / "a" / "m_latest.pth")["acc"]))
