"""The epoch and checkpoint loop the four training drivers share (`Spatial_cnn`, `Spatial_transformer`, `Temporal_tenco`, `Temporal_mstct`
`run.py -t`): the schedule flags, `lr_at_epoch`, the round-robin dealing of batches to ranks, the `Traning | lr:` line, one `weight_mgt`, and
the resume state of --resume (`load_resume`, `resume_file`).  Host code only: it imports without the HIP library."""
from __future__ import annotations

import argparse
import hashlib
import io
import json
import math
import os
import time
from typing import Callable, Dict, List, Tuple

import torch


def _dist():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _barrier():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()


def _log(path: str, msg: str):
    print(msg)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a+") as f:
        print(msg, file=f)


def add_schedule_flags(p: argparse.ArgumentParser):
    """the schedule flags every driver declares (`Temporal_tenco/run.py`, `Spatial_cnn/run.py`, ...)"""
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("-w", "--warmups", type=int, nargs="+", default=[9, 18, 58])
    p.add_argument("-l", "--initial_learning_rates", type=float, nargs="+", default=[0.01, 0.01, 0.01])
    p.add_argument("--weight_decay", type=float, default=1e-5)
    p.add_argument("--decay_rate", type=float, default=0.99)
    p.add_argument("--power", type=float, default=0.1)
    p.add_argument("--val_interval", type=int, default=1)


def lr_at_epoch(epoch: int, lr: float, power: float, warmup: int, decay_rate: float) -> float:
    """The schedule of `Temporal_tenco/run.py:341-348` (same in Spatial_cnn): SGD(lr/power) under
    SequentialLR([LinearLR(start_factor=power, total_iters=warmup), ExponentialLR(gamma)], milestones=[warmup+1]);
    the value torch's schedulers hold during epoch `epoch` (0-based)."""
    base = lr / power
    if epoch <= warmup:
        return base * (power + (1.0 - power) * min(epoch, warmup) / warmup)
    return base * decay_rate ** (epoch - warmup - 1)


def deal(order: list, batch: int, world: int, rank: int) -> List[list]:
    """the batches rank `rank` takes of an epoch's `order` cut into `nb` batches of `batch` (drop_last False): batch (s * world + rank) % nb
    in step s of ceil(nb / world), so every rank runs the same number of steps (the last step wraps around to the first batches)"""
    nb = (len(order) + batch - 1) // batch
    return [order[bi * batch:(bi + 1) * batch] for bi in ((s * world + rank) % nb for s in range((nb + world - 1) // world))]


def guard_flags(F) -> Tuple[float, bool]:
    """(--clip_grad_norm, --skip_nonfinite) of a trainer's flags; (0.0, False) where they are not declared"""
    return float(getattr(F, "clip_grad_norm", 0.0) or 0.0), bool(getattr(F, "skip_nonfinite", False))


class LossMean:
    """the loss an epoch logs: `add(loss)` per step -> `total` / `steps`.  finite_only (--skip_nonfinite): a step whose loss is NaN or Inf is
    left out of both, so the epoch's loss is the mean over the steps with a finite loss; otherwise the plain running sum over every step"""

    def __init__(self, finite_only: bool = False):
        self.finite_only, self.total, self.steps = bool(finite_only), 0.0, 0

    def add(self, loss: float):
        if self.finite_only and not math.isfinite(loss):
            return
        self.total += loss
        self.steps += 1


def save_atomic(state: Dict[str, torch.Tensor], path: str):
    """torch.save through a temporary file and os.replace: a run killed during the write leaves the previous file intact"""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = path + ".tmp"
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


# ------------------------------------------------------------------------------------------------ --resume
# The resume state of a run lives beside its newest checkpoint `<latest>` (which stays the plain state dict it always was):
#   <latest>.resume          rank 0: {"format", "world", "records": [newest, the one before]}, a record = {"epoch": the last completed epoch,
#                            "top": the best score so far, "digest": "sha256:<hex of the <latest> bytes it belongs to>", "generators": {name: state}}
#   <latest>.resume.rank<r>  rank r > 0: {"format", "world", "rank", "records": [...]}, a record = {"epoch", "generators"} -- that rank's own draws
# JSON, readable with any editor.  TWO records are kept because the pair cannot be replaced in one step: the sidecar is replaced first, then
# `<latest>`; a run killed in between leaves the new sidecar beside the old `<latest>`, whose digest the older record still names.
# A trainer with optimizer state (--momentum, --optimizer adamw) adds
#   <latest>.optim.e<epoch>  rank 0: torch.save of `tr.optimizer_state_dict()` behind that epoch, written BEFORE the sidecar whose record names it:
#                            "optim": {"file": its base name, "digest": "sha256:<hex of its bytes>", "config": the rule's config}
# Both records' files are kept; older ones are removed once the pair is written, so a kill at any point leaves every named file in place.  Every
# rank reads the file on resume (the state is the same on every rank).  Without optimizer state nothing of this is written.
# A trainer with a weight average (--ema_decay) adds, with exactly that life cycle,
#   <latest>.ema.e<epoch>    rank 0: torch.save of `tr.ema_export()` behind that epoch, named in the record as
#                            "ema": {"file": its base name, "digest": "sha256:<hex of its bytes>", "config": the average's config}
# Without the average nothing of this is written.
RESUME_SUFFIX = ".resume"
OPTIM_SUFFIX = ".optim.e"
EMA_SUFFIX = ".ema.e"
_RESUME_FORMAT = 1


def resume_file(latest: str, rank: int = 0) -> str:
    """the file rank `rank` keeps its resume state in, beside the checkpoint `latest`"""
    return latest + RESUME_SUFFIX + (f".rank{rank}" if rank else "")


def _digest(data) -> str:
    return "sha256:" + hashlib.sha256(data).hexdigest()


def _file_digest(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return "sha256:" + h.hexdigest()


def _generator_state(g):
    """a host generator's state as JSON: `random.Random`-like objects (getstate / setstate), `torch.Generator`-like ones (get_state / set_state)"""
    if hasattr(g, "getstate"):
        version, words, gauss = g.getstate()
        return {"py": [version, list(words), gauss]}
    if hasattr(g, "get_state"):
        return {"torch": bytes(g.get_state().tolist()).hex()}
    raise TypeError(f"a generator handed to run_epochs needs getstate/setstate or get_state/set_state: {type(g).__name__}")


def _set_generator_state(g, s):
    if "py" in s:
        version, words, gauss = s["py"]
        g.setstate((version, tuple(words), gauss))
    else:
        g.set_state(torch.tensor(list(bytes.fromhex(s["torch"])), dtype=torch.uint8))


def _write_json_atomic(obj, path: str):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = path + ".tmp"
    try:
        with open(tmp, "w") as f:
            json.dump(obj, f)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _read_json(path: str) -> dict:
    try:
        with open(path) as f:
            obj = json.load(f)
        if obj.get("format") != _RESUME_FORMAT or not isinstance(obj.get("records"), list):
            raise ValueError("not a resume state of this format")
        return obj
    except (OSError, ValueError, AttributeError) as e:
        raise ValueError(f"--resume: {path} cannot be read as resume state ({e}); move it and the checkpoint beside it away to start a fresh run, "
                         "or drop --resume to start again at epoch 0 from the checkpoint's weights") from None


class Resume:
    """what `load_resume` found: `epoch` = the last completed epoch (-1: a fresh run), `top`, this rank's generator states by name, and
    `state_dict()` = the tensors of exactly the `<latest>` bytes the digest was checked on (None for a fresh run)"""

    def __init__(self, epoch: int = -1, top: float = 0.0, generators: dict = None, data: bytes = None, record: dict = None,
                 optim_data: bytes = None, ema_data: bytes = None):
        self.epoch, self.top, self.generators, self._data, self.record = epoch, top, generators or {}, data, record
        # `ema_state()` = the `ema_export()` of exactly the bytes the record's digest was checked on; None where the record names none
        self.ema_state = None if ema_data is None else (lambda: torch.load(io.BytesIO(ema_data), map_location="cpu"))
        # `optim_state()` = the optimizer state of exactly the bytes the record's digest was checked on; None where the record names none
        self.optim_state = None if optim_data is None else (lambda: torch.load(io.BytesIO(optim_data), map_location="cpu"))

    def state_dict(self):
        return None if self._data is None else torch.load(io.BytesIO(self._data), map_location="cpu")


def optim_file(latest: str, epoch: int) -> str:
    """the file the optimizer state behind `epoch` is kept in, beside the checkpoint `latest`"""
    return latest + OPTIM_SUFFIX + str(epoch)


def _load_optim_bytes(latest: str, side: str, rec: dict, optim) -> bytes:
    """the optimizer file a record names, checked against the record and against this run's flags (`optim` = their config, None: plain SGD)"""
    named = rec.get("optim")
    if named is None:
        if optim is not None:
            raise ValueError(f"--resume: {side} (epoch {rec.get('epoch')}) holds no optimizer state and this run asks for {optim}: the run that wrote "
                             "it used plain SGD.  Drop --momentum / --optimizer to continue it as it was, or drop --resume to start again at epoch "
                             "0 from the weights with the new update rule")
        return None
    path = os.path.join(os.path.dirname(latest), named["file"])
    if optim is None:
        raise ValueError(f"--resume: {side} (epoch {rec.get('epoch')}) was written with optimizer state ({named['config']}, {path}) and this run has no "
                         "optimizer flags: give the flags of the run that wrote it, or drop --resume to start again at epoch 0 from the weights")
    if named["config"] != optim:
        raise ValueError(f"--resume: the optimizer state {path} belongs to {named['config']} and this run asks for {optim}; changing the update rule "
                         "across a resume is not supported.  Give the recorded flags, or drop --resume to start again at epoch 0 from the weights")
    if not os.path.exists(path):
        raise ValueError(f"--resume: the optimizer state {path} that {side} names is missing.  Put it back, or drop --resume to start again at epoch 0 "
                         "from the weights (momentum and moments start at zero)")
    with open(path, "rb") as f:
        data = f.read()
    if _digest(data) != named["digest"]:
        raise ValueError(f"--resume: {path} ({_digest(data)[:19]}...) is not the optimizer state {side} was written for ({named['digest'][:19]}...): it "
                         "was replaced or its write was torn.  Put the matching file back, or drop --resume to start again at epoch 0 from the weights")
    return data


def ema_file(latest: str, epoch: int) -> str:
    """the file the weight average behind `epoch` is kept in, beside the checkpoint `latest`"""
    return latest + EMA_SUFFIX + str(epoch)


def _load_ema_bytes(latest: str, side: str, rec: dict, ema) -> bytes:
    """the weight-average file a record names, checked against the record and against this run's flags (`ema` = their config, None: no average)"""
    named = rec.get("ema")
    if named is None:
        if ema is not None:
            raise ValueError(f"--resume: {side} (epoch {rec.get('epoch')}) holds no weight average and this run asks for {ema}: the run that wrote it "
                             "kept none.  Drop --ema_decay / --ema_warmup to continue it as it was, or drop --resume to start again at epoch 0 "
                             "from the weights with a fresh average")
        return None
    path = os.path.join(os.path.dirname(latest), named["file"])
    if ema is None:
        raise ValueError(f"--resume: {side} (epoch {rec.get('epoch')}) was written with a weight average ({named['config']}, {path}) and this run has "
                         "no --ema_decay: give the flags of the run that wrote it, or drop --resume to start again at epoch 0 from the weights")
    if named["config"] != ema:
        raise ValueError(f"--resume: the weight average {path} belongs to {named['config']} and this run asks for {ema}; changing the average "
                         "across a resume is not supported.  Give the recorded flags, or drop --resume to start again at epoch 0 from the weights")
    if not os.path.exists(path):
        raise ValueError(f"--resume: the weight average {path} that {side} names is missing.  Put it back, or drop --resume to start again at epoch 0 "
                         "from the weights (the average starts from them)")
    with open(path, "rb") as f:
        data = f.read()
    if _digest(data) != named["digest"]:
        raise ValueError(f"--resume: {path} ({_digest(data)[:19]}...) is not the weight average {side} was written for ({named['digest'][:19]}...): it "
                         "was replaced or its write was torn.  Put the matching file back, or drop --resume to start again at epoch 0 from the weights")
    return data


def load_resume(latest: str, rank: int = 0, world: int = 1, optim: dict = None, ema: dict = None) -> Resume:
    """--resume at the start of a run, before any model is built and without touching a file: a fresh `Resume` when there is no `latest`, the
    state to continue from when its sidecar names the bytes of `latest`, ValueError otherwise (no sidecar: the checkpoint was written without
    --resume; another `world`; no record with the digest of `latest`; rank > 0: no record of that epoch in its own file).  optim: the config of
    this run's update rule (`flatparams.Optim.config()`), None for plain SGD: the record's optimizer file must be there with the recorded
    digest and config, a record without one takes no optimizer flags and one with it needs them (ValueError otherwise).  ema: the config of
    this run's weight average (`flatparams.Ema.config()`), None without one: the same rules for the record's weight-average file"""
    if not os.path.exists(latest):
        return Resume()                                            # (a sidecar alone: the run died before its first checkpoint; it is overwritten)
    side = resume_file(latest)
    if not os.path.exists(side):
        raise ValueError(f"--resume: {latest} has no resume state beside it ({side} is missing): it was written by a run without --resume.  "
                         "Drop --resume to start again at epoch 0 from its weights, or move the checkpoint away to start a fresh run")
    obj = _read_json(side)
    if obj.get("world") != world:
        raise ValueError(f"--resume: {side} was written by a run of {obj.get('world')} rank(s) and this one has {world}; the ranks' draws do not "
                         "carry over.  Start it with the same number of ranks, or drop --resume to start again at epoch 0 from the weights")
    with open(latest, "rb") as f:
        data = f.read()
    digest = _digest(data)
    rec = next((r for r in obj["records"] if r.get("digest") == digest), None)
    if rec is None:
        raise ValueError(f"--resume: {latest} ({digest[:19]}...) is not the checkpoint {side} was written for (epochs "
                         f"{[r.get('epoch') for r in obj['records']]}): it was replaced or its write was torn.  Put the matching file back, or move "
                         "both away to start a fresh run, or drop --resume to start again at epoch 0 from these weights")
    optim_data = _load_optim_bytes(latest, side, rec, optim)
    ema_data = _load_ema_bytes(latest, side, rec, ema)
    gens = rec["generators"]
    if rank:
        mine = resume_file(latest, rank)
        if not os.path.exists(mine):
            raise ValueError(f"--resume: rank {rank} has no resume state ({mine} is missing) for {latest}; restore it or start a fresh run")
        own = _read_json(mine)
        own_rec = next((r for r in own["records"] if r.get("epoch") == rec["epoch"]), None)
        if own.get("world") != world or own_rec is None:
            raise ValueError(f"--resume: {mine} (world {own.get('world')}, epochs {[r.get('epoch') for r in own['records']]}) does not belong to "
                             f"epoch {rec['epoch']} of {side} (world {world}); restore the matching file or start a fresh run")
        gens = own_rec["generators"]
    return Resume(int(rec["epoch"]), float(rec["top"]), gens, data, rec, optim_data, ema_data)


def _save_named(obj, path: str) -> str:
    """torch.save through a temporary file and os.replace; -> the digest of the bytes"""
    tmp = path + ".tmp"
    try:
        torch.save(obj, tmp)
        digest = _file_digest(tmp)
        os.replace(tmp, path)
        return digest
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _remove_unnamed(latest: str, suffix: str, key: str, records: list):
    """the `<latest><suffix><epoch>` files none of `records` names under `key` are removed"""
    keep = {r[key]["file"] for r in records if r.get(key)}
    head, where = os.path.basename(latest) + suffix, os.path.dirname(latest) or "."
    for name in os.listdir(where):
        if name.startswith(head) and name[len(head):].isdigit() and name not in keep:
            os.remove(os.path.join(where, name))


def _save_pair(state, latest: str, record: dict, older: list, world: int, optim_state: dict = None, ema_state: dict = None):
    """`latest` and its sidecar: the checkpoint is written to its temporary file and digested there, the sidecar (the new record in front of
    the one before) is replaced, then `latest` is.  Killed before the first replace: the old pair; between the two: the new sidecar, whose
    older record names the old `latest`; after: the new pair.  optim_state (a trainer with optimizer state): written to `optim_file` of the
    record's epoch (temporary file, then replace) BEFORE the sidecar that names it; the optimizer files neither kept record names are removed
    behind the pair -- a kill at any point leaves a pair whose optimizer file exists.  ema_state (a trainer with a weight average,
    `tr.ema_export()`): `ema_file` of the record's epoch, in exactly the same way"""
    os.makedirs(os.path.dirname(latest) or ".", exist_ok=True)
    tmp = latest + ".tmp"
    try:
        torch.save(state, tmp)
        record["digest"] = _file_digest(tmp)
        if optim_state is not None:
            opath = optim_file(latest, record["epoch"])
            record["optim"] = {"file": os.path.basename(opath), "digest": _save_named(optim_state, opath), "config": optim_state["optim"]}
        if ema_state is not None:
            epath = ema_file(latest, record["epoch"])
            record["ema"] = {"file": os.path.basename(epath), "digest": _save_named(ema_state, epath), "config": ema_state["ema"]}
        _write_json_atomic({"format": _RESUME_FORMAT, "world": world, "records": [record] + older[:1]}, resume_file(latest))
        os.replace(tmp, latest)
        if optim_state is not None:
            _remove_unnamed(latest, OPTIM_SUFFIX, "optim", [record] + older[:1])
        if ema_state is not None:
            _remove_unnamed(latest, EMA_SUFFIX, "ema", [record] + older[:1])
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def run_epochs(F, tr, rank: int, train_epoch: Callable[[int], Tuple[float, int]], validate: Callable[[dict], Tuple[float, str]],
               logfile: str, latest: str, best: str, latest_every_epoch: bool = False, score_key: str = "val_mAP",
               epoch_note: Callable[[], str] = None, generators: Dict[str, object] = None, resume: Resume = None,
               world: int = None) -> Dict[str, float]:
    """--epochs epochs: `tr.lr` from the schedule, `train_epoch(epoch) -> (loss sum, steps)` runs the epoch's steps (it owns the data and
    every random draw), then rank 0 logs and runs `weight_mgt`, and all ranks meet at a barrier.  `weight_mgt` (`Spatial_cnn/run.py:258-269`,
    `Temporal_tenco/run.py:270-282`): every --val_interval epochs `validate(state) -> (score, "<head>: [<mAP>]")`, the best `.pth` by that
    score; `_latest` at validation epochs, or after every epoch with `latest_every_epoch`.  Returns the last epoch's loss and lr (+ its
    validation score under `score_key`).  `epoch_note()`, if given, is appended to the epoch's `Traning |` line.

    --resume (`F.resume`; off: every byte and line as above): `generators` = {name: the host generators `train_epoch` draws from}.  Whenever
    `latest` is written its sidecar is too (`resume_file`: epoch, best score, world, the digest of the `latest` bytes, the generators' states;
    ranks > 0 write their own generators' states), AFTER the epoch's validation and best `.pth`, so the record holds the score of its own
    epoch.  `resume` = what `load_resume(latest, rank, world)` returned at the start of the run (loaded here when not given; the driver has
    loaded `resume.state_dict()` into `tr`): the loop starts at the epoch after the recorded one with that `top` and those generator states.
    {} when nothing is left to train.

    --clip_grad_norm / --skip_nonfinite (`guard_flags`; both off: every byte and line as above): after an epoch's steps `tr.guard_stats(reset=True)`
    is read once and the `Traning |` line gets `| gnorm mean M max X | clipped c | skipped k`; an epoch whose steps were ALL skipped raises a
    RuntimeError before `latest` or `best` is written.  `train_epoch` sums its losses with `LossMean(skip_nonfinite)`.

    Optimizer state (`tr.optimizer_state_dict()` not None: --momentum, --optimizer adamw) under --resume: rank 0 writes it beside every `latest`
    (`optim_file`, named and digested in the record; `_save_pair`), the driver has loaded `resume.optim_state()` into `tr`.  Without --resume no
    optimizer file is written; without optimizer state the sidecar is byte for byte what it was.

    Weight average (`tr.ema_config()` not None: --ema_decay; off: every byte and line as above): `validate` is given `tr.ema_state_dict()`, its
    score decides the best `.pth` and the best `.pth` HOLDS the averaged weights, so everything that loads a best `.pth` gets them; `latest`
    stays the raw weights (a continued run needs them).  --ema_eval both also validates the raw weights and appends `| raw => ...` to the
    `video-wise |` line; that score decides nothing.  The `Traning |` line gets `| ema t N decay D` from the device record (one read per epoch on
    rank 0).  Under --resume rank 0 writes `tr.ema_export()` beside every `latest` (`ema_file`, named and digested in the record), the driver
    has loaded `resume.ema_state()` into `tr`."""
    val_interval = max(1, F.epochs - 1 if F.val_interval == -1 else F.val_interval)
    top, last, first = 0.0, {}, 0
    resuming = bool(getattr(F, "resume", False))
    clip, skip_nonfinite = guard_flags(F)
    guarded = clip > 0 or skip_nonfinite
    ema_config = getattr(tr, "ema_config", lambda: None)()
    averaged, ema_both = ema_config is not None, getattr(F, "ema_eval", "ema") == "both"
    if resuming:
        world = _dist()[1] if world is None else world
        generators = generators or {}
        resume = load_resume(latest, rank, world, getattr(tr, "optim_config", lambda: None)(), ema_config) if resume is None else resume
        older = [resume.record] if resume.record else []           # rank 0: the record on disk that names the `latest` on disk
        own_older = [{"epoch": resume.epoch, "generators": resume.generators}] if resume.epoch >= 0 else []
        if resume.epoch >= 0:
            if set(resume.generators) != set(generators):
                raise ValueError(f"--resume: {resume_file(latest, rank)} holds the generators {sorted(resume.generators)} and this trainer draws "
                                 f"from {sorted(generators)}; it belongs to another trainer or version: start a fresh run")
            for name, g in generators.items():
                _set_generator_state(g, resume.generators[name])
            top, first = resume.top, resume.epoch + 1
            if rank == 0:
                _log(logfile, f"Resuming at epoch {first} (best so far {top:.5f})" if first < F.epochs else
                     f"Resuming: epoch {resume.epoch} was the last of --epochs {F.epochs} (best so far {top:.5f}); nothing left to train")
    for epoch in range(first, F.epochs):
        tr.lr = lr_at_epoch(epoch, F.initial_learning_rates[2], F.power, F.warmups[2], F.decay_rate)
        t0 = time.time()
        tot, steps = train_epoch(epoch)
        note = epoch_note() if epoch_note else ""
        if guarded:                                                # one read of the trainer's device record per epoch; the same on every rank
            gs = tr.guard_stats(reset=True)
            if gs["steps"] > 0 and gs["skipped"] == gs["steps"]:   # before anything is written: a run that can no longer learn stops here
                raise RuntimeError(f"epoch {epoch}: --skip_nonfinite skipped all {gs['steps']} steps (every gradient held a NaN or an Inf); no "
                                   f"checkpoint was written for this epoch.  The parameters or the inputs are no longer finite: look at the data "
                                   f"and at {latest} before starting again")
            note += f" | gnorm mean {gs['norm_mean']:.4g} max {gs['norm_max']:.4g} | clipped {gs['clipped']} | skipped {gs['skipped']}"
            if not steps:                                          # (no step with a finite loss, though some were applied)
                tot, steps = float("nan"), 1
        last = {"loss": tot / steps, "lr": tr.lr}
        val = epoch % val_interval == 0
        ema_state = None
        if rank == 0:
            if averaged:
                er = tr.ema_record()
                note += f" | ema t {er['t']} decay {er['decay']:.6g}"
            _log(logfile, f"Traning | lr: {tr.lr:.6f} | epoch {epoch} | loss {tot / steps:.4f} | {time.time() - t0:.2f} secs" + note)
            if val or latest_every_epoch:
                state = tr.state_dict()
                if not resuming:
                    save_atomic(state, latest)
                else:                                              # (None: the trainer keeps no optimizer state)
                    optim_state = getattr(tr, "optimizer_state_dict", lambda: None)()
                    ema_state = tr.ema_export() if averaged else None
            if val:
                t1 = time.time()
                scored = state if not averaged else ema_state["state"] if ema_state is not None else tr.ema_state_dict()
                score, shown = validate(scored)
                last[score_key] = score
                if score > top or not os.path.exists(best):
                    top = max(top, score)
                    save_atomic(scored, best)
                    _log(logfile, f">>> Saving checkpoint for epoch {epoch + 1} at {best}, time {time.ctime()} ")
                if averaged and ema_both:                          # (the raw weights' score is shown and decides nothing)
                    shown += f" | raw => {validate(state)[1]}"
                _log(logfile, f"\t\t\t\t\t\t\t video-wise | eta {time.time() - t1:.2f} secs | mAP => {shown} ")
        if resuming and (val or latest_every_epoch):
            gens = {name: _generator_state(g) for name, g in generators.items()}
            if rank:
                rec = {"epoch": epoch, "generators": gens}
                _write_json_atomic({"format": _RESUME_FORMAT, "world": world, "rank": rank, "records": [rec] + own_older[:1]}, resume_file(latest, rank))
                own_older = [rec]
            _barrier()                                             # every other rank's record of this epoch is on disk before rank 0's names it
            if rank == 0:
                rec = {"epoch": epoch, "top": top, "generators": gens}
                _save_pair(state, latest, rec, older, world, optim_state, ema_state)
                older = [rec]
        _barrier()
    _barrier()                                                     # the last checkpoint is on disk before any rank goes on to -e
    return last
