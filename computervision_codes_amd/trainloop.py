"""The epoch and checkpoint loop the four training drivers share (`Spatial_cnn`, `Spatial_transformer`, `Temporal_tenco`, `Temporal_mstct`
`run.py -t`): the schedule flags, `lr_at_epoch`, the round-robin dealing of batches to ranks, the `Traning | lr:` line and one `weight_mgt`.
Host code only: it imports without the HIP library."""
from __future__ import annotations

import argparse
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


def run_epochs(F, tr, rank: int, train_epoch: Callable[[int], Tuple[float, int]], validate: Callable[[dict], Tuple[float, str]],
               logfile: str, latest: str, best: str, latest_every_epoch: bool = False, score_key: str = "val_mAP",
               epoch_note: Callable[[], str] = None) -> Dict[str, float]:
    """--epochs epochs: `tr.lr` from the schedule, `train_epoch(epoch) -> (loss sum, steps)` runs the epoch's steps (it owns the data and
    every random draw), then rank 0 logs and runs `weight_mgt`, and all ranks meet at a barrier.  `weight_mgt` (`Spatial_cnn/run.py:258-269`,
    `Temporal_tenco/run.py:270-282`): every --val_interval epochs `validate(state) -> (score, "<head>: [<mAP>]")`, the best `.pth` by that
    score; `_latest` at validation epochs, or after every epoch with `latest_every_epoch`.  Returns the last epoch's loss and lr (+ its
    validation score under `score_key`).  `epoch_note()`, if given, is appended to the epoch's `Traning |` line."""
    val_interval = max(1, F.epochs - 1 if F.val_interval == -1 else F.val_interval)
    top, last = 0.0, {}
    for epoch in range(F.epochs):
        tr.lr = lr_at_epoch(epoch, F.initial_learning_rates[2], F.power, F.warmups[2], F.decay_rate)
        t0 = time.time()
        tot, steps = train_epoch(epoch)
        last = {"loss": tot / steps, "lr": tr.lr}
        if rank == 0:
            _log(logfile, f"Traning | lr: {tr.lr:.6f} | epoch {epoch} | loss {tot / steps:.4f} | {time.time() - t0:.2f} secs" + (epoch_note() if epoch_note else ""))
            val = epoch % val_interval == 0
            if val or latest_every_epoch:
                state = tr.state_dict()
                save_atomic(state, latest)
            if val:
                t1 = time.time()
                score, shown = validate(state)
                last[score_key] = score
                if score > top or not os.path.exists(best):
                    top = max(top, score)
                    save_atomic(state, best)
                    _log(logfile, f">>> Saving checkpoint for epoch {epoch + 1} at {best}, time {time.ctime()} ")
                _log(logfile, f"\t\t\t\t\t\t\t video-wise | eta {time.time() - t1:.2f} secs | mAP => {shown} ")
        _barrier()
    _barrier()                                                     # the last checkpoint is on disk before any rank goes on to -e
    return last
