"""The random pieces of a Temporal_tenco training step as functions of (seed, step): what `csrc/tenco_draw_kernels.hip` draws on the device,
reproduced on the host bit for bit, and the reference's sub-clip sampling.  Pure numpy / torch-CPU: imports without the HIP library.

A step's draws are numbered by *slots*; draw `slot` of step `step` is the counter stream `synth.uniform01(seed, step * 4096 + slot, n)`:
    base = splitmix64(seed * 0x100000001B3 + step * 4096 + slot),   key_i = splitmix64(base + i),   u_i = (key_i >> 11) * 2^-53
* slot 0: keys of the 75 % input mask (`Temporal_tenco/network.py:43-48`).  Element t*D + d is kept where its key is among the (3 T D) // 4
  smallest -- exactly `int(n * 0.75)` ones, the count the reference gets from a permutation; the keys are distinct (splitmix64's finaliser
  is a bijection), so "the k smallest" needs no tie rule.
* slot 1: Dropout2d over the D input channels (`network.py:123-127`): 2 where u_d >= 0.5, else 0.
* slots 2 ...: nn.Dropout of each DilatedResidualLayer (`network.py:194-196`), stages in order, over the device's row-major [T_stage][C]
  layout: element t*C + c is 2 where u >= 0.5, else 0.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import synth

SLOTS_PER_STEP = 4096
SLOT_INPUT_KEYS = 0
SLOT_CHANNEL = 1
_FIRST_LAYER_SLOT = 2


def stage_slots(stages: Sequence[Tuple[str, int]]) -> Dict[str, int]:
    """slot of every draw of a step for `stages` = [(prefix, layers), ...] in forward order"""
    out = {"input_keys": SLOT_INPUT_KEYS, "channel": SLOT_CHANNEL}
    s = _FIRST_LAYER_SLOT
    for prefix, n in stages:
        for i in range(n):
            out[f"{prefix}.layers.{i}"] = s
            s += 1
    assert s <= SLOTS_PER_STEP, "more draws in a step than slots"
    return out


def slots(LP: int, LR: int, R: int) -> Dict[str, int]:
    """slot of every draw of a step: 'input_keys', 'channel' and '<prefix>.layers.<i>' for PG (LP layers) and Rs.0 .. Rs.R-1 (LR layers)"""
    return stage_slots([("PG", LP)] + [(f"Rs.{r}", LR) for r in range(R)])


def _stream(step: int, slot: int) -> int:
    assert 0 <= slot < SLOTS_PER_STEP
    return step * SLOTS_PER_STEP + slot


def keys(seed: int, step: int, slot: int, n: int) -> np.ndarray:
    """key_0 .. key_{n-1} of a draw (uint64)"""
    base = synth._splitmix64(np.array([(seed * 0x100000001B3 + _stream(step, slot)) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0]
    with np.errstate(over="ignore"):
        ctr = np.arange(n, dtype=np.uint64) + base
    return synth._splitmix64(ctr)


def keep_mask(seed: int, step: int, slot: int, n: int, p: float = 0.5) -> np.ndarray:
    """nn.Dropout(p) keep mask of a draw, float32: 1/(1-p) (in float32, as the kernels form it) where u_i >= p, else 0"""
    p32 = np.float32(p)
    u = synth.uniform01(seed, _stream(step, slot), n)
    return np.where(u >= np.float64(p32), np.float32(1.0) / (np.float32(1.0) - p32), np.float32(0.0)).astype(np.float32)


def input_keep(seed: int, step: int, n: int) -> Tuple[np.ndarray, int]:
    """(bool [n] with exactly (3 n) // 4 ones, the threshold key) of the input mask"""
    k = (3 * n) // 4
    ks = keys(seed, step, SLOT_INPUT_KEYS, n)
    if k == 0:
        return np.zeros(n, dtype=bool), 0
    thr = np.partition(ks, k - 1)[k - 1]
    return ks <= thr, int(thr)


def host_masks(seed: int, step: int, T: int, D: int, C: int, stages: Sequence[Tuple[str, int]], level_lengths: Sequence[int],
               input_mask: bool = True) -> dict:
    """the draws of step (seed, step) as the reference-shaped tensors `TencoTrainer.draw_masks` returns: 'input_mask' [1,D,T] of {0,1} (None
    without `input_mask`), 'channel_mask' [1,D,1] of {0,2}, 'layer_masks' {prefix.layers.i: [1,C,T_stage]} of {0,2}.  `stages` =
    [(prefix, layers), ...]; `level_lengths` = frames of the FPN levels: stage s > 0 runs at level_lengths[s - 1], the first at T."""
    sl = stage_slots(stages)
    rows = lambda flat, t, c: torch.from_numpy(np.ascontiguousarray(flat.reshape(t, c).T)).unsqueeze(0)     # device order [t][c] -> [1,c,t]
    out = {"input_mask": rows(input_keep(seed, step, T * D)[0].astype(np.float32), T, D) if input_mask else None,
           "channel_mask": torch.from_numpy(keep_mask(seed, step, SLOT_CHANNEL, D)).view(1, D, 1), "layer_masks": {}}
    for si, (prefix, n) in enumerate(stages):
        ts = level_lengths[max(si - 1, 0)]
        for i in range(n):
            name = f"{prefix}.layers.{i}"
            out["layer_masks"][name] = rows(keep_mask(seed, step, sl[name], ts * C), ts, C)
    return out


def tenco_clip(rng, length: int) -> Tuple[int, int]:
    """the frames of one training item, (start, n), by the arithmetic of `Temporal_tenco/dataloader.py:220-222`: with probability 0.3 a window
    of n in [10, min(1000, length) - 1] frames starting in [0, length - n - 1], else the whole video (0, length).  `rng` is a
    `random.Random`; it is consumed exactly as the reference consumes the global generator (one `random()`, then two uniform picks from a
    range when it exceeds 0.7).  Videos of <= 10 frames are taken whole: the reference's `range(10, len)` is empty there and its `choice`
    raises.  (The driver also takes a clip whole that --hier cannot pool: `TencoTrainer.level_lengths`.)"""
    if not rng.random() > 0.7 or length <= 10:
        return 0, length
    n = rng.randrange(10, min(1000, length))
    return rng.randrange(0, length - n), n
