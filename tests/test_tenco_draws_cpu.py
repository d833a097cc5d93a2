"""CPU: the host form of the Temporal_tenco device draws (`tenco_draws.host_masks`, `slots`) and the reference's sub-clip sampling
(`tenco_clip`, `Temporal_tenco/dataloader.py:219-222`)."""
import random

import numpy as np
import pytest
import torch

from computervision_codes_amd import tenco_draws as td

STAGES = [("PG", 3), ("Rs.0", 2), ("Rs.1", 2), ("Rs.2", 2)]


def test_host_masks_shapes_and_values():
    T, D, C = 37, 32, 64
    lens = [37, 11, 5, 3]
    m = td.host_masks(123, 4, T, D, C, STAGES, lens)
    assert tuple(m["input_mask"].shape) == (1, D, T) and m["input_mask"].dtype == torch.float32
    assert set(m["input_mask"].unique().tolist()) == {0.0, 1.0}
    assert tuple(m["channel_mask"].shape) == (1, D, 1) and set(m["channel_mask"].unique().tolist()) == {0.0, 2.0}
    assert list(m["layer_masks"]) == [f"{p}.layers.{i}" for p, n in STAGES for i in range(n)]
    for si, (p, n) in enumerate(STAGES):
        for i in range(n):
            lm = m["layer_masks"][f"{p}.layers.{i}"]
            assert tuple(lm.shape) == (1, C, lens[max(si - 1, 0)]) and set(lm.unique().tolist()) == {0.0, 2.0}
    assert td.host_masks(123, 4, T, D, C, STAGES, lens, input_mask=False)["input_mask"] is None
    # element (t, c) of the device's row-major [T][C] buffer is draw t*C + c
    flat = td.keep_mask(123, 4, td.stage_slots(STAGES)["Rs.1.layers.1"], lens[1] * C)
    assert torch.equal(m["layer_masks"]["Rs.1.layers.1"][0].T.contiguous().flatten(), torch.from_numpy(flat))


@pytest.mark.parametrize("n", [4, 512, 18944])
def test_input_mask_has_exactly_three_quarters_ones(n):
    D = 4 if n == 4 else 512 if n == 18944 else 64
    m = td.host_masks(7, 2, n // D, D, 8, [("PG", 1)], [n // D])["input_mask"]
    assert int(m.sum()) == (3 * n) // 4 == int(n * 0.75)
    keep, thr = td.input_keep(7, 2, n)
    ks = td.keys(7, 2, td.SLOT_INPUT_KEYS, n)
    assert len(np.unique(ks)) == n and int((ks <= np.uint64(thr)).sum()) == (3 * n) // 4
    assert torch.equal(m[0].T.contiguous().flatten(), torch.from_numpy(keep.astype(np.float32)))


def test_step_and_slot_change_the_draw():
    a = td.host_masks(5, 0, 16, 32, 64, STAGES, [16] * 4)
    b = td.host_masks(5, 1, 16, 32, 64, STAGES, [16] * 4)
    c = td.host_masks(6, 0, 16, 32, 64, STAGES, [16] * 4)
    for other in (b, c):
        assert not torch.equal(a["input_mask"], other["input_mask"]) and not torch.equal(a["channel_mask"], other["channel_mask"])
        assert all(not torch.equal(a["layer_masks"][k], other["layer_masks"][k]) for k in a["layer_masks"])
    lm = list(a["layer_masks"].values())
    assert all(not torch.equal(lm[i], lm[j]) for i in range(len(lm)) for j in range(i))       # every layer its own slot
    assert torch.equal(a["input_mask"], td.host_masks(5, 0, 16, 32, 64, STAGES, [16] * 4)["input_mask"])


def test_slots_unique_and_within_a_step():
    s = td.slots(11, 10, 3)
    assert len(s) == 2 + 11 + 3 * 10 and len(set(s.values())) == len(s)
    assert all(0 <= v < 4096 == td.SLOTS_PER_STEP for v in s.values())
    assert {"input_keys", "channel", "PG.layers.0", "PG.layers.10", "Rs.0.layers.0", "Rs.2.layers.9"} <= set(s)
    # the stream of (step, slot) is step * 4096 + slot: consecutive steps cannot collide
    assert td.keys(3, 0, 4095, 4)[0] != td.keys(3, 1, 0, 4)[0]


def _clip_independent(rng, length):
    """`dataloader.py:220-222` spelled with random() / choice(range(...))"""
    if rng.random() > 0.7 and length > 10:
        n = rng.choice(range(10, 1000 if length > 1000 else length))
        return rng.choice(range(0, length - n)), n
    return 0, length


@pytest.mark.parametrize("length", [11, 12, 700, 3000])
def test_tenco_clip_equals_the_reference_arithmetic(length):
    a, b = random.Random(length), random.Random(length)
    clipped = 0
    for _ in range(10000):
        got, want = td.tenco_clip(a, length), _clip_independent(b, length)
        assert got == want
        start, n = got
        if n != length:
            clipped += 1
            assert 10 <= n <= min(1000, length) - 1 and 0 <= start <= length - n - 1
        else:
            assert start == 0
    assert a.getstate() == b.getstate()
    assert 2500 < clipped < 3500            # both branches: P(clip) = 0.3


def test_tenco_clip_takes_short_videos_whole():
    a, b = random.Random(1), random.Random(1)
    for _ in range(200):
        assert td.tenco_clip(a, 10) == (0, 10) and td.tenco_clip(a, 3) == (0, 3)
        b.random(), b.random()              # one random() per item, nothing else
    assert a.getstate() == b.getstate()
