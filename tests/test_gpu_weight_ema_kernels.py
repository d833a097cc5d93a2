"""GPU: the weight-average kernels (`mt4_ema_advance`, `mt4_ema_step_f32`; csrc/update_kernels.hip) against their host restatements
`ops.ema_advance_host` / `ops.ema_step_host`, BIT FOR BIT on an int32 view of e: five consecutive steps at sizes that cover every tail length, a
buffer shorter than one vector, one element past a workgroup's span and a buffer longer than the capped grid covers in one pass; a skipping guard
record writes nothing; elements behind n are untouched; the record follows the host's doubles exactly, skipped steps included.  Non-finite
numbers here are DATA fed to correct kernels."""
import struct

import numpy as np
import pytest
import torch

from test_optimizer_state_cpu import _ramps

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1025, 2 ** 22 + 3]          # 2^22 + 3: 2^20 float4s = 4096 workgroups' worth, twice the 2048 the launch caps at
PAD = 8                                                          # elements behind n: pre-filled, must stay
FILL = -7.25
STEPS = 5
FRESH = {"t": 0, "decay": 0.0, "comp": 1.0}


def _guard_tensor(cuda, coef=1.0, skip=0):
    """an mt4_guard_state as `mt4_grad_guard_finalize` would leave it: double sumsq, double norm, float coef, int32 skip, int64 nonfinite"""
    raw = struct.pack("<ddfiq", 4.0, 2.0, coef, skip, 1 if skip else 0)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.float64).copy()).to(cuda)


def _padded(x, cuda):
    return torch.cat([x, torch.full((PAD,), FILL)]).to(cuda)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _tile(a, n):
    return torch.from_numpy(np.resize(a, n).astype(np.float32))


def _ramp_inputs(n, step):
    """the power-of-two ramps of the CPU test (exponents -12 .. 12, all four sign pairs), repeated to n elements; p walks from step to step"""
    e0, _ = _ramps(0)
    return _tile(e0, n), _tile(_ramps(step)[1], n)


def _real_inputs(n, step):
    """real-valued draws; from 16 elements on also subnormals, zeros of both signs and -- in p, at one index -- a NaN"""
    g = torch.Generator().manual_seed(1000 * step + n % 991)
    e, p = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    nan_at = None
    if n >= 16:
        tiny = float(np.finfo(np.float32).tiny)
        e[1], e[2], e[3], e[4] = tiny / 4, -tiny / 1024, 0.0, -0.0
        p[1], p[2], p[3], p[5] = -tiny / 8, tiny * 0.75, -0.0, 0.0
        p[n - 6], e[n - 7] = tiny / 2, tiny / 16
        if step == 1:
            nan_at = n - 3
            p[nan_at] = float("nan")
    return e, p, nan_at


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("decay,warmup", [(0.999, False), (0.9, True)], ids=["0.999", "0.9-warmup"])
def test_step_equals_the_host_restatement_bit_for_bit(cuda, n, decay, warmup):
    from computervision_codes_amd import ops
    guards = (("unguarded", None), ("guarded", _guard_tensor(cuda, 0.5)))
    for kind in ("ramp", "real"):
        for gname, guard in (guards if n <= 4096 else guards[:1] if kind == "ramp" else guards[1:]):      # (the long buffer: one guard form per input kind)
            e =_ramp_inputs(n, 0)[0] if kind == "ramp" else _real_inputs(n, 0)[0]
            de, rec_dev, rec = _padded(e, cuda), ops.ema_state_buffer(cuda), dict(FRESH)
            nans = set()
            for step in range(STEPS):                                    # consecutive: an error would compound
                if kind == "ramp":
                    p, nan_at = _ramp_inputs(n, step)[1], None
                else:
                    _, p, nan_at = _real_inputs(n, step)
                dp = _padded(p, cuda)
                rec = ops.ema_advance_host(rec, decay, warmup)
                want = ops.ema_step_host(e, p, rec)
                ops.ema_advance(rec_dev, decay, warmup, guard)
                ops.ema_step(de[:n], dp[:n], rec_dev, guard)
                what = f"{kind} {gname} n={n} step {step}"
                assert ops.read_ema_state(rec_dev) == rec, what
                got = de[:n].cpu()
                if nan_at is not None:
                    nans.add(nan_at)
                mask = torch.isnan(want)
                assert set(torch.nonzero(mask).flatten().tolist()) == nans, what             # the NaN is data: at its own index, nowhere else
                assert torch.equal(torch.isnan(got), mask), what
                ok = ~mask
                assert torch.equal(_bits(got)[ok], _bits(want)[ok]), f"{what}: {int((_bits(got)[ok] != _bits(want)[ok]).sum())} of {n} elements differ"
                assert bool((de[n:].cpu() == FILL).all()), f"{what}: wrote behind n"
                assert torch.equal(_bits(dp[:n])[~torch.isnan(p)], _bits(p)[~torch.isnan(p)]) and bool((dp[n:].cpu() == FILL).all()), what
                e = want
            if kind == "real" and n >= 16:
                assert nans and bool((e[~torch.isnan(e)].abs() < float(np.finfo(np.float32).tiny)).any())     # subnormals were in play


@pytest.mark.parametrize("n", [5, 2 ** 22 + 3])
def test_a_skipping_guard_record_writes_nothing_and_a_passing_one_moves_both(cuda, n):
    from computervision_codes_amd import ops
    e, p, _ = _real_inputs(n, 0)
    de, dp = _padded(e, cuda), _padded(p, cuda)
    rec_dev = ops.ema_state_buffer(cuda)
    ops.ema_advance(rec_dev, 0.9, True)                                  # a record one step in
    before_e, before_rec = de.clone(), rec_dev.clone()
    skip = _guard_tensor(cuda, 1.0, skip=1)
    ops.ema_advance(rec_dev, 0.9, True, skip)
    ops.ema_step(de[:n], dp[:n], rec_dev, skip)
    assert torch.equal(_bits(de), _bits(before_e)) and torch.equal(rec_dev.view(torch.int64), before_rec.view(torch.int64))
    go = _guard_tensor(cuda, 1.0, skip=0)                                # the same call with skip = 0 moves them
    ops.ema_advance(rec_dev, 0.9, True, go)
    ops.ema_step(de[:n], dp[:n], rec_dev, go)
    rec = ops.ema_advance_host(ops.ema_advance_host(dict(FRESH), 0.9, True), 0.9, True)
    assert ops.read_ema_state(rec_dev) == rec and rec["t"] == 2
    assert not torch.equal(_bits(de[:n]), _bits(before_e[:n]))
    assert torch.equal(_bits(de[:n]), _bits(ops.ema_step_host(e, p, rec))) and bool((de[n:].cpu() == FILL).all())


def test_the_record_follows_the_host_over_twelve_steps_with_two_skipped(cuda):
    """decay 0.5 with warmup: (1 + t) / (10 + t) reaches 0.5 at t = 8, inside the ten counted steps -- the ramp, the crossover and the plateau"""
    from computervision_codes_amd import ops
    rec_dev, rec = ops.ema_state_buffer(cuda), dict(FRESH)
    assert ops.read_ema_state(rec_dev) == rec
    skip, go = _guard_tensor(cuda, 1.0, skip=1), _guard_tensor(cuda, 0.25, skip=0)
    seen = []
    for step in range(12):
        skipped = step in (4, 5)
        guard = skip if skipped else go if step % 2 else None
        ops.ema_advance(rec_dev, 0.5, True, guard)
        rec = ops.ema_advance_host(rec, 0.5, True, skip=skipped)
        got = ops.read_ema_state(rec_dev)
        assert got == rec, (step, got, rec)                              # t and both floats equal
        seen.append((rec["t"], rec["decay"]))
    assert rec == {"t": 10, "decay": 0.5, "comp": 0.5}
    assert seen[3] == seen[4] == seen[5] and seen[6][0] == 5             # the skipped steps left the record as it was
    assert seen[0] == (1, float(np.float32(2 / 11))) and [d for t, d in seen if t == 7] == [float(np.float32(8 / 17))] and seen[-3][1] == 0.5
    # no warmup: the floats of the decay itself from the first step on
    ops.write_ema_state(rec_dev, 0, 0.0, 1.0)
    ops.ema_advance(rec_dev, 0.999, False)
    assert ops.read_ema_state(rec_dev) == {"t": 1, "decay": float(np.float32(0.999)), "comp": float(np.float32(1.0 - 0.999))}
