"""CPU: the per-element fp32 bound of `bf16_bounds.check_f32` on the fp32 training kernels' arithmetic.

A correct fp32 weight-gradient reduction of a dilated Conv1d (row range split over workgroups, fp32 partial sums added in fp32, as
`mt4_wgrad_conv1d_f32` and `mt4_wgrad_conv2d_f32` do) and a correct SGD update pass it; each of seven subtly wrong ones fails it.  The operands
carry per-channel power-of-two scales from 2^8 down to 2^-8 (descending with the channel index, so the ragged tail tiles hold the smallest
values), as the GPU tests' operands do.  The max-scaled tolerance the GPU tests used before accepts the corner form of (a), and (b), (c) and (e):

  (a) the partial sum of the last row split dropped -- everywhere (the old tolerance rejects that too), or only in the workgroup of the ragged
      corner tile (it does not)
  (b) a tap shift that crosses a sequence boundary reads the neighbouring sequence's row instead of zero, in the workgroup of the ragged corner
      tile (last output-channel tile x last K tile) -- the same leak in every workgroup moves the largest elements, and the old tolerance
      rejects that one too (shown below)
  (c) the ragged corner tile's partial sum added twice; one K column of the ragged output-channel tile left stale
  (d) accumulate mode overwriting the output instead of adding to it
  (e) the SGD tail (index n - n % 4 .. n - 1, the scalar loop) updated without the weight decay
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bf16_bounds import check_exact, check_f32, pow2_ramp, rne_f32, sgd_ref64  # noqa: E402

B, T, CIN, COUT, TAPS, DIL = 4, 250, 100, 72, 3, 4
PAD = DIL * (TAPS - 1) // 2
K = TAPS * CIN                      # 300 packed columns: K tiles of 64 at 0, 64, .., 256 (the last one ragged)
SPLITS = 4                          # row splits of 256 rows (the kernels' minimum)


def _operands(seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((B * T, CIN), generator=g) * 2 - 1) * pow2_ramp(CIN)
    dy = (torch.rand((B * T, COUT), generator=g) * 2 - 1) * pow2_ramp(COUT)
    return x, dy


def _shifted(x, leak_cols=None):
    """[B*T, K]: column tap*CIN + ci of row (b, t) = x[b, t + tap*DIL - PAD, ci], zero outside [0, T); in `leak_cols` the row is read from
    the flat [B*T] array instead, i.e. from the neighbouring sequence across a boundary (zero only at the ends of the whole array)"""
    t = torch.arange(B * T) % T
    m = torch.arange(B * T)
    cols = []
    for tap in range(TAPS):
        s = tap * DIL - PAD
        ok = ((t + s) >= 0) & ((t + s) < T)
        inb = ((m + s) >= 0) & ((m + s) < B * T)
        src = x[(m + s).clamp(0, B * T - 1)]
        right = torch.where(ok[:, None], src, torch.zeros_like(src))
        leak = torch.where(inb[:, None], src, torch.zeros_like(src))
        cols.append((right, leak))
    good = torch.cat([c[0] for c in cols], 1)
    if leak_cols is None:
        return good
    bad = torch.cat([c[1] for c in cols], 1)
    sel = torch.zeros(K, dtype=torch.bool)
    sel[leak_cols] = True
    return torch.where(sel[None], bad, good)


def _reduce_f32(dy, xs, drop_last_split=False):
    """fp32: per row split a fp32 partial product, partials added in fp32 in split order (the atomics)"""
    rows = B * T // SPLITS
    out = torch.zeros((COUT, K))
    for s in range(SPLITS - (1 if drop_last_split else 0)):
        out += dy[s * rows:(s + 1) * rows].t() @ xs[s * rows:(s + 1) * rows]
    return out


def _ref64(dy, xs):
    return dy.double().t() @ xs.double(), dy.double().abs().t() @ xs.double().abs()


def _old_wgrad_tolerance_accepts(got, ref64, rel=2e-5):
    """the assertion of test_wgrad_conv1d_long_rows_vs_autograd: max |err| < 2e-5 x max(1, max |ref|) (4e-5 for the accumulating call)"""
    return (got.double() - ref64).abs().max().item() < rel * max(1.0, ref64.abs().max().item())


def test_rne_f32_and_check_exact():
    r = torch.randn(10000, dtype=torch.float64) * 10.0 ** torch.randint(-30, 30, (10000,)).double()
    assert torch.equal(rne_f32(r), r.float().double())
    assert rne_f32(torch.tensor([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24], dtype=torch.float64)).tolist() == [1.0, 1.0 + 2.0 ** -22]  # ties to even
    a = torch.arange(12.0).view(3, 4)
    check_exact(a.clone(), a, what="copy")
    b = a.clone()
    b[2, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"first differing element \(2, 1\)"):
        check_exact(b, a, what="nan")
    with pytest.raises(AssertionError, match="exact copy differs"):
        check_exact(torch.tensor([0.0]), torch.tensor([-0.0]).abs() + 2.0 ** -149, what="denormal")
    with pytest.raises(AssertionError, match=r"first differing element \(1,\)"):
        check_exact(torch.tensor([1.0, -0.0]), torch.tensor([1.0, 0.0], dtype=torch.float64), what="signed zero")     # bit patterns, not values


def test_single_rounding_f32_catches_a_double_rounding():
    g = torch.Generator().manual_seed(3)
    a, b, c = (torch.randn(20000, generator=g) for _ in range(3))
    ref64 = a.double() * b.double() + c.double()
    fma = rne_f32(ref64).float()                      # one rounding: what an FMA stores
    st = check_f32(fma, ref64, single_rounding=True, what="fma")
    assert st["match"] == 1.0
    acc64 = (a.double() * b.double()).abs() + c.double().abs()
    check_f32(a * b + c, ref64, acc64=acc64, k=2, what="mul then add")      # two roundings: inside the two-rounding bound ...
    with pytest.raises(AssertionError, match="bound exceeded or biased"):
        check_f32(a * b + c, ref64, acc64=acc64, k=2, single_rounding=True, what="mul then add as one rounding")   # ... but not RNE of the exact result


def test_correct_reduction_passes():
    x, dy = _operands(1)
    xs = _shifted(x)
    ref64, acc64 = _ref64(dy, xs)
    st = check_f32(_reduce_f32(dy, xs), ref64, acc64=acc64, k=B * T, what="correct wgrad_conv1d emulation")
    assert st["worst_ratio"] < 0.5
    base = (torch.rand((COUT, K), generator=torch.Generator().manual_seed(2)) * 2 - 1) * ref64.abs().float()
    check_f32(base + _reduce_f32(dy, xs), base.double() + ref64, acc64=base.double().abs() + acc64, k=B * T + 1, what="correct accumulate")


def _bug_a(dy, x):
    return _reduce_f32(dy, _shifted(x), drop_last_split=True)


def _bug_a_corner(dy, x):
    out = _reduce_f32(dy, _shifted(x))
    out[64:, 256:] = _reduce_f32(dy, _shifted(x), drop_last_split=True)[64:, 256:]
    return out


def _bug_b(dy, x):
    out = _reduce_f32(dy, _shifted(x))
    out[64:, 256:] = _reduce_f32(dy, _shifted(x, leak_cols=slice(256, K)))[64:, 256:]
    return out


def _bug_c_twice(dy, x):
    out = _reduce_f32(dy, _shifted(x))
    out[64:, 256:] *= 2.0
    return out


def _bug_c_stale(dy, x):
    out = _reduce_f32(dy, _shifted(x))
    out[64:, 70] = 0.0                                 # the zeroed buffer's value
    return out


@pytest.mark.parametrize("bug,old_accepts", [(_bug_a, False), (_bug_a_corner, True), (_bug_b, True), (_bug_c_twice, True), (_bug_c_stale, True)])
def test_emulated_wgrad_bug_rejected(bug, old_accepts):
    x, dy = _operands(10)
    ref64, acc64 = _ref64(dy, _shifted(x))
    got = bug(dy, x)
    assert _old_wgrad_tolerance_accepts(got, ref64) == old_accepts
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(got, ref64, acc64=acc64, k=B * T, what=bug.__name__)


def test_boundary_leak_in_every_workgroup_is_seen_by_the_old_tolerance_too():
    x, dy = _operands(11)
    ref64, _ = _ref64(dy, _shifted(x))
    assert not _old_wgrad_tolerance_accepts(_reduce_f32(dy, _shifted(x, leak_cols=slice(0, K))), ref64)


def test_emulated_accumulate_overwrite_rejected():
    x, dy = _operands(12)
    xs = _shifted(x)
    ref64, acc64 = _ref64(dy, xs)
    base = (torch.rand((COUT, K), generator=torch.Generator().manual_seed(13)) * 2 - 1) * ref64.abs().float() * 0.01
    got = _reduce_f32(dy, xs)                          # (d): base overwritten
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(got, base.double() + ref64, acc64=base.double().abs() + acc64, k=B * T + 1, what="accumulate overwrites")


# ------------------------------------------------------------------------------------------------ SGD
LR, WD, GS = 0.05, 1e-5, 0.5


def _sgd_operands(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand(n, generator=g) * 2 - 1) * pow2_ramp(n)
    gr = (torch.rand(n, generator=g) * 2 - 1) * pow2_ramp(n) * 2.0 ** -6
    return p, gr


def _sgd_f32(p, g, lr, wd, gs, tail_wd=None):
    n = p.numel()
    out = p - lr * (g * gs + wd * p)
    t0 = n - n % 4
    if tail_wd is not None:
        out[t0:] = p[t0:] - lr * (g[t0:] * gs + tail_wd * p[t0:])
    return out


def test_sgd_correct_passes_and_tail_without_weight_decay_rejected():
    n = 4 * 40 + 3
    p, g = _sgd_operands(n, 20)
    ref64, acc64 = sgd_ref64(p, g, LR, WD, GS)
    # up to four fp32 roundings inside the bracket, each a relative 2^-24 of a term of acc64: k = 16 (the output's own rounding is the half-ulp)
    check_f32(_sgd_f32(p, g, LR, WD, GS), ref64, acc64=acc64, k=16, what="sgd correct")
    bad = _sgd_f32(p, g, LR, WD, GS, tail_wd=0.0)
    # the old tolerance: the whole-step parameter check of test_train_step_vs_oracle_every_tensor, 2e-5 x max(1, max |new|)
    assert (bad.double() - ref64).abs().max().item() <= 2e-5 * max(1.0, ref64.abs().max().item())
    with pytest.raises(AssertionError, match=rf"bound exceeded.*worst element \(({n - 3}|{n - 2}|{n - 1}),\)"):
        check_f32(bad, ref64, acc64=acc64, k=16, what="sgd tail without weight decay")
