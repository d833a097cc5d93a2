"""CPU: the flip-aware staged bound of `fused_bounds` on torch fp32 emulations of the six fused inference launches (layer1 Bottleneck in its
identity / downsample / `next` forms, chain_gemm in its Bottleneck and MLP forms, conv3x3_expand, the stem + max-pool, the one-launch TCN layer).

A correct emulation -- fp32 accumulation, fp32 bias / residual / activation, every hidden map rounded to bf16 (RNE) where the stand-alone launch
stores it, one rounding at the store -- passes in two accumulation orders (torch's own, and K walked in 128-byte chunks from the last to the
first); each emulated bug violates the bound; and the share of outputs the RNE statistics are taken over stays above a floor written next to
each shape (half of what the reference gives: it depends on the reference alone and keeps the statistic from going vacuous)."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_bounds as fb  # noqa: E402
from bf16_bounds import check_bf16  # noqa: E402
from fused_bounds import Stage  # noqa: E402

CHUNK = 64              # bf16 elements in 128 bytes


def _bf(t):
    return t.bfloat16().float()


def _trunc(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------- the cases
# name -> (shape, floor of the selected share = half the share measured on the reference)
CASES = {
    "bottleneck_identity": ((2, 9, 15), 0.159),   # measured 0.3181
    "bottleneck_downsample": ((1, 9, 15), 0.245),   # measured 0.4909
    "bottleneck_next": ((1, 9, 15), 0.198),   # measured 0.3977
    "chain_bottleneck": ((129, 128, 512, 128), 1.0),   # y1 is stored: nothing propagates, every output is selected
    "chain_mlp": ((300, 128), 0.351),   # measured 0.7029
    "expand": ((2, 6, 7), 0.159),   # measured 0.3182
    "stem": ((2, 22, 38), 0.500),   # measured 1.0000
    "tcn": ((2, 40, 2), 0.057),   # measured 0.1156
}


def _mat(g, cout, cin, kh, kw, scale):
    return fb.conv_weight(g, cout, cin, kh, kw, scale)[1]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, stages): operands holding bf16 values, scaled as in the GPU tests; built once and never written to"""
    shape = CASES[name][0]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name.startswith("bottleneck"):
        b, h, w = shape
        cin = 64 if name.endswith("downsample") else 256
        x = fb.ring_image((b, h, w, cin), g)
        b1, b2, b3, bds, bn = fb.distinct_biases((64, 64, 256, 256, 128))
        c1, c2, c3 = (_mat(g, 64, cin, 1, 1, cin ** -0.5), b1), (_mat(g, 64, 64, 3, 3, 1 / 24), b2), (_mat(g, 256, 64, 1, 1, 1 / 8), b3)
        ds = (_mat(g, 256, cin, 1, 1, cin ** -0.5), bds) if name.endswith("downsample") else None
        nx = (_mat(g, 128, 256, 1, 1, 1 / 16), bn) if name.endswith("next") else None
        return x, fb.bottleneck_stages(x, c1, c2, c3, ds, nx)
    if name.startswith("chain"):
        m, k1, n1, n2 = shape if len(shape) == 4 else (shape[0], shape[1], 4 * shape[1], shape[1])
        x = _bf(torch.randn((m, k1), generator=g))
        b1, b2 = fb.distinct_biases((n1, n2))
        w1, w2 = _mat(g, n1, k1, 1, 1, k1 ** -0.5), _mat(g, n2, n1, 1, 1, n1 ** -0.5)
        r = _bf(torch.randn((m, n1 if name == "chain_bottleneck" else n2), generator=g))
        return x, (fb.chain_stages(w1, b1, w2, b2, r1=r) if name == "chain_bottleneck" else fb.chain_stages(w1, b1, w2, b2, r2=r))
    if name == "expand":
        b, h, w = shape
        x = fb.ring_image((b, h, w, 128), g)
        b2, b3 = fb.distinct_biases((128, 512))
        res = _bf(torch.randn((b, h, w, 512), generator=g))
        return x, fb.expand_stages((_mat(g, 128, 128, 3, 3, 1 / 34), b2), (_mat(g, 512, 128, 1, 1, 1 / 11), b3), res)
    if name == "stem":
        b, h, w = shape                                   # the space-to-depth frame of a 3-padded h x w frame: (h + 6) / 2 x (w + 6) / 2 x 16
        x = _bf(torch.randn((b, (h + 6) // 2, (w + 6) // 2, 16), generator=g))
        return x, fb.stem_stages(_mat(g, 64, 16, 4, 4, 0.1), fb.distinct_biases((64,))[0])
    b, t, d = shape
    x = fb.ring_image((b, t, 512), g)
    b1, b2 = fb.distinct_biases((512, 512))
    w1 = (torch.randn((512, 512, 3), generator=g) * 0.03).bfloat16().float().permute(0, 2, 1).reshape(512, -1)
    return x, fb.tcn_stages(x, w1, b1, _mat(g, 512, 512, 1, 1, 0.05), b2, d)


# ------------------------------------------------------------------------------------------------------------------------------ the emulation
def _clamped(x, st):
    """padding that repeats the border pixel (a clamped halo address whose value is not zeroed)"""
    if st.kind == "conv1d":
        p, t = st.dil * (st.taps - 1) // 2, x.shape[1]
        return x[:, torch.arange(-p, t + p).clamp(0, t - 1)]
    (ph, pw), (h, w) = st.pad, x.shape[1:3]
    return x[:, torch.arange(-ph, h + ph).clamp(0, h - 1)][:, :, torch.arange(-pw, w + pw).clamp(0, w - 1)]


def _neighbour(x, st):
    """padding rows (frames) taken from the image (video) before / behind in the batch: a halo address that leaves its image"""
    p = st.dil * (st.taps - 1) // 2 if st.kind == "conv1d" else st.pad[0]
    b, n = x.shape[:2]
    flat = F.pad(x.reshape((1, b * n) + tuple(x.shape[2:])), (0, 0) * (x.dim() - 2) + (p, p))[0]
    out = torch.stack([flat[i * n:(i + 1) * n + 2 * p] for i in range(b)])
    return out if st.kind == "conv1d" else F.pad(out, (0, 0, st.pad[1], st.pad[1]))


def _gemm(p, w, order, bf16_partials):
    if order == "plain" and not bf16_partials:
        return p @ w.T
    acc = torch.zeros(p.shape[:-1] + (w.shape[0],))
    for k0 in reversed(range(0, w.shape[1], CHUNK)):
        part = p[..., k0:k0 + CHUNK] @ w[:, k0:k0 + CHUNK].T
        acc = acc + (_bf(part) if bf16_partials else part)
    return acc


def _act(v, act):
    return {"none": lambda t: t, "relu": torch.relu, "gelu": F.gelu}[act](v)


def emulate(x, stages, order="plain", bug=None, at=-1):
    """every stage's output as the launch holds it (fp32 tensors of bf16 values), in fp32 arithmetic; `bug` applies at stage `at`"""
    x = x.float()

    def run(i, st, h, last):
        here = i == at
        pad_fn = {"clamped_halo": _clamped, "neighbour_image": _neighbour}.get(bug if here else None, fb.zero_pad)
        bias = st.bias.float().roll(1) if here and bug == "neighbour_bias" else st.bias.float()
        acc = _gemm(fb.patches(st, h, pad_fn), st.w.float(), order, here and bug == "bf16_partials")
        act = "relu" if bug == "gelu_as_relu" and st.act == "gelu" else st.act
        if st.pool and bug == "pool_zero_pad":      # pools the accumulators (max commutes with + bias and ReLU) -- but over a border of zeros
            return _bf(_act(_pool_zero(acc) + bias, act))
        v = acc + bias
        r = None
        if isinstance(st.residual, Stage):
            r = run(-2, st.residual, x, False)
        elif st.residual is not None:
            r = st.residual.float()
        if r is not None and here and bug == "residual_after_relu":
            v = _act(v, act) + r
        else:
            v = _act(v + r if r is not None else v, act)
        if st.pool:
            v = fb.pool3x3s2(v)
        if not last and here and bug == "hidden_truncated":
            return _trunc(v)
        if not last and here and bug == "hidden_unrounded":
            return v
        return _bf(v)

    outs, h = [], x
    for i, st in enumerate(stages):
        h = run(i, st, h, i == len(stages) - 1)
        outs.append(h)
    return outs


def _pool_zero(a):
    """3x3 / 2 max-pool whose padding is 0 instead of -inf"""
    return F.max_pool2d(F.pad(a.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2, 0).permute(0, 2, 3, 1)


def judge(name, x, stages, outs):
    """the checks the GPU test applies to the launch's outputs"""
    if name == "chain_bottleneck":          # y1 is stored: each stage against the plain bound, the second on the launch's own y1
        for i, h in enumerate((x, outs[0])):
            fb.check_fused(outs[i], fb.stored_stage(stages[i], x, h), f"{name} y{i + 1}")
    elif name == "bottleneck_next":         # y at the even pixels and t
        ev = (slice(None), slice(None, None, 2), slice(None, None, 2))
        fb.check_fused(outs[2][ev], fb.staged_reference(x, stages[:3]), f"{name} y_even", sl=ev)
        fb.check_fused(outs[3], fb.next_reference(x, stages, outs[2][ev]), f"{name} t")
    else:
        fb.check_fused(outs[-1], _reference(name), name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    x, stages = _case(name)
    return fb.staged_reference(x, stages)


# ----------------------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("order", ["plain", "reverse_chunks"])
@pytest.mark.parametrize("name", list(CASES))
def test_correct_emulation_passes(name, order):
    x, stages = _case(name)
    judge(name, x, stages, emulate(x, stages, order))


BUGS = [
    ("bottleneck_identity", "hidden_truncated", 1), ("chain_mlp", "hidden_truncated", 0), ("expand", "hidden_truncated", 0),
    ("tcn", "hidden_truncated", 0), ("bottleneck_downsample", "hidden_truncated", 0),
    ("bottleneck_identity", "hidden_unrounded", 1), ("chain_mlp", "hidden_unrounded", 0), ("expand", "hidden_unrounded", 0),
    ("tcn", "hidden_unrounded", 0), ("bottleneck_next", "hidden_unrounded", 2),
    ("bottleneck_identity", "bf16_partials", 0), ("chain_bottleneck", "bf16_partials", 0), ("chain_bottleneck", "bf16_partials", 1),
    ("chain_mlp", "bf16_partials", 1), ("expand", "bf16_partials", 0), ("stem", "bf16_partials", 0), ("tcn", "bf16_partials", 1),
    ("bottleneck_identity", "clamped_halo", 1), ("bottleneck_downsample", "clamped_halo", 1), ("expand", "clamped_halo", 0), ("tcn", "clamped_halo", 0),
    ("bottleneck_identity", "neighbour_image", 1), ("expand", "neighbour_image", 0), ("tcn", "neighbour_image", 0),
    ("bottleneck_identity", "neighbour_bias", 1), ("bottleneck_downsample", "neighbour_bias", 2), ("bottleneck_next", "neighbour_bias", 3),
    ("chain_bottleneck", "neighbour_bias", 0), ("chain_mlp", "neighbour_bias", 0), ("expand", "neighbour_bias", 1), ("stem", "neighbour_bias", 0),
    ("tcn", "neighbour_bias", 0),
    ("bottleneck_identity", "residual_after_relu", 2), ("bottleneck_downsample", "residual_after_relu", 2), ("chain_bottleneck", "residual_after_relu", 0),
    ("expand", "residual_after_relu", 1),
    ("chain_mlp", "gelu_as_relu", 0),
    ("stem", "pool_zero_pad", 0),
]


@pytest.mark.parametrize("name,bug,at", BUGS)
def test_emulated_bug_violates_the_bound(name, bug, at):
    x, stages = _case(name)
    outs = emulate(x, stages, "plain", bug, at)
    with pytest.raises(AssertionError, match="bound exceeded or biased"):
        judge(name, x, stages, outs)


@pytest.mark.parametrize("name", [n for n in CASES if n != "chain_bottleneck"])
def test_selected_share_stays_above_its_floor(name):
    """the share of outputs with extra <= ulp / 16 (where `check_bf16` takes its RNE statistics): a property of the reference alone"""
    x, stages = _case(name)
    f = fb.next_reference(x, stages, emulate(x, stages)[2][:, ::2, ::2]) if name == "bottleneck_next" else _reference(name)
    share = f.selected_share()
    print(f"{name} {CASES[name][0]}: selected share {share:.4f}")
    assert share >= CASES[name][1] > 0.0


def test_flip_delta():
    """zero away from a rounding boundary, one ulp across it, and ReLU's kink: a hidden value the kernel may compute on either side of zero"""
    z = torch.tensor([1.0 + 2 ** -9, 1.0 + 2 ** -8 - 2 ** -30, 1.0 + 2 ** -8 + 2 ** -30, -2 ** -30, 3.0], dtype=torch.float64)
    d = torch.full_like(z, 2.0 ** -24)
    got = fb.flip_delta(z, d, "relu")
    assert got[0] == 0 and got[1] == 2 ** -7 and got[2] == 2 ** -7 and got[4] == 0
    assert got[3] == fb.rne_bf16(torch.tensor(2.0 ** -24 - 2.0 ** -30, dtype=torch.float64))
    assert float(fb.flip_delta(torch.tensor([0.5], dtype=torch.float64), torch.tensor([0.0], dtype=torch.float64), "gelu")) >= 0.0


def test_plain_reference_with_rounded_hidden_maps_is_not_enough():
    """why the deltas exist: a launch whose every hidden pre-activation is off by the whole accumulation term, all to the same side -- allowed by
    the model, and exact in everything else -- is within the staged bound, and outside the single-rounding bound of the same reference without
    its deltas (extra = 0)"""
    import math
    x, stages = _case("chain_mlp")
    f = _reference("chain_mlp")
    x64 = x.double()
    z, acc, _, k = fb._terms(stages[0], x64, x64, torch.zeros_like(x64))
    h = fb.rne_bf16(fb.gelu64(z + math.sqrt(k) * fb.ACC_EPS * acc))
    assert 0 < float((h != f.hidden[0].value).double().mean()) < 0.05 and bool(((h - f.hidden[0].value).abs() <= f.hidden[0].delta).all())
    got = fb.rne_bf16(fb.stored_stage(stages[1], x, h).ref64).bfloat16()
    fb.check_fused(got, f, "shifted hidden map")
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_bf16(got, f.ref64, acc64=f.acc64, k=f.k, what="no deltas")
