"""Float64 references and per-element bounds for launches that keep one to three intermediate maps on chip and round them to bf16 there
(`mt4_bottleneck_fused*_bf16`, `mt4_chain_gemm_bf16`, the `fuse_expand` form of `mt4_conv_nhwc`, `mt4_stem_maxpool_bf16`,
`mt4_tcn_layer_fused_bf16`).

The contract of such a launch is "every hidden map is rounded to bf16 (RNE) where the stand-alone launch would store it".  A float64 reference
that rounds its hidden maps the same way is still not within half an ulp of a correct kernel: a hidden element whose exact value lies within the
fp32 accumulation error of a rounding boundary may round the other way in the kernel, and that whole bf16 ulp then reaches the outputs.  Letting
every hidden element be an ulp off gives bounds of tens of output ulps.  `staged_reference` walks the stages and keeps, per hidden element, the
distance by which the kernel's rounded value can differ from the reference's (`flip_delta`): zero wherever both ends of the interval the
kernel's pre-rounding value lies in round to the same bf16 number -- almost everywhere -- and the distance between the two roundings otherwise.

    stage s:   z_s   = W_s (*) H_{s-1} + b_s [+ r_s]                 float64, on the reference's own rounded map H_{s-1}
               acc_s = |W_s| (*) |H_{s-1}| + |b_s| [+ |r_s|]
               D_s   = sqrt(k_s) ACC_EPS acc_s + |W_s| (*) d_{s-1}   the kernel's pre-rounding value is within D_s of z_s
               H_s   = rne_bf16(act(z_s)),  d_s = flip_delta(z_s, D_s, act)
    last:      ref = act(z), and `extra` = |W| (*) d_{last-1} goes to `bf16_bounds.check_bf16(..., acc64=acc, k=k, extra=extra)`, whose
               RNE-match and signed-bias statistics run over the outputs with extra <= ulp / 16

The order the kernel sums in does not enter.  No constant of its own: ACC_EPS, GELU_MAX_SLOPE and GELU_APPROX_ERR are those of `bf16_bounds`.
A plain module (tests/ is on sys.path while pytest runs), not a conftest.
"""
import math
from dataclasses import dataclass, field
from typing import List, Tuple, Union

import torch
import torch.nn.functional as F
from bf16_bounds import ACC_EPS, GELU_APPROX_ERR, GELU_MAX_SLOPE, half_ulp_bf16, rne_bf16


@dataclass
class Stage:
    """one convolution / linear layer of a fused launch, channels-last.  `w` [N, K]: K runs over (tap, channel) in the order `patches` lays the taps
    out -- (kh, kw, c) of a 2-D kernel, (tap, c) of a 1-D one.  `residual`: an operand of the output's shape, or a `Stage` applied to the input of
    the whole chain whose result the launch rounds to bf16 before it adds it (the downsample branch of a Bottleneck).  `pool`: a 3x3 / stride 2 /
    pad 1 max-pool behind the activation, before the rounding."""
    kind: str                                   # "conv2d" [B, H, W, C] | "conv1d" [B, T, C] | "linear" [M, C]
    w: torch.Tensor
    bias: torch.Tensor
    act: str = "none"                           # "none" | "relu" | "gelu"
    kh: int = 1
    kw: int = 1
    pad: Tuple[int, int] = (0, 0)
    taps: int = 1
    dil: int = 1
    residual: Union[None, torch.Tensor, "Stage"] = None
    pool: bool = False


@dataclass
class Hidden:
    """a map the launch rounds on chip: the reference's rounded values and how far the kernel's may be from them, per element"""
    value: torch.Tensor
    delta: torch.Tensor


@dataclass
class Fused:
    ref64: torch.Tensor
    acc64: torch.Tensor
    k: int
    extra: torch.Tensor
    hidden: List[Hidden] = field(default_factory=list)

    def selected_share(self):
        """share of the outputs whose `extra` is at most 1/16 ulp: the ones `check_bf16` takes its RNE-match and signed-bias statistics over"""
        return float((self.extra <= half_ulp_bf16(self.ref64) / 8).double().mean())


def zero_pad(x, st):
    """the input of `st` with the zero padding of its convolution"""
    if st.kind == "conv1d":
        p = st.dil * (st.taps - 1) // 2
        return F.pad(x, (0, 0, p, p))
    if st.kind == "conv2d":
        return F.pad(x, (0, 0, st.pad[1], st.pad[1], st.pad[0], st.pad[0]))
    return x


def patches(st, x, pad_fn=zero_pad):
    """im2col: [..., K] rows of the GEMM `st` is, K ordered as `Stage.w`.  `pad_fn` supplies the padded input (the CPU emulations of wrong
    kernels pad with something other than zeros)."""
    xp = pad_fn(x, st)
    if st.kind == "conv1d":
        t = x.shape[1]
        return torch.cat([xp[:, i * st.dil:i * st.dil + t] for i in range(st.taps)], -1)
    if st.kind == "conv2d":
        ho, wo = xp.shape[1] - st.kh + 1, xp.shape[2] - st.kw + 1
        return torch.cat([xp[:, i:i + ho, j:j + wo] for i in range(st.kh) for j in range(st.kw)], -1)
    assert st.kind == "linear"
    return xp


def pool3x3s2(x):
    """MaxPool2d(3, 2, 1) on [B, H, W, C]: the padding never wins (-inf)"""
    return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def act64(z, act):
    return {"none": lambda v: v, "relu": torch.relu, "gelu": gelu64}[act](z)


def flip_delta(z64, delta, act):
    """How far the kernel's rounded hidden value can be from `rne_bf16(act(z64))` when its pre-activation value is within `delta` of z64.
    The activation's value lies in [lo, hi]: act(z -+ delta) for the monotone none / relu; gelu(z) -+ (GELU_MAX_SLOPE delta + GELU_APPROX_ERR) for
    GELU (not monotone; its slope is at most GELU_MAX_SLOPE and the kernel's gelu_erf is GELU_APPROX_ERR from the exact one).  Rounding is
    monotone, so both the kernel's value and the reference's lie in [rne(lo), rne(hi)]: zero where those are equal (no flip possible, the kernel's
    value IS the reference's), their distance otherwise."""
    if act == "gelu":
        a = gelu64(z64)
        d = GELU_MAX_SLOPE * delta + GELU_APPROX_ERR
        lo, hi = a - d, a + d
    else:
        lo, hi = act64(z64 - delta, act), act64(z64 + delta, act)
    return rne_bf16(hi) - rne_bf16(lo)


def _terms(st, x_chain, h, delta):
    """(z, acc, prop, k) of one stage on the map h whose elements may be `delta` off"""
    w = st.w.to(torch.float64)
    b = st.bias.to(torch.float64)
    z = patches(st, h) @ w.T + b
    acc = patches(st, h.abs()) @ w.abs().T + b.abs()
    prop = patches(st, delta) @ w.abs().T
    k = w.shape[1] + 1
    if st.residual is not None:
        if isinstance(st.residual, Stage):
            r = round_stage(st.residual, x_chain, x_chain, torch.zeros_like(x_chain))
            rv, rd = r.value, r.delta
        else:
            rv = st.residual.to(torch.float64)
            rd = torch.zeros_like(rv)
        z, acc, prop, k = z + rv, acc + rv.abs(), prop + rd, k + 1
    return z, acc, prop, k


def round_stage(st, x_chain, h, delta):
    """a stage whose result the launch rounds to bf16 on chip -> Hidden"""
    z, acc, prop, k = _terms(st, x_chain, h, delta)
    d = flip_delta(z, math.sqrt(k) * ACC_EPS * acc + prop, st.act)
    v = rne_bf16(act64(z, st.act))
    if st.pool:
        v, d = pool3x3s2(v), pool3x3s2(d)      # |max a - max b| <= max |a - b|
    return Hidden(v, d)


def staged_reference(x, stages) -> Fused:
    """Walk `stages` from the bf16 operand `x`.  Every stage but the last is rounded on chip; the last is the launch's output, rounded once at the
    store.  Returns the output's (ref64, acc64, k, extra) for `check_bf16(..., single_rounding=True)` and the reference's hidden maps."""
    x = x.to(torch.float64)
    cur = Hidden(x, torch.zeros_like(x))
    hidden = []
    for st in stages[:-1]:
        cur = round_stage(st, x, cur.value, cur.delta)
        hidden.append(cur)
    st = stages[-1]
    z, acc, extra, k = _terms(st, x, cur.value, cur.delta)
    ref = act64(z, st.act)
    if st.act == "gelu":
        acc, extra = GELU_MAX_SLOPE * acc, GELU_MAX_SLOPE * extra + GELU_APPROX_ERR
    if st.pool:
        # rounding is monotone, rne(max) = max(rne): pooling the rounded map and rounding the pooled one store the same; the error of a max is at
        # most the largest error in its window
        ref, acc, extra = pool3x3s2(ref), pool3x3s2(acc), pool3x3s2(extra)
    return Fused(ref, acc, k, extra, hidden)


def stored_stage(st, x, h_stored) -> Fused:
    """a stage that reads a map the launch STORED (chain_gemm's y1, `bottleneck_fused_next`'s y at the even pixels, a TCN layer's h): the plain
    single-rounding bound on the kernel's own stored values, nothing to propagate.  x: the input of the whole chain."""
    h = h_stored.to(torch.float64)
    z, acc, prop, k = _terms(st, x.to(torch.float64), h, torch.zeros_like(h))
    assert not st.pool
    return Fused(act64(z, st.act), acc, k, prop, [])


# ------------------------------------------------------------------------------------------------------- operands shared by the CPU and GPU tests
IMAGE_SCALE = (1.0, 3.0, 0.5)


def ring_image(shape, gen, ring=64.0):
    """randn [B, H, W, C] (or [B, T, C]) as bf16 values: the outermost ring of pixels (frames) `ring` x the interior and consecutive images scaled
    1 / 3 / 0.5, so a clamped halo value that reaches zero padding, or a pixel of the neighbouring image, moves a result far beyond rounding"""
    x = torch.randn(shape, generator=gen)
    m = torch.zeros(shape[1:-1])
    if m.dim() == 2:
        m[0], m[-1], m[:, 0], m[:, -1] = 1, 1, 1, 1
    else:
        m[0], m[-1] = 1, 1
    x = x * (1 + (ring - 1) * m)[None, ..., None]
    x = x * torch.tensor([IMAGE_SCALE[i % 3] for i in range(shape[0])]).view((-1,) + (1,) * (len(shape) - 1))
    return x.bfloat16().float()


def distinct_biases(sizes):
    """fp32 vectors of the given sizes, every value of every vector different from every other (multiples of 1 / 512), none zero, signs mixed"""
    n = torch.arange(1, sum(sizes) + 1, dtype=torch.float32)
    v = n / 512 * torch.where(n.long() % 3 == 0, -1.0, 1.0)
    return [t.contiguous() for t in v.split(list(sizes))]


def conv_weight(gen, cout, cin, kh, kw, scale):
    """OIHW fp32 weights holding bf16 values (packing them to bf16 on the device is then exact) and the same as the [N, K] matrix of a `Stage`"""
    w = (torch.randn((cout, cin, kh, kw), generator=gen) * scale).bfloat16().float()
    return w, w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()


# ------------------------------------------------------------------------------------------------------------ the stage lists of the six launches
def bottleneck_stages(x, c1, c2, c3, ds=None, nxt=None):
    """`mt4_bottleneck_fused_bf16` (identity: residual x; downsample: residual = the rounded 1x1 branch `ds`) and, with `nxt`, the conv1 of the
    following block that `mt4_bottleneck_fused_next_bf16` runs on the block's rounded output.  c* = ([N, K] matrix, bias)."""
    res = Stage("conv2d", ds[0], ds[1]) if ds is not None else x
    st = [Stage("conv2d", c1[0], c1[1], "relu"), Stage("conv2d", c2[0], c2[1], "relu", kh=3, kw=3, pad=(1, 1)),
          Stage("conv2d", c3[0], c3[1], "relu", residual=res)]
    return st + ([Stage("conv2d", nxt[0], nxt[1], "relu")] if nxt is not None else [])


def next_reference(x, stages, y_even):
    """t of `bottleneck_fused_next`: at the even pixels the launch stored the map conv1 reads (y_even), so there the plain single-rounding bound on
    the kernel's own y_even holds; everywhere else the map existed on chip only and the bound comes by propagation"""
    f = staged_reference(x, stages)
    e = stored_stage(stages[-1], x, y_even)
    f.ref64[:, ::2, ::2], f.acc64[:, ::2, ::2], f.extra[:, ::2, ::2] = e.ref64, e.acc64, 0.0
    return f


def chain_stages(w1, b1, w2, b2, r1=None, r2=None):
    """`mt4_chain_gemm_bf16`: Bottleneck form (r1: relu(x W1 + b1 + r1) is STORED, then relu(. W2 + b2)) or MLP form (r2: gelu stays on chip)"""
    if r1 is not None:
        return [Stage("linear", w1, b1, "relu", residual=r1), Stage("linear", w2, b2, "relu")]
    return [Stage("linear", w1, b1, "gelu"), Stage("linear", w2, b2, "none", residual=r2)]


def expand_stages(c2, c3, residual):
    """`ops.conv3x3_expand`: conv2 3x3 + ReLU on chip, conv3 1x1 + residual + ReLU"""
    return [Stage("conv2d", c2[0], c2[1], "relu", kh=3, kw=3, pad=(1, 1)), Stage("conv2d", c3[0], c3[1], "relu", residual=residual)]


def stem_stages(w, bias):
    """`mt4_stem_maxpool_bf16` on the space-to-depth frame [B, Hs, Ws, 16]: the 7x7 / 2 stem is a 4x4 convolution there; ReLU; 3x3 / 2 max-pool;
    one rounding"""
    return [Stage("conv2d", w, bias, "relu", kh=4, kw=4, pool=True)]


def tcn_stages(x, w1, b1, w2, b2, dil):
    """`mt4_tcn_layer_fused_bf16`: relu(dilated 3-tap conv) on chip, 1x1 conv + x"""
    return [Stage("conv1d", w1, b1, "relu", taps=3, dil=dil), Stage("conv1d", w2, b2, "none", residual=x)]


def check_fused(got, f: Fused, what, sl=None):
    """`check_bf16` of a launch's output against its staged reference (`sl`: an index into both, e.g. the even pixels).  The share of outputs the
    RNE statistics were taken over goes to the log beside the check's own line."""
    from bf16_bounds import _log, check_bf16
    ref, acc, extra = (f.ref64, f.acc64, f.extra) if sl is None else (f.ref64[sl], f.acc64[sl], f.extra[sl])
    st = check_bf16(got, ref, acc64=acc, k=f.k, extra=extra, single_rounding=True, what=what)
    st["selected"] = Fused(ref, acc, f.k, extra).selected_share()
    _log(dict(what=what, kind="selected", share=st["selected"]))
    return st
