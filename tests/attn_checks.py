"""float64 references and per-element bounds of the attention cores and of LayerNorm, shared by the GPU tests of the transformer kernels
(test_gpu_transformer_kernels.py, test_gpu_attention_variants.py) and the CPU test that shows they reject wrong kernels (test_attn_bounds_cpu.py).

This is a plain module beside `bf16_bounds.py` (`tests/` is on sys.path while pytest runs), not a conftest."""
import torch
from bf16_bounds import FAST_EXP, check_bf16, check_f32, rne_bf16


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def ln64(x64, g, b, eps=1e-5):
    """float64 LayerNorm over the last dim and its accumulation scale: `layernorm_kernel` (transformer_kernels.hip:38-84) sums the row in fp32,
    then the squared deviations from that mean (two passes), and stores (x - mean) * rstd * gamma + beta with one rounding.  The fp32 error of
    the mean reaches the output as |gamma| rstd mean|x|, that of rstd as |gamma x_hat|."""
    mu = x64.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(((x64 - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x64 - mu) * r
    g64, b64 = g.double(), b.double()
    return xh * g64 + b64, g64.abs() * (xh.abs() + r * x64.abs().mean(-1, keepdim=True)) + b64.abs()


def _attn_terms(q, k, v, scale, bias, mask, nw, *, mfma, region=False):
    """float64 attention on q / k / v [B,H,N,hd] (bias [H,Nq,Nk], mask [nW,Nq,Nk]) and the sizes its errors scale with; see `check_attn_bf16`"""
    q64, k64, v64 = q.double(), k.double(), v.double()
    qs = rne_bf16(q.float() * scale) if mfma else q64 * scale
    s = qs @ k64.transpose(-1, -2)
    sa = qs.abs() @ k64.abs().transpose(-1, -2)
    if bias is not None:
        s, sa = s + bias.double().unsqueeze(0), sa + bias.double().abs().unsqueeze(0)
    if mask is not None:
        b = q.shape[0]
        m64 = mask.double().unsqueeze(1).unsqueeze(0)
        s = (s.view(b // nw, nw, *s.shape[1:]) + m64).view(*s.shape)
        sa = (sa.view(b // nw, nw, *sa.shape[1:]) + m64.abs()).view(*sa.shape)
    if region:
        sa = sa + 100.0
    sa = sa + sa.amax(-1, keepdim=True)
    p = torch.softmax(s, -1)
    o = p @ v64
    pv = p @ v64.abs()
    acc = pv + (p * sa) @ v64.abs() + (p * sa).sum(-1, keepdim=True) * o.abs()
    B, H, N, hd = o.shape
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, H * hd)
    return dict(s=s, p=p, o=o, pv=pv, acc=acc, v64=v64, flat=flat, k=max(k.shape[2], hd))


def check_attn_bf16(out, q, k, v, scale, bias, mask, nw, *, mfma, region=False, what=""):
    """`out` [B*N, H*hd] of a bf16 attention core against float64 on the same bf16 q / k / v ([B,H,N,hd]).

    mfma: the matrix-unit kernels (mha_mfma_kernel, window_attention_mfma_kernel) multiply Q by the scale in fp32 and round it to bf16 before
    the score MFMA (transformer_kernels.hip:344,1176) -- the reference rounds it there too; they round the unnormalised probabilities
    p_j = exp(s_j - max) to bf16 as the B operand of the P.V MFMA while the normaliser is the fp32 sum of the unrounded p_j, and scale the fp32
    result by 1 / sum before the one rounding of the store (:403-458, :1302-1337).  That P rounding is not emulated: it adds at most
    2^-9 * sum_j p_j |v_j| per output, and the bound allows 2^-8 of it.  The generic kernel (attention_kernel, :179-307) keeps q * scale and P in
    fp32 (online softmax, one rounding at the store): single rounding.
    The fp32 score error (a dot product of hd terms, the bias / mask added, exp2 of s * log2 e - max * log2 e) reaches an output as
    sum_j p_j |ds_j| (|v_j| + |o|): in the accumulation term with sum_d |q_d k_d| + |bias| + |mask| (+ 100 on the region form, which adds 100
    where the regions are equal) + the row's largest such sum as the size of ds_j."""
    t = _attn_terms(q, k, v, scale, bias, mask, nw, mfma=mfma, region=region)
    flat = t["flat"]
    check_bf16(out.cpu(), flat(t["o"]), acc64=flat(t["acc"]), k=t["k"], extra=flat(t["pv"]) * 2.0 ** -8 if mfma else 0.0, single_rounding=not mfma, what=what)


def attn_f32_bound(q, k, v, scale, bias, mask, nw):
    """(ref64, acc64, k, extra), each [B*Nq, H*hd], of an fp32 attention core on fp32 q / k / v ([B,H,N,hd]) for `check_f32`: the float64 result with
    the fp32 value of `scale` (the kernels take a float) and q * scale unrounded -- every fp32 core keeps it in fp32, one rounding among the hd of the
    score's dot product --; the accumulation term of `check_attn_bf16` (k = max(Nk, hd)); and for the hardware exponential
    extra = sum_j p_j FAST_EXP(x_j) (|v_j| + |o|), x_j = s_j - max_j s: a relative error e_j of p_j moves the output by p_j e_j (v_j - o)."""
    scale = float(torch.tensor(scale, dtype=torch.float32))
    t = _attn_terms(q, k, v, scale, bias, mask, nw, mfma=False)
    w = t["p"] * FAST_EXP(t["s"] - t["s"].amax(-1, keepdim=True))
    extra = w @ t["v64"].abs() + w.sum(-1, keepdim=True) * t["o"].abs()
    flat = t["flat"]
    return flat(t["o"]), flat(t["acc"]), t["k"], flat(extra)


def check_attn_f32(out, q, k, v, scale, bias, mask, nw, *, what=""):
    """`out` [B*N, H*hd] of an fp32 attention core (attention_kernel<float>, mha_mfma_f32_kernel) against float64 on the same operands, per element"""
    ref64, acc64, kk, extra = attn_f32_bound(q, k, v, scale, bias, mask, nw)
    return check_f32(out.cpu(), ref64, acc64=acc64, k=kk, extra=extra, what=what)


def split_heads(t, B, N, H, hd):
    """rows [B N, H hd] -> [B, H, N, hd]"""
    return t.reshape(B, N, H, hd).permute(0, 2, 1, 3)


# ---- the operands of a probe row of `attn_variants`, the same on the GPU and in the CPU emulations
def attn_inputs(p, amp=2.0):
    """q rows [B Nq, H hd], kv rows [B Nk, 2 H hd] (k | v) in the row's dtype, the fp32 bias [H, Nq, Nk] and -100 / 0 mask [nW, Nq, Nk] (or None)"""
    dtype = torch.bfloat16 if p["dt"] == 1 else torch.float32
    c = p["H"] * p["hd"]
    q = rand((p["B"] * p["Nq"], c), 11, amp).to(dtype)
    kv = rand((p["B"] * p["Nk"], 2 * c), 12, amp).to(dtype)
    bias = rand((p["H"], p["Nq"], p["Nk"]), 13) if p["bias"] else None
    mask = torch.where(rand((p["nw"], p["Nq"], p["Nk"]), 14) > 0.3, torch.tensor(-100.0), torch.tensor(0.0)).contiguous() if p["nw"] else None
    return q, kv, bias, mask


def attn_heads(p, q, kv):
    """q, k, v as [B, H, N, hd] views of the rows of `attn_inputs`"""
    c = p["H"] * p["hd"]
    return (split_heads(q, p["B"], p["Nq"], p["H"], p["hd"]), split_heads(kv[:, :c], p["B"], p["Nk"], p["H"], p["hd"]),
            split_heads(kv[:, c:], p["B"], p["Nk"], p["H"], p["hd"]))


def window_inputs(n, nw, B, H):
    """packed qkv rows [B n, 3 H 32] (bf16), bias [H, n, n], mask [nw, n, n] or None of a window probe"""
    qkv = rand((B * n, 3 * H * 32), 61, 2.0).to(torch.bfloat16)
    bias = rand((H, n, n), 62)
    mask = torch.where(rand((nw, n, n), 63) > 0.3, torch.tensor(-100.0), torch.tensor(0.0)).contiguous() if nw else None
    return qkv, bias, mask


def ln_inputs(dt, m, c):
    """x [m, c] in the row's dtype, fp32 gamma and beta, and rows with mean / std ~ 100 (a one-pass E[x^2] - E[x]^2 variance loses
    ~2^-24 * 100^2 * sqrt(C) of it; the two-pass kernels do not)"""
    dtype = torch.bfloat16 if dt == 1 else torch.float32
    return rand((m, c), 1, 3.0).to(dtype), rand((c,), 2) + 1.5, rand((c,), 3), (rand((m, c), 4) + 60.0).to(dtype)


def check_ln(got, x, g, b, *, what=""):
    """LayerNorm output (bf16 or fp32, rows [m, C]) against float64 on the same x, per element; k = the row length"""
    ref64, acc64 = ln64(x.double(), g, b)
    chk = check_bf16 if got.dtype == torch.bfloat16 else check_f32
    return chk(got.cpu(), ref64, acc64=acc64, k=x.shape[-1], what=what)
