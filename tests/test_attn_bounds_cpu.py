"""CPU: the per-element bounds the GPU tests of the attention cores and of LayerNorm apply (`attn_checks`) accept a torch emulation of a correct
kernel on the operands of one probe row per family, and reject emulations of the ways such kernels go wrong at a ragged edge.

The correct emulation accumulates in fp32 and rounds once at the store; for the matrix-unit bf16 kernels it rounds q * scale and the unnormalised
probabilities to bf16 as they do, with the normaliser the fp32 sum of the unrounded ones.  The wrong ones:
  - the last key dropped (a chunk or tile loop that stops one short);
  - a padded key admitted with score 0 and a zero V row (a key tile's padding not set to -inf);
  - the padded head dims left non-zero: q, K and V slices read past hd into the next head's dims, as a kernel without the `d < hd` guards would.
    (V's padded dims alone never reach a stored element in any of the cores -- their outputs are not stored; it is the q and K side that does);
  - LayerNorm: the mean taken over the padded chunk count of the kernel instead of N;
  - LayerNorm: a one-pass variance E[x^2] - E[x]^2 on rows with mean / std ~ 100."""
import attn_checks as ac
import attn_variants as av
import pytest
import torch


def _row(table, **kw):
    return next(p for p in table if all(p[k] == v for k, v in kw.items()))


# one row per family; the bf16 matrix-unit rows with few keys: one key more or less must show through the 2^-8 allowed to the bf16 probabilities
ROWS = {
    "generic fp32 a": (_row(av.GENERIC_PROBES, dt=av.F32, variant=(28, 4), bias=True), False),
    "generic fp32 b": (_row(av.GENERIC_PROBES, dt=av.F32, variant=(28, 4), bias=False), False),
    "generic bf16 a": (_row(av.GENERIC_PROBES, dt=av.BF16, variant=(64, 8), bias=True), False),
    "generic bf16 b": (_row(av.GENERIC_PROBES, dt=av.BF16, variant=(24, 2), bias=False), False),
    "bf16 MFMA": (_row(av.MHA_BF16_PROBES, variant=(1, 256)), True),
    "fp32 MFMA": (_row(av.MHA_F32_PROBES, variant=(8, 4), Nk=128), False),
    "fp32 MFMA, no split": (_row(av.MHA_F32_PROBES, variant=(16, 1), Nk=129), False),
}


def _emulate(p, mfma, *, drop_last=False, pad_key=False, pad_dims=0, amp=2.0):
    """[B Nq, H hd] in the row's dtype; (q, k, v, bias, mask) are returned with it for the check"""
    q, kv, bias, mask = ac.attn_inputs(p, amp)
    qh, kh, vh = ac.attn_heads(p, q, kv)
    scale = p["hd"] ** -0.5
    qf, kf, vf = qh.float(), kh.float(), vh.float()
    if pad_dims:      # every head's slices run pad_dims into the next head
        qf, kf, vf = [torch.cat([t, t.roll(-1, dims=1)[..., :pad_dims]], -1) for t in (qf, kf, vf)]
    qs = qf * torch.tensor(scale, dtype=torch.float32)
    if mfma:
        qs = qs.bfloat16().float()
    s = qs @ kf.transpose(-1, -2)
    if bias is not None:
        s = s + bias.unsqueeze(0)
    if mask is not None:
        s = (s.view(p["B"] // p["nw"], p["nw"], *s.shape[1:]) + mask.unsqueeze(1).unsqueeze(0)).view(*s.shape)
    if drop_last:
        s, vf = s[..., :-1], vf[..., :-1, :]
    if pad_key:
        s, vf = torch.cat([s, torch.zeros_like(s[..., :1])], -1), torch.cat([vf, torch.zeros_like(vf[..., :1, :])], -2)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    o = ((e.bfloat16().float() if mfma else e) @ vf) / e.sum(-1, keepdim=True)
    o = o[..., :p["hd"]].permute(0, 2, 1, 3).reshape(p["B"] * p["Nq"], p["H"] * p["hd"]).to(q.dtype)
    return o, qh, kh, vh, scale, bias, mask


def _check(p, mfma, o, qh, kh, vh, scale, bias, mask, what):
    if p["dt"] == av.BF16:
        ac.check_attn_bf16(o, qh, kh, vh, scale, bias, mask, p["nw"], mfma=mfma, what=what)
    else:
        ac.check_attn_f32(o, qh, kh, vh, scale, bias, mask, p["nw"], what=what)


@pytest.mark.parametrize("name", list(ROWS))
def test_attention_correct_emulation_passes(name):
    p, mfma = ROWS[name]
    _check(p, mfma, *_emulate(p, mfma), what=name)


def test_store_rounding_across_a_binade_edge():
    """mha_mfma_kernel<8, 256>, 125 keys, scale 1, output (40, 185): float64 gives 0.24989, the bf16 rounding of P (allowed: 2^-8 sum p |v|) puts the fp32
    result at 0.25103, which the store rounds to 0.25 + 2^-9 -- half an ulp of [0.25, 0.5), twice that of the reference's binade.  The MI355X stores the
    same value; the bound takes the half ulp at |ref| + slack and accepts it (0.83), the half ulp of the reference's own binade did not (1.04)"""
    p = _row(av.MHA_BF16_PROBES, variant=(8, 256), Nk=125)
    q, kv, _, _ = ac.attn_inputs(p, 1.0)
    qh, kh, vh = ac.attn_heads(p, q, kv)
    s = qh.float() @ kh.float().transpose(-1, -2)                  # (scale 1: q * scale is q, already bf16)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    o = ((e.bfloat16().float() @ vh.float()) / e.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(p["B"] * p["Nq"], -1)
    assert 0.2510 < o[40, 185].item() < 0.2511 and o[40, 185].bfloat16().item() == 0.25 + 2.0 ** -9
    ac.check_attn_bf16(o.bfloat16(), qh, kh, vh, 1.0, None, None, 0, mfma=True, what="binade edge")
    t = ac._attn_terms(qh, kh, vh, 1.0, None, None, 0, mfma=True)
    assert 0.2498 < t["flat"](t["o"])[40, 185].item() < 0.25


@pytest.mark.parametrize("bug", ["drop_last", "pad_key"])
@pytest.mark.parametrize("name", [n for n in ROWS if not n.endswith(" b")])
def test_attention_wrong_key_count_rejected(name, bug):
    p, mfma = ROWS[name]
    with pytest.raises(AssertionError, match="bound exceeded"):
        _check(p, mfma, *_emulate(p, mfma, **{bug: True}), what=f"{name}, {bug}")


@pytest.mark.parametrize("name", ["generic fp32 b", "generic bf16 b"])
def test_attention_nonzero_padded_head_dims_rejected(name):
    p, mfma = ROWS[name]
    dpl, lpq = p["variant"]
    assert dpl * lpq > p["hd"]
    with pytest.raises(AssertionError, match="bound exceeded"):
        _check(p, mfma, *_emulate(p, mfma, pad_dims=dpl * lpq - p["hd"]), what=f"{name}, padded head dims")


def _window(n, nw, **bug):
    """the window core on the operands of the probe (n, nw): the matrix-unit emulation over [B, H, n, 32]"""
    B, H = av.WINDOW_B, av.WINDOW_H
    qkv, bias, mask = ac.window_inputs(n, nw, B, H)
    c = H * 32
    qh, kh, vh = [ac.split_heads(qkv[:, i * c:(i + 1) * c], B, n, H, 32) for i in range(3)]
    scale = 32 ** -0.5
    s = (qh.float() * torch.tensor(scale, dtype=torch.float32)).bfloat16().float() @ kh.float().transpose(-1, -2) + bias.unsqueeze(0)
    if mask is not None:
        s = (s.view(B // nw, nw, H, n, n) + mask.unsqueeze(1).unsqueeze(0)).view(B, H, n, n)
    vf = vh.float()
    if bug.get("drop_last"):
        s, vf = s[..., :-1], vf[..., :-1, :]
    if bug.get("pad_key"):
        s, vf = torch.cat([s, torch.zeros_like(s[..., :1])], -1), torch.cat([vf, torch.zeros_like(vf[..., :1, :])], -2)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    o = ((e.bfloat16().float() @ vf) / e.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(B * n, c).bfloat16()
    ac.check_attn_bf16(o, qh, kh, vh, scale, bias, mask, nw, mfma=True, what=f"window {n} {bug}")


def test_window_emulations():
    n, nw = av.WINDOW_PROBES[0]
    _window(n, nw)
    _window(*av.WINDOW_PROBES[2])
    for bug in ("drop_last", "pad_key"):
        with pytest.raises(AssertionError, match="bound exceeded"):
            _window(n, nw, **{bug: True})


def _ln(x, g, b, *, npad=None, one_pass=False):
    """fp32 LayerNorm the way the kernels compute it (row sum, then the squared deviations from that mean), stored with one rounding"""
    xf = x.float()
    n = xf.shape[-1]
    mean = xf.sum(-1, keepdim=True) / (npad or n)
    if one_pass:
        var = (xf * xf).sum(-1, keepdim=True) / n - mean * mean
    else:
        var = ((xf - mean) ** 2).sum(-1, keepdim=True) / n
    return ((xf - mean) * torch.rsqrt(var + 1e-5) * g + b).to(x.dtype)


@pytest.mark.parametrize("dt,m,c", [(av.F32, 7, 4 * 33), (av.BF16, 7, 8 * 33), (av.F32, 37, 4 * 17), (av.BF16, 37, 8 * 513)])
def test_layernorm_emulations(dt, m, c):
    assert (dt, m, c, 1) in av.LN_PROBES
    x, g, b, xo = ac.ln_inputs(dt, m, c)
    ac.check_ln(_ln(x, g, b), x, g, b, what="correct")
    ac.check_ln(_ln(xo, g, b), xo, g, b, what="correct, mean/std ~ 100")
    kind, width = av.ln_kernel(dt, 1, c)
    npad = (width if kind == "narrow" else 64 * width) * av.LN_V[dt]       # the chunks the kernel's lanes span, in elements
    assert npad > c
    with pytest.raises(AssertionError, match="bound exceeded"):
        ac.check_ln(_ln(x, g, b, npad=npad), x, g, b, what="mean over the padded chunks")
    with pytest.raises(AssertionError, match="bound exceeded"):
        ac.check_ln(_ln(xo, g, b, one_pass=True), xo, g, b, what="one-pass variance")
