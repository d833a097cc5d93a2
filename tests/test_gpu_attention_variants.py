"""GPU: every launchable instantiation of the attention cores and of LayerNorm (the variant lists of csrc/transformer_kernels.hip), each on the
smallest shapes that reach its ragged edges, every output element against float64 on the same operands.

The rows are the probe tables of `attn_variants`; test_variant_probes_cpu.py shows without a GPU that they reach every variant.  Each test first
asks the library (`mt4_attention_plan`), or the mirrored rule, that its row gets the variant it names.  The bounds are those of `attn_checks`
(bf16: half a bf16 ulp + the fp32 accumulation term; fp32: half an fp32 ulp + the same term + the hardware exponential's allowance);
test_attn_bounds_cpu.py shows that they reject a dropped key, an admitted padded key and non-zero padded head dims."""
import attn_checks as ac
import attn_variants as av
import pytest
import torch

pytestmark = pytest.mark.gpu
DTN = {av.F32: "f32", av.BF16: "bf16"}


def _id(p):
    return f"{DTN[p['dt']]}-{p['variant'][0]}_{p['variant'][1]}-B{p['B']}H{p['H']}-q{p['Nq']}k{p['Nk']}-hd{p['hd']}"


def _attention(cuda, p, q, kv, bias, mask, scale):
    from computervision_codes_amd import ops
    c = p["H"] * p["hd"]
    kvd = kv.to(cuda)
    return ops.attention(q.to(cuda), kvd[:, :c], kvd[:, c:], batch=p["B"], heads=p["H"], nq=p["Nq"], nk=p["Nk"], hd=p["hd"], q_stride=c, k_stride=2 * c,
                         v_stride=2 * c, scale=scale, bias=bias.to(cuda) if bias is not None else None, mask=mask.to(cuda) if mask is not None else None)


@pytest.mark.parametrize("p", av.GENERIC_PROBES, ids=_id)
def test_generic_attention_variant(cuda, p):
    """attention_kernel<T, DPL, LPQ>: row a -- the whole slice width, vector staging, bias + mask, two LDS chunks with a ragged last group of keys;
    row b -- hd % 4 != 0: element-wise staging and zero-padded head dims.  q * scale and P stay in fp32, one rounding at the store"""
    assert av.probe_plan(p) == (av.GENERIC,) + p["variant"]
    q, kv, bias, mask = ac.attn_inputs(p)
    scale = p["hd"] ** -0.5
    out = _attention(cuda, p, q, kv, bias, mask, scale)
    what = f"generic {DTN[p['dt']]} {_id(p)}"
    if p["dt"] == av.BF16:
        ac.check_attn_bf16(out, *ac.attn_heads(p, q, kv), scale, bias, mask, p["nw"], mfma=False, what=what)
    else:
        ac.check_attn_f32(out, *ac.attn_heads(p, q, kv), scale, bias, mask, p["nw"], what=what)


@pytest.mark.parametrize("p", av.MHA_BF16_PROBES, ids=_id)
def test_mha_mfma_bf16_variant(cuda, p):
    """mha_mfma_kernel<NKT, HD>: a ragged second query workgroup, a ragged last key tile (or a full one), and for odd NKT a zero upper half of the last
    32-key block of P and V; with scale hd^-0.5 and with scale 1 (a few keys dominate: the probabilities' bf16 rounding shows most)"""
    assert av.probe_plan(p) == (av.MFMA_BF16,) + p["variant"]
    q, kv, _, _ = ac.attn_inputs(p, 1.0)
    for scale in (p["hd"] ** -0.5, 1.0):
        out = _attention(cuda, p, q, kv, None, None, scale)
        ac.check_attn_bf16(out, *ac.attn_heads(p, q, kv), scale, None, None, 0, mfma=True, what=f"mha bf16 {_id(p)} scale {scale:.3g}")


@pytest.mark.parametrize("p", av.MHA_F32_PROBES, ids=_id)
def test_mha_mfma_f32_variant(cuda, p):
    """mha_mfma_f32_kernel<NKT, KSPLIT>: one wave per 16 queries and the keys split over four; one key, full and ragged key tiles, head dims of one
    4-vector, of a ragged last 32-dim chunk (108) and the widest (128)"""
    assert av.probe_plan(p) == (av.MFMA_F32,) + p["variant"]
    q, kv, _, _ = ac.attn_inputs(p, 1.5)
    scale = p["hd"] ** -0.5
    out = _attention(cuda, p, q, kv, None, None, scale)
    ac.check_attn_f32(out, *ac.attn_heads(p, q, kv), scale, None, None, 0, what=f"mha f32 {_id(p)}")


@pytest.mark.parametrize("n,nw", av.WINDOW_PROBES, ids=lambda v: str(v))
def test_window_attention_variant(cuda, n, nw):
    """window_attention_mfma_kernel<NT, NW> on expanded bias (+ mask) tables: every tile count, a ragged last tile (staging rows past N stay zero,
    padded keys take -1e30 from the padded tables, queries past N are not stored) and two full ones"""
    from computervision_codes_amd import ops
    B, H = av.WINDOW_B, av.WINDOW_H
    assert (av.window_nt(n), 3 if av.window_nt(n) == 9 else 4) in av.WINDOW
    qkv, bias, mask = ac.window_inputs(n, nw, B, H)
    c = H * 32
    scale = 32 ** -0.5
    d = qkv.to(cuda)
    out = ops.window_attention_bf16(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], batch=B, heads=H, n=n, q_stride=3 * c, k_stride=3 * c, v_stride=3 * c, scale=scale,
                                    bias_padded=ops.pad_attention_bias(bias.to(cuda)),
                                    mask_padded=ops.pad_attention_bias(mask.to(cuda), 0.0) if mask is not None else None)
    q, k, v = [ac.split_heads(qkv[:, i * c:(i + 1) * c], B, n, H, 32) for i in range(3)]
    ac.check_attn_bf16(out, q, k, v, scale, bias, mask, nw, mfma=True, what=f"window N={n} NT={av.window_nt(n)} nW={nw}")


@pytest.mark.parametrize("ws,H,res,shift", av.WINDOW_REL_PROBES[5:], ids=lambda v: str(v))
def test_window_attention_rel_variant(cuda, ws, H, res, shift):
    """the table / region-id form at every window size it accepts (the shapes of test_window_attention_from_relative_table_equals_expanded_tables
    run there): bit equality with the expanded form on unshifted blocks, the float64 bound on shifted ones (+100 where the regions are equal)"""
    from computervision_codes_amd import ops
    from computervision_codes_amd.spatial_transformer import _rel_pos_index, _shift_mask, _shift_regions
    N, nwin = ws * ws, (res // ws) ** 2
    B = 2 * nwin
    c = H * 32
    qkv = ac.rand((B * N, 3 * c), 71, 2.0).to(torch.bfloat16)
    d = qkv.to(cuda)
    table = ac.rand(((2 * ws - 1) ** 2, H), 72)
    bias = table[_rel_pos_index(ws).view(-1)].view(N, N, H).permute(2, 0, 1).contiguous()
    mask = _shift_mask(res, ws, shift) if shift else None
    scale = 32 ** -0.5
    kw = dict(batch=B, heads=H, q_stride=3 * c, k_stride=3 * c, v_stride=3 * c, scale=scale)
    got = ops.window_attention_rel_bf16(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], ws=ws, rel_table=table.t().contiguous().to(cuda),
                                        region=_shift_regions(res, ws, shift).to(torch.int32).to(cuda) if shift else None, **kw)
    q, k, v = [ac.split_heads(qkv[:, i * c:(i + 1) * c], B, N, H, 32) for i in range(3)]
    ac.check_attn_bf16(got, q, k, v, scale, bias, mask, nwin, mfma=True, region=bool(shift), what=f"window rel ws={ws} NT={av.window_nt(N)} shift={shift}")
    if not shift:
        ref = ops.window_attention_bf16(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], n=N, bias_padded=ops.pad_attention_bias(bias.to(cuda)), mask_padded=None, **kw)
        assert torch.equal(got, ref)


@pytest.mark.parametrize("nch", av.LN_NCH)
@pytest.mark.parametrize("dt", [av.F32, av.BF16], ids=["f32", "bf16"])
def test_layernorm_variant(cuda, dt, nch):
    """every LayerNorm kernel at the two ends of its chunk range, on row counts ragged against the rows of a workgroup; also rows with
    mean / std ~ 100.  Two-pass fp32 mean / variance, one rounding at the store"""
    from computervision_codes_amd import ops
    c = nch * av.LN_V[dt]
    kern = av.ln_kernel(dt, 1, c)
    assert kern is not None
    for m in av.LN_ROWS:
        assert (dt, m, c, 1) in av.LN_PROBES
        x, g, b, xo = ac.ln_inputs(dt, m, c)
        ac.check_ln(ops.layernorm(x.to(cuda), g.to(cuda), b.to(cuda)), x, g, b, what=f"layernorm {DTN[dt]} {kern} nch={nch} M={m}")
        ac.check_ln(ops.layernorm(xo.to(cuda), g.to(cuda), b.to(cuda)), xo, g, b, what=f"layernorm {DTN[dt]} {kern} nch={nch} M={m}, mean/std ~ 100")


@pytest.mark.parametrize("dt,b,res,c", av.LN_MERGE_PROBES, ids=lambda v: str(v))
def test_layernorm_patch_merging_gather_wide(cuda, dt, b, res, c):
    """the G = 4 gather of PatchMerging on the wide kernels (bf16 4 C = 2048: Swin-B's last merge, wide<4>; fp32 4 C = 512: wide<2>)"""
    from computervision_codes_amd import ops
    from computervision_codes_amd.spatial_transformer import _merge_row_map
    assert av.ln_kernel(dt, 4, c) == ("wide", 4 if dt == av.BF16 else 2)
    x, g, be, _ = ac.ln_inputs(dt, b * res * res, c)
    g, be = ac.rand((4 * c,), 9) + 1.5, ac.rand((4 * c,), 10)
    got = ops.layernorm(x.to(cuda), g.to(cuda), be.to(cuda), row_map=_merge_row_map(res).to(cuda), group=4, l_out=(res // 2) ** 2, l_in=res * res,
                        m_out=b * (res // 2) ** 2)
    xv = x.view(b, res, res, c)
    cat = torch.cat([xv[:, 0::2, 0::2], xv[:, 1::2, 0::2], xv[:, 0::2, 1::2], xv[:, 1::2, 1::2]], -1).reshape(-1, 4 * c)
    ac.check_ln(got, cat, g, be, what=f"layernorm {DTN[dt]} patch-merging gather 4C={4 * c}")


@pytest.mark.parametrize("dt,b,res,ws,shift,c", av.LN_WINDOW_PROBES, ids=lambda v: str(v))
def test_layernorm_window_gather_wide(cuda, dt, b, res, ws, shift, c):
    """the shifted-window row gather on a wide kernel (the gather moves rows; the arithmetic is that of the plain form)"""
    from computervision_codes_amd import ops
    from computervision_codes_amd.spatial_transformer import _window_row_map
    from oracle.swin_q2l import window_partition
    assert av.ln_kernel(dt, 1, c) == ("wide", 2)
    x, g, be, _ = ac.ln_inputs(dt, b * res * res, c)
    rm = _window_row_map(res, ws, shift)
    got = ops.layernorm(x.to(cuda), g.to(cuda), be.to(cuda), row_map=rm.to(cuda), group=1, l_out=res * res, l_in=res * res)
    xw = window_partition(torch.roll(x.view(b, res, res, c), shifts=(-shift, -shift), dims=(1, 2)), ws).reshape(-1, c)
    ac.check_ln(got, xw, g, be, what=f"layernorm {DTN[dt]} window gather C={c}")
