"""CPU: what `mt4_attention` would launch, asked of the library instead of restated in a test.

Every probe of `attn_variants.DISPATCH` (each expectation derived by hand beside its row) through `mt4_attention_plan`; every refused probe
through `mt4_attention` as well, which returns the same code before any launch; the refusals of the window entries through the entries
themselves, with addresses that a refusal never dereferences.  No call that the checks accept is ever passed to a launching entry here."""
import ctypes

import attn_variants as av
import pytest


@pytest.mark.parametrize("i", range(len(av.DISPATCH)), ids=lambda i: f"{i}-{av.DISPATCH[i]['note'][:36].replace(' ', '_')}-dt{av.DISPATCH[i]['dt']}")
def test_dispatch_table(i):
    """one probe: the planner's answer equals the hand-derived one; a refusal is also what `mt4_attention` answers"""
    from computervision_codes_amd import _lib
    r = av.DISPATCH[i]
    args = av.plan_args(r)
    got = av.plan_call(args)
    if isinstance(r["expect"], tuple):
        assert got == (av.MT4_OK,) + r["expect"], (r["note"], got)
    else:
        assert got == (r["expect"], -9, -9, -9, -9), (r["note"], got)           # refused, nothing written
        assert _lib.lib.mt4_attention(*args, None) == r["expect"], r["note"]


def test_dispatch_table_covers_what_it_claims():
    exp = [r["expect"] for r in av.DISPATCH if isinstance(r["expect"], tuple)]
    assert {e[0] for e in exp} == {av.GENERIC, av.MFMA_BF16, av.MFMA_F32}
    assert {e[1:3] for e in exp if e[0] == av.MFMA_F32} == set(av.MHA_F32)                     # both tile counts, with and without the key split
    assert {e[1:3] for e in exp if e[0] == av.MFMA_BF16} <= set(av.MHA_BF16)
    generic = {e[1:3] for e in exp if e[0] == av.GENERIC}
    assert generic <= set(av.ATTN_GENERIC) and generic & set(av.ATTN_BASE) and generic & set(av.ATTN_FEW) and generic == generic | set(av.ATTN_WIDE)
    assert {r["expect"] for r in av.DISPATCH if not isinstance(r["expect"], tuple)} == {av.MT4_EINVAL, av.MT4_EUNSUPPORTED}
    assert all(e[3] <= 65536 for e in exp)
    assert len(av.ATTN_GENERIC) == 11 and len(set(av.ATTN_GENERIC)) == 11 and len(av.MHA_BF16) == 20 and len(av.WINDOW) == 16


@pytest.mark.parametrize("dt", [av.F32, av.BF16])
def test_generic_variant_follows_the_head_dim(dt):
    """with a bias (no matrix-unit kernel) and plenty of workgroups (no few-workgroups rule): the first pair of BASE + WIDE that covers hd"""
    for hd in list(range(1, 40)) + [47, 48, 49, 64, 65, 80, 81, 112, 113, 128, 129, 256, 257, 384, 385, 512]:
        want = next((d, l) for d, l in av.ATTN_BASE + av.ATTN_WIDE if d * l >= hd)
        rc, fam, p0, p1, lds = av.plan_call(av.plan_args(av.attn("walk", dt, 64, 8, 64, 64, hd, None, bias=True)))
        row = want[1] * (want[0] + 4)
        assert (rc, fam, p0, p1) == (av.MT4_OK, av.GENERIC) + want and lds == 2 * min(8192 // row // 4 * 4, 64) * row * 4, (hd, rc, fam, p0, p1, lds)


def test_bf16_mfma_covers_every_key_tile_count():
    for hd in (256, 384):
        for nk in range(1, 161):
            nkt = -(-nk // 16)
            assert av.plan(av.BF16, 2, 4, 64, nk, hd) == (av.MFMA_BF16, nkt, hd, 16 * nkt * 160 + 32 * ((nkt + 1) // 2) * 128), (hd, nk)
    assert av.plan(av.BF16, 2, 4, 64, 144, 320)[0] == av.GENERIC            # a head dim without a variant
    assert av.plan(av.BF16, 2, 4, 64, 144, 256, q_stride=1028)[0] == av.GENERIC
    assert av.plan(av.BF16, 2, 4, 64, 144, 256, o_stride=1026)[0] == av.GENERIC


def test_plan_outputs_are_optional():
    from computervision_codes_amd import _lib
    args = av.plan_args(av.DISPATCH[0])
    assert _lib.lib.mt4_attention_plan(*args, None, None, None, None) == av.MT4_OK
    lds = ctypes.c_int32(-9)
    assert _lib.lib.mt4_attention_plan(*args, None, None, None, ctypes.byref(lds)) == av.MT4_OK and lds.value == 65536


def _window_rel(ws, B=4, H=4, **kw):
    """`mt4_window_attention_rel_bf16` on a packed qkv projection [B ws ws, 3 H 32] with addresses that a refusal never dereferences"""
    from computervision_codes_amd import _lib
    a = dict(q=av.FAKE_PTR, k=av.FAKE_PTR, v=av.FAKE_PTR, out=av.FAKE_PTR, table=av.FAKE_PTR, region=None, qkv_stride=3 * H * 32, o_stride=H * 32, nW=0)
    a.update(kw)
    return _lib.lib.mt4_window_attention_rel_bf16(a["q"], a["k"], a["v"], a["out"], a["table"], a["region"], ws, B, H, a["qkv_stride"], a["qkv_stride"],
                                                  a["qkv_stride"], a["o_stride"], a["nW"], 32 ** -0.5, None)


def test_window_refusals():
    """the relative-position form needs 2 NP 64 + NP2 64 + (2 (2 ws - 1)^2 + 4) 4 + NP 4 + 16 + NP 64 bytes of LDS: ws 14 (NP 208, NP2 224):
    26624 + 14336 + 5848 + 832 + 16 + 13312 = 60968 fits (and would launch: not called here); ws 15 (NP 240, NP2 256): 30720 + 16384 + 6744 + 960
    + 16 + 15360 = 70184 and ws 16 (NP = NP2 = 256): 32768 + 16384 + 7704 + 1024 + 16 + 16384 = 74280 exceed 64 KiB: refused, not launched"""
    from computervision_codes_amd import _lib
    assert _window_rel(15) == av.MT4_EUNSUPPORTED
    assert _window_rel(16) == av.MT4_EUNSUPPORTED
    assert _window_rel(16, region=av.FAKE_PTR, nW=4) == av.MT4_EUNSUPPORTED
    # the checks in front of it keep their codes and their order
    assert _window_rel(0) == av.MT4_EINVAL and _window_rel(17) == av.MT4_EINVAL            # N = 289 > 256
    assert _window_rel(12, q=None) == av.MT4_EINVAL and _window_rel(12, table=None) == av.MT4_EINVAL
    assert _window_rel(12, region=av.FAKE_PTR, nW=0) == av.MT4_EINVAL
    assert _window_rel(12, B=65536) == av.MT4_EUNSUPPORTED
    assert _window_rel(12, qkv_stride=3 * 4 * 32 + 4) == av.MT4_EALIGN and _window_rel(12, q=av.FAKE_PTR + 8) == av.MT4_EALIGN
    assert _window_rel(16, q=av.FAKE_PTR + 8) == av.MT4_EALIGN                            # alignment is checked before the LDS size
    expanded = lambda N, **kw: _lib.lib.mt4_window_attention_bf16(kw.get("q", av.FAKE_PTR), av.FAKE_PTR, av.FAKE_PTR, av.FAKE_PTR, kw.get("bias", av.FAKE_PTR),
                                                                  None, 4, 4, N, 384, 384, 384, 128, 0, 32 ** -0.5, None)
    assert expanded(257) == av.MT4_EINVAL and expanded(0) == av.MT4_EINVAL and expanded(144, bias=None) == av.MT4_EINVAL
    assert expanded(256, q=av.FAKE_PTR + 4) == av.MT4_EALIGN
