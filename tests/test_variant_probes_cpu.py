"""CPU: the launch probes of `attn_variants` reach the variants they name, and together every variant of the lists.

The GPU tests of test_gpu_attention_variants.py launch these rows; here the host-only `mt4_attention_plan` (and the mirrored rules of the window and
LayerNorm launches) says which kernel each row gets, so a variant added to a list without a probe, or a probe that a changed rule sends elsewhere,
fails without a GPU.  The refusals of `mt4_layernorm` are asked of the entry itself with addresses it never dereferences: its checks precede any launch."""
import attn_variants as av
import pytest

FAMILY = {av.GENERIC: "generic", av.MFMA_BF16: "bf16 MFMA", av.MFMA_F32: "fp32 MFMA"}


def _ids(rows):
    return [f"{i}-dt{p['dt']}-{p['variant'][0]}_{p['variant'][1]}-hd{p['hd']}-nk{p['Nk']}" for i, p in enumerate(rows)]


@pytest.mark.parametrize("p", av.GENERIC_PROBES, ids=_ids(av.GENERIC_PROBES))
def test_generic_probe_reaches_its_variant(p):
    assert av.probe_plan(p) == (av.GENERIC,) + p["variant"], p
    dpl, lpq = p["variant"]
    assert p["Nq"] == 5 and dpl * lpq >= p["hd"]
    if p["bias"]:      # row a: the whole slice width, two LDS chunks, a last chunk that is no multiple of 4
        assert p["hd"] == dpl * lpq and p["Nk"] == av.max_keys(dpl, lpq) + 5 and p["nw"] == 2 and (p["Nk"] - av.max_keys(dpl, lpq)) % 4
    else:              # row b: element-wise staging, zero-padded head dims
        assert p["hd"] % 4 and p["hd"] < dpl * lpq and p["Nk"] == 7 and not p["nw"]


@pytest.mark.parametrize("p", av.MHA_BF16_PROBES, ids=_ids(av.MHA_BF16_PROBES))
def test_bf16_mfma_probe_reaches_its_variant(p):
    assert av.probe_plan(p) == (av.MFMA_BF16,) + p["variant"], p
    assert p["Nk"] in (16 * p["variant"][0] - 3, 16 * p["variant"][0]) and p["Nq"] == 70


@pytest.mark.parametrize("p", av.MHA_F32_PROBES, ids=_ids(av.MHA_F32_PROBES))
def test_fp32_mfma_probe_reaches_its_variant(p):
    assert av.probe_plan(p) == (av.MFMA_F32,) + p["variant"], p


def test_fp32_mfma_probes_cover_the_edges():
    rows = av.MHA_F32_PROBES
    assert {p["hd"] for p in rows} == {4, 108, 128} and {1, 128, 129, 256} <= {p["Nk"] for p in rows}
    assert any(p["Nq"] == 65 and p["variant"][1] == 1 for p in rows) and any(p["Nq"] == 17 and p["variant"][1] == 4 for p in rows)
    assert dict(dt=av.F32, variant=(8, 1), B=16, H=8, Nq=64, Nk=100, hd=108, bias=False, nw=0) in rows


def test_window_probes_reach_every_tile_count():
    assert [av.window_nt(n) for n, _ in av.WINDOW_PROBES[:16]] == list(range(1, 17))
    assert [(n, av.window_nt(n)) for n, _ in av.WINDOW_PROBES[16:]] == [(128, 8), (240, 15)]
    assert {av.window_nt(n) for n, _ in av.WINDOW_PROBES} == {nt for nt, _ in av.WINDOW}
    assert all(n % 16 for n, _ in av.WINDOW_PROBES[:16])                          # ragged last tile
    assert [nw for _, nw in av.WINDOW_PROBES[:16]] == [2, 0] * 8                   # a mask on every other row
    assert {ws for ws, _, _, shift in av.WINDOW_REL_PROBES if shift} == {ws for ws, _, _, shift in av.WINDOW_REL_PROBES if not shift} == set(range(2, 15))
    assert all(res % ws == 0 and 0 <= shift < ws and av.window_nt(ws * ws) <= 16 for ws, _, res, shift in av.WINDOW_REL_PROBES)


def test_layernorm_rule_and_probes():
    """nch = G C / V; the first narrow kernel with nch <= LPR, else the first wide one with nch <= 64 MAXCH"""
    assert [av.ln_kernel(av.BF16, 1, 8 * n) for n in (1, 16, 17, 32, 33, 128, 129, 256, 257, 512, 513, 1024, 1025)] == \
        [("narrow", 16)] * 2 + [("narrow", 32)] * 2 + [("wide", 2)] * 2 + [("wide", 4)] * 2 + [("wide", 8)] * 2 + [("wide", 16)] * 2 + [None]
    assert av.ln_kernel(av.F32, 1, 4 * 33) == ("wide", 2) and av.ln_kernel(av.F32, 4, 128) == ("wide", 2) and av.ln_kernel(av.BF16, 4, 512) == ("wide", 4)
    assert av.ln_kernel(av.BF16, 1, 132) is None and av.ln_kernel(av.F32, 1, 130) is None
    every = {("narrow", l) for l in av.LN_NARROW} | {("wide", m) for m in av.LN_WIDE}
    for dt in (av.F32, av.BF16):
        rows = [(m, c, g) for d, m, c, g in av.LN_PROBES if d == dt]
        assert {av.ln_kernel(dt, g, c) for _, c, g in rows} == every
        assert {g * c // av.LN_V[dt] for _, c, g in rows} == set(av.LN_NCH) and {m for m, _, _ in rows} == set(av.LN_ROWS)
    # both ends of every kernel's range: the one before's limit + 1, its own limit
    limits = av.LN_NARROW + [64 * m for m in av.LN_WIDE]
    assert av.LN_NCH == sorted([1] + [l + 1 for l in limits[:-1]] + limits)
    assert [av.ln_kernel(dt, 4, c) for dt, _, _, c in av.LN_MERGE_PROBES] == [("wide", 4), ("wide", 2)]
    assert [av.ln_kernel(dt, 1, c) for dt, _, _, _, _, c in av.LN_WINDOW_PROBES] == [("wide", 2), ("wide", 2)]


def test_probes_cover_every_variant_per_dtype():
    """the set of variants the tables reach (as the library plans them) equals the full lists: a variant added later without a probe fails here"""
    reached = {}
    for p in av.GENERIC_PROBES + av.MHA_BF16_PROBES + av.MHA_F32_PROBES:
        fam, p0, p1 = av.probe_plan(p)
        reached.setdefault((fam, p["dt"]), set()).add((p0, p1))
    assert reached[(av.GENERIC, av.F32)] == set(av.ATTN_GENERIC), set(av.ATTN_GENERIC) ^ reached[(av.GENERIC, av.F32)]
    assert reached[(av.GENERIC, av.BF16)] == set(av.ATTN_GENERIC), set(av.ATTN_GENERIC) ^ reached[(av.GENERIC, av.BF16)]
    assert reached[(av.MFMA_BF16, av.BF16)] == set(av.MHA_BF16)
    assert reached[(av.MFMA_F32, av.F32)] == set(av.MHA_F32)
    assert set(reached) == {(av.GENERIC, av.F32), (av.GENERIC, av.BF16), (av.MFMA_BF16, av.BF16), (av.MFMA_F32, av.F32)}
    assert len(av.ATTN_GENERIC) == len(set(av.ATTN_GENERIC)) == len(av.GENERIC_ROWS) and [r[0] for r in av.GENERIC_ROWS] == av.ATTN_GENERIC


def test_every_listed_variant_is_reachable():
    """sweep of the planner: every member of ATTN_GENERIC, MHA_BF16 and MHA_F32 is what SOME call gets (a variant no call can reach is dead code
    that is compiled, shipped and never tested)"""
    reached = set()
    for hd in range(1, 513):
        for dt in (av.F32, av.BF16):
            for bias in (False, True):
                for bh in (1, 256):
                    for nq in (5, 256):
                        for nk in (7, 144, 300):
                            reached.add(av.plan(dt, bh, 1, nq, nk, hd, bias=bias))
    got = {fam: {(p0, p1) for f, p0, p1, _ in reached if f == fam} for fam in FAMILY}
    for fam, want in ((av.GENERIC, av.ATTN_GENERIC), (av.MFMA_BF16, av.MHA_BF16), (av.MFMA_F32, av.MHA_F32)):
        if fam == av.MFMA_BF16:        # its key-tile counts need more Nk than the sweep's three: test_bf16_mfma_covers_every_key_tile_count walks 1 .. 160
            got[fam] |= {av.plan(av.BF16, 2, 4, 64, nk, hd)[1:3] for hd in (256, 384) for nk in range(8, 161, 16)}
        assert got[fam] == set(want), (FAMILY[fam], "never chosen:", sorted(set(want) - got[fam]), "not listed:", sorted(got[fam] - set(want)))


def test_layernorm_refusals():
    from computervision_codes_amd import _lib
    ln = lambda m, c, g, dt, map_=None, l_out=0, l_in=0: _lib.lib.mt4_layernorm(av.FAKE_PTR, av.FAKE_PTR, av.FAKE_PTR, av.FAKE_PTR, m, c, g, map_, l_out,
                                                                               l_in, 1e-5, dt, None)
    assert ln(4, 8 * 1025, 1, av.BF16) == av.MT4_EUNSUPPORTED and ln(4, 4 * 1025, 1, av.F32) == av.MT4_EUNSUPPORTED          # nch = 1025
    assert ln(4, 2050, 4, av.BF16, av.FAKE_PTR, 4, 16) == av.MT4_EALIGN and ln(4, 4 * 1025, 4, av.F32, av.FAKE_PTR, 4, 16) == av.MT4_EUNSUPPORTED
    assert ln(4, 132, 1, av.BF16) == av.MT4_EALIGN and ln(4, 130, 1, av.F32) == av.MT4_EALIGN                                  # C % V != 0
    assert ln(4, 128, 4, av.BF16) == av.MT4_EINVAL and ln(4, 128, 2, av.F32) == av.MT4_EINVAL                                  # G != 1 without a map
    assert ln(4, 128, 1, 7) == av.MT4_EUNSUPPORTED and ln(0, 128, 1, av.BF16) == av.MT4_EINVAL
