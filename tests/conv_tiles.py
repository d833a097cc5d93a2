"""The tile list of `mt4_conv_nhwc` and what it launches for which descriptor, as Python literals.

`GENERIC_TILES`, `PATCH_TILES`, `STEM_TILE` and `RETIRED_TILES` mirror `MT4_CONV_TILES` of csrc/igemm_conv.hip; `test_conv_plan_cpu.py` asserts
every entry against `mt4_conv_tile_info`, so the GPU tests can parametrise over them without loading the library at collection.

`DISPATCH` holds every probe of `tools/conv_dispatch_sweep.py` with the tile (or the error) the launch path must answer, asserted through
`mt4_conv_plan` on a CPU.  The expectation of each row is worked out BY HAND from the rule's arithmetic in csrc/igemm_conv.hip (`choose_tile`,
`auto_tile`, `patch3x3_lds`, `stem_patch_lds`) and written beside it; none was produced by running the library.  Shorthand of the comments:
  es        bytes per element (fp32 4, bf16 2);  CPT = Cin es / 16;  nsteps = ceil(KH KW CPT / 8);  fast <=> Cin es % 128 == 0 and KH, KW <= 8
  tiles(t)  ceil(M / BM_t) * ceil(N / BN_t), M = B Ho Wo, N = Cout      t64 = ceil(M / 64) ceil(N / 64)
  small     the "most blocks" loop of auto_tile over tiles 1..6: the 32 x 32 tile 6 wins whenever it is allowed, and becomes 11 at nsteps >= 8

This is a plain module beside `bf16_bounds.py` (`tests/` is on sys.path while pytest runs), not a conftest.
"""
import ctypes

MT4_OK, MT4_EINVAL, MT4_EALIGN, MT4_ELAUNCH, MT4_EUNSUPPORTED = 0, -1, -2, -3, -4
GENERIC, PATCH, STEM, RETIRED = 0, 1, 2, 3        # MT4_TILE_* of include/mt4hip.h

# id: (BM, BN, operand stages, K-split groups)     igemm_conv_kernel
GENERIC_TILES = {
    1: (128, 128, 2, 1), 2: (128, 64, 2, 1), 3: (64, 64, 2, 1), 4: (64, 128, 2, 1), 5: (32, 64, 2, 1), 6: (32, 32, 2, 1),
    7: (128, 128, 3, 1), 8: (64, 128, 3, 1), 9: (64, 64, 4, 1), 10: (32, 64, 4, 1), 11: (32, 32, 4, 1), 12: (128, 64, 3, 1),
    13: (256, 128, 2, 1), 14: (256, 128, 3, 1), 15: (256, 256, 2, 1), 16: (128, 256, 3, 1),
    17: (256, 256, 2, 1), 18: (256, 128, 2, 1), 19: (256, 128, 3, 1), 20: (256, 64, 2, 1),
    35: (32, 32, 2, 4), 36: (32, 64, 2, 4), 37: (32, 32, 2, 8), 38: (32, 32, 3, 4),
    39: (64, 64, 2, 2), 40: (64, 64, 2, 4), 41: (64, 64, 3, 2), 42: (64, 128, 2, 2),
}
# id: (BM, BN, waves, weight stages)               conv3x3_patch_kernel (bf16, 3x3, stride 1, pad 1)
PATCH_TILES = {23: (256, 256, 16, 2), 24: (256, 64, 8, 2), 26: (256, 128, 16, 2), 30: (128, 128, 4, 2), 32: (256, 128, 8, 2)}
STEM_TILE = 33                                     # stem_patch_kernel: 256 x 64, 8 waves
STEM_TILE_CFG = (256, 64, 8)
RETIRED_TILES = (21, 22, 25, 27, 28, 29, 31, 34)   # the tuning record: MT4_EUNSUPPORTED
NUM_TILES = 42

SEQ_TILES = sorted(t for t, c in GENERIC_TILES.items() if c[3] == 1)        # one wave group walks K in order
KSPLIT_TILES = sorted(t for t, c in GENERIC_TILES.items() if c[3] > 1)      # LDS-DMA geometries only
RING_TILES = sorted(t for t, c in GENERIC_TILES.items() if c[2] > 2 or c[3] > 1)   # what the K-step sweep walks


def fast_rule(cin, es, kh, kw):
    """the documented rule of the LDS-DMA path for tensors far below 2 GiB (csrc/igemm_conv.hip, fill_conv_args)"""
    return (cin * es) % 128 == 0 and kh <= 8 and kw <= 8


def conv(note, B, H, W, cin, cout, kh, kw, dt, expect, *, tile=0, latency=False, stride=(1, 1), pad=(0, 0), dil=(1, 1), stats=False, od=None,
         run_pixels=1, out_hw=None, relu=False):
    """one probe: the arguments of an `ops.conv_nhwc` call on a [B, H, W, cin / run_pixels] tensor; expect = (kind, tile) or an MT4_E* code"""
    return dict(note=note, B=B, H=H, W=W, cin=cin, cout=cout, kh=kh, kw=kw, dt=dt, expect=expect, tile=-1 if latency else tile, stride=stride,
                pad=pad, dil=dil, stats=stats, od=od or dt, run_pixels=run_pixels, out_hw=out_hw, relu=relu)


def gemm(note, M, cin, cout, dt, expect, **kw):      # 1x1: nsteps = cin * es / 128
    return conv(note, M // 256 if M % 256 == 0 else 1, 1, 256 if M % 256 == 0 else M, cin, cout, 1, 1, dt, expect, **kw)


def tcn(note, T, cin, cout, kw, dt, expect, **k):    # 1 x kw over one video of T frames, 'same' padding
    return conv(note, 1, 1, T, cin, cout, 1, kw, dt, expect, pad=(0, kw // 2), **k)


def stem(note, B, H, W, kh, cout, expect, tile=0):   # the space-to-depth stem: runs of 4 pixels x 16 channels, kh x 1, valid
    return conv(note, B, H, W, 64, cout, kh, 1, "bf16", expect, tile=tile, run_pixels=4, out_hw=(H - kh + 1, W - 3), relu=True)


def _explicit():
    rows = []
    # bf16 3x3 pad 1 on 3 x 14 x 14 x 128 -> 128: Cin es = 256: fast; M = 588; nsteps = ceil(9 * 16 / 8) = 18 = 9 SPT (SPT = 2): patch3x3_ok.
    # Generic ids launch as named (K-split ids too: the geometry is fast); retired ids and the stem id (KW != 1) refuse.  Patch ids,
    # patch3x3_lds with W = 14, two slices: pra = (BM + 2 W + 4 + 7) // 8 * 8 = 288 (BM 256) or 160 (BM 128),
    #   23: 2 * 288 * 128 + 2 * 256 * 128 = 139264 <= 163840, ceil(288 / 128) = 3 <= 9      24: 73728 + 16384 = 90112, ceil(288 / 64) = 5 <= 9
    #   26: 73728 + 32768 = 106496, 3 <= 9      30: 2 * 160 * 128 + 32768 = 73728, ceil(160 / 32) = 5 <= 9      32: 106496, 5 <= 9     all fit
    # fp32 1x3 TCN layer 1 x 1 x 256 x 64 -> 64: Cin es = 256: fast, nsteps = ceil(3 * 16 / 8) = 6; fp32 is not patch3x3_ok, KW = 3 is no stem
    for t in range(1, NUM_TILES + 1):
        if t in GENERIC_TILES:
            a = b = (GENERIC, t)
        elif t in PATCH_TILES:
            a, b = (PATCH, t), MT4_EUNSUPPORTED
        else:
            a = b = MT4_EUNSUPPORTED
        rows.append(conv("explicit, bf16 3x3", 3, 14, 14, 128, 128, 3, 3, "bf16", a, tile=t, pad=(1, 1)))
        rows.append(tcn("explicit, fp32 TCN 1x3", 256, 64, 64, 3, "f32", b, tile=t))
    return rows


DISPATCH = _explicit() + [
    conv("tile > count: EINVAL", 1, 14, 14, 64, 64, 3, 3, "bf16", MT4_EINVAL, tile=NUM_TILES + 1, pad=(1, 1)),
    conv("tile < -1: EINVAL", 1, 14, 14, 64, 64, 3, 3, "bf16", MT4_EINVAL, tile=-2, pad=(1, 1)),

    # ---- the stem rule.  Cin 64 bf16 = CPT 8: fast; x_pixel_stride 16 = 32 bytes; nsteps = KH
    # 2 x 67 x 115, kh 4: Ho x Wo = 64 x 112, HoWo 7168 >= 256: stem_patch_ok.  stem_patch_lds: rows crossed = ceil(256 / 112) + 1 = 4, span =
    # 256 + 3 * 4 + 3 * 115 + 4 = 617, pra = 640, lds = 640 * 32 + 4 * 64 * 128 = 53248 <= 163840 -> the stem kernel
    stem("stem_patch_ok, tile 0 -> stem kernel", 2, 67, 115, 4, 64, (STEM, 33)),
    stem("stem_patch_ok, tile 33", 2, 67, 115, 4, 64, (STEM, 33), tile=33),
    # 1 x 8 x 453, kh 8: Ho x Wo = 1 x 450, HoWo 450 >= 256: ok.  rows crossed = ceil(256 / 450) + 1 = 2, span = 256 + 6 + 7 * 453 + 4 = 3437,
    # pra = 3456, lds = 3456 * 32 + 8 * 64 * 128 = 110592 + 65536 = 176128 > 163840: no stem launch.  tile 0 goes on: KW 1 is no patch;
    # auto_tile(450, 64, 8, 2): tiles(20) = 2, tiles(2) = 4, tiles(3) = 8: all < 256; small: tile 6 (15 * 2 = 30 blocks), nsteps 8 >= 8 -> 11
    stem("stem patch > 160 KB, tile 0 -> generic", 1, 8, 453, 8, 64, (GENERIC, 11)),
    stem("stem patch > 160 KB, tile 33 -> unsupported", 1, 8, 453, 8, 64, MT4_EUNSUPPORTED, tile=33),
    # 1 x 11 x 19, kh 4: HoWo = 8 * 16 = 128 < 256.  auto_tile(128, 64, 4, 2): tiles(2) = 1, tiles(3) = 2; small: 6 (4 * 2 = 8), nsteps 4 < 8 -> 6
    stem("HoWo < 256: not stem_patch_ok -> generic", 1, 11, 19, 4, 64, (GENERIC, 6)),

    # ---- the patch rule: tile 0, patch3x3_ok and ceil(M / 256) ceil(Cout / 256) >= 256.  Cin 64 bf16: one slice, nsteps 9
    # M = 21 * 3136 = 65856: ceil(/ 256) = 258 >= 256; Cout 64 -> 24: pra = (256 + 112 + 11) // 8 * 8 = 376, lds = 376 * 128 + 2 * 64 * 128 = 64512: fits
    conv("patch: 258 tiles, Cout 64 -> 24", 21, 56, 56, 64, 64, 3, 3, "bf16", (PATCH, 24), pad=(1, 1)),
    # M = 62720 = 245 * 256 < 256 tiles.  auto_tile(62720, 64, 9, 2): tiles(20) = 245 < 2048, tiles(2) = 490 >= 256 -> 2
    conv("patch: 245 tiles < 256 -> generic", 20, 56, 56, 64, 64, 3, 3, "bf16", (GENERIC, 2), pad=(1, 1)),
    # M = 68 * 961 = 65348: 256 tiles; 64 < Cout 72 <= 128 and W 31 <= 31 -> 30: pra = (128 + 62 + 11) // 8 * 8 = 200, lds = 25600 + 32768: fits
    conv("patch: Cout 72 > 64, W 31 -> 30", 68, 31, 31, 64, 72, 3, 3, "bf16", (PATCH, 30), pad=(1, 1)),
    # M = 65536: 256 tiles; Cout 128, W 32 > 31 -> 32: pra = (256 + 64 + 11) // 8 * 8 = 328, lds = 41984 + 32768: fits
    conv("patch: Cout 128, W 32 > 31 -> 32", 64, 32, 32, 64, 128, 3, 3, "bf16", (PATCH, 32), pad=(1, 1)),
    # 256 tiles * ceil(136 / 256) = 256; Cout 136 > 128 -> 23: pra = (256 + 62 + 11) // 8 * 8 = 328, lds = 41984 + 65536: fits
    conv("patch: Cout 136 > 128 -> 23", 68, 31, 31, 64, 136, 3, 3, "bf16", (PATCH, 23), pad=(1, 1)),
    # M = 147 * 448 = 65856: 258 tiles -> 24, but pra = (256 + 896 + 11) // 8 * 8 = 1160, lds = 148480 + 16384 = 164864 > 163840: generic.
    # auto_tile(65856, 64, 9, 2): tiles(20) = 258, tiles(2) = 515 >= 256 -> 2
    conv("patch: W 448, patch > 160 KB -> generic", 1, 147, 448, 64, 64, 3, 3, "bf16", (GENERIC, 2), pad=(1, 1)),
    # stride 2: Ho = Wo = 28, M = 84 * 784 = 65856; tiles(2) = 515 -> 2
    conv("patch: stride 2, not patch3x3_ok -> generic", 84, 56, 56, 64, 64, 3, 3, "bf16", (GENERIC, 2), pad=(1, 1), stride=(2, 2)),
    # fp32 Cin 32: CPT 8, nsteps 9; auto_tile(65856, 64, 9, 4): tiles(2) = 515 -> 2
    conv("patch: fp32, not patch3x3_ok -> generic", 21, 56, 56, 32, 64, 3, 3, "f32", (GENERIC, 2), pad=(1, 1)),
    conv("patch: latency caller, the rule holds for tile -1 too -> 24", 21, 56, 56, 64, 64, 3, 3, "bf16", (PATCH, 24), pad=(1, 1), latency=True),

    # ---- auto_tile(M, N, nsteps, es)
    # nsteps 1; tiles(13) = 128 * 2 = 256 >= 256 -> 13
    gemm("es 2, N >= 256, nsteps 1, tiles(13) = 256 -> 13", 128 * 256, 64, 256, "bf16", (GENERIC, 13)),
    # tiles(13) = 127 * 2 = 254; nsteps 1 and tiles(3) = 508 * 4 = 2032 >= 1024 -> 3
    gemm("tiles(13) = 254 -> on (nsteps 1, tiles(3) >= 1024 -> 3)", 127 * 256, 64, 256, "bf16", (GENERIC, 3)),
    # nsteps 2; tiles(15) = 190 * 1 >= 190 -> 17
    gemm("es 2, N >= 256, nsteps 2, tiles(15) = 190 -> 17", 190 * 256, 128, 256, "bf16", (GENERIC, 17)),
    # tiles(15) = 189; N > 64: nsteps 2 < 4, tiles(4) = 756 * 2 = 1512 >= 256 -> 4
    gemm("tiles(15) = 189 -> on (1: nsteps < 4, tiles(4) >= 256 -> 4)", 189 * 256, 128, 256, "bf16", (GENERIC, 4)),
    # fp32: nsteps 4; N > 64: tiles(1) = 256 * 2 = 512 >= 256 -> 1
    gemm("es 4, N >= 256: the 8-wave rules do not apply -> 1", 128 * 256, 128, 256, "f32", (GENERIC, 1)),
    # nsteps 4; N 248: tiles(1) = 256 * 2 -> 1
    gemm("es 2, N 248 < 256 -> 1", 128 * 256, 256, 248, "bf16", (GENERIC, 1)),
    # nsteps 1; tiles(20) = 1024 * 2 = 2048 >= 2048 -> 20
    gemm("es 2, 64 < N <= 128, nsteps 1 < 4, tiles(20) = 2048 -> 20", 1024 * 256, 64, 128, "bf16", (GENERIC, 20)),
    # tiles(20) = 2046; nsteps 1 and tiles(3) = 4092 * 2 >= 1024 -> 3
    gemm("tiles(20) = 2046 -> on (nsteps 1, tiles(3) >= 1024 -> 3)", 1023 * 256, 64, 128, "bf16", (GENERIC, 3)),
    # 1x4 valid over W 259: Wo 256, M = 2048 * 256; nsteps = 4 * 8 / 8 = 4; tiles(19) = 2048 * 1 -> 19
    conv("es 2, N 128, nsteps 4, tiles(19) = 2048 -> 19", 2048, 1, 259, 64, 128, 1, 4, "bf16", (GENERIC, 19)),
    # tiles(19) = 2047; N > 64, nsteps 4 >= 4, tiles(1) = 4094 >= 256 -> 1
    conv("tiles(19) = 2047 -> on (1)", 2047, 1, 259, 64, 128, 1, 4, "bf16", (GENERIC, 1)),
    # 1x3 valid over W 258: M = 512 * 256 = 131072, nsteps 3; tiles(20) = 512 * 2 = 1024 < 2048; N > 64: nsteps < 4, tiles(4) = 2048 -> 4
    conv("es 2, N 128, nsteps 3 < 4, tiles(20) < 2048 -> 4", 512, 1, 258, 64, 128, 1, 3, "bf16", (GENERIC, 4)),
    # nsteps 1; tiles(3) = 1024 * 1 >= 1024 -> 3
    gemm("nsteps 1, tiles(3) = 1024 -> 3", 65536, 32, 64, "f32", (GENERIC, 3)),
    # tiles(3) = 1023; 32 < N <= 64, fp32: tiles(2) = ceil(65472 / 128) = 512 >= 256 -> 2
    gemm("nsteps 1, tiles(3) = 1023 -> on (N <= 64, tiles(2) >= 256 -> 2)", 65472, 32, 64, "f32", (GENERIC, 2)),
    # nsteps 4; tiles(1) = 256 * 1 -> 1
    gemm("N > 64, nsteps 4, tiles(1) = 256 -> 1", 32768, 128, 128, "f32", (GENERIC, 1)),
    # tiles(1) = 255; tiles(4) = 510 >= 256 -> 4
    gemm("N > 64, nsteps 4, tiles(1) = 255, tiles(4) >= 256 -> 4", 32640, 128, 128, "f32", (GENERIC, 4)),
    # nsteps 2; tiles(4) = 256 -> 4
    gemm("N > 64, nsteps 2 < 4, tiles(4) = 256 -> 4", 16384, 64, 128, "f32", (GENERIC, 4)),
    # tiles(4) = 255, tiles(1) = 128; small: 6 (510 * 4 = 2040 blocks), nsteps 2 < 8 -> 6
    gemm("N > 64, tiles(4) = 255 -> small tiles, nsteps 2 < 8 -> 6", 16320, 64, 128, "f32", (GENERIC, 6)),
    # nsteps 2; tiles(20) = 2048 * 1 -> 20
    gemm("32 < N <= 64, es 2, tiles(20) = 2048 -> 20", 2048 * 256, 128, 64, "bf16", (GENERIC, 20)),
    # tiles(20) = 2047; tiles(2) = 4094 -> 2
    gemm("32 < N <= 64, es 2, tiles(20) = 2047 -> 2", 2047 * 256, 128, 64, "bf16", (GENERIC, 2)),
    # nsteps 2; tiles(2) = 256 -> 2
    gemm("32 < N <= 64, es 4, tiles(2) = 256 -> 2", 32768, 64, 64, "f32", (GENERIC, 2)),
    # tiles(2) = 255; tiles(3) = 510 -> 3
    gemm("32 < N <= 64, tiles(2) = 255, tiles(3) >= 256 -> 3", 32640, 64, 64, "f32", (GENERIC, 3)),
    # tiles(2) = 128, tiles(3) = 255; small: 6 (510 * 2), nsteps 2 -> 6
    gemm("32 < N <= 64, tiles(3) = 255 -> small tiles -> 6", 16320, 64, 64, "f32", (GENERIC, 6)),
    # N 32: only tile 6 is allowed; nsteps 2 -> 6
    gemm("N 32: neither N block -> 6", 16320, 64, 32, "f32", (GENERIC, 6)),
    # nsteps = 1024 * 4 / 128 = 32; tiles(2) = 96, tiles(3) = 192 < 256; nsteps >= 32, N > 32, tiles(3) >= 192 -> 9
    gemm("nsteps 32, N > 32, tiles(3) = 192 -> 9", 192 * 64, 1024, 64, "f32", (GENERIC, 9)),
    # tiles(3) = 191; small: 6, nsteps 32 >= 8 -> 11
    gemm("nsteps 32, tiles(3) = 191 -> 11", 191 * 64, 1024, 64, "f32", (GENERIC, 11)),
    # nsteps = 992 / 32 = 31 < 32 -> small -> 11
    gemm("nsteps 31 < 32, tiles(3) = 192 -> 11", 192 * 64, 992, 64, "f32", (GENERIC, 11)),
    # N 32 is not > 32 -> small -> 11
    gemm("nsteps 32, N 32 -> 11", 192 * 64, 1024, 32, "f32", (GENERIC, 11)),
    # M 256, nsteps 6: tiles(2) = 2, tiles(3) = 4; small: 6 (8 * 2), nsteps 6 < 8 -> 6
    tcn("few tiles, nsteps 6 < 8 -> 6", 256, 64, 64, 3, "f32", (GENERIC, 6)),
    # nsteps = ceil(3 * 32 / 8) = 12 >= 8 -> 11
    tcn("few tiles, nsteps 12 >= 8 -> 11", 256, 128, 64, 3, "f32", (GENERIC, 11)),

    # ---- the latency overrides (tile -1)
    # auto 11 (row above); fast, fp32: tiles(37) = 8 * 2 = 16 <= 256 -> 37 (37 is not in the list of the whole-video rule: stays)
    tcn("latency, fast, fp32, 11, tiles(37) = 16 <= 256 -> 37", 256, 128, 64, 3, "f32", (GENERIC, 37), latency=True),
    # auto_tile(4096, 64, 12, 4): tiles(2) = 32, tiles(3) = 64 -> small -> 11; tiles(37) = 128 * 2 = 256 <= 256 -> 37
    tcn("latency, fp32, 11, tiles(37) = 256 -> 37", 4096, 128, 64, 3, "f32", (GENERIC, 37), latency=True),
    # tiles(37) = 129 * 2 = 258 > 256: 11 stays; t64 = 65 * 1 < 192: 11 stays
    tcn("latency, fp32, 11, tiles(37) = 258 > 256, t64 = 65 < 192 -> 11", 4128, 128, 64, 3, "f32", (GENERIC, 11), latency=True),
    # Cin 48 fp32: CPT 12, not fast; nsteps = ceil(7 * 12 / 8) = 11 -> auto 11; every override asks for fast
    tcn("latency, not fast (CPT 12), 11 stays", 256, 48, 64, 7, "f32", (GENERIC, 11), latency=True),
    # bf16 Cin 256: CPT 32, nsteps 12 -> auto 11; t64 = 4 * 1; 32 x 64 tiles = 8 * 1 < 256 -> 11
    tcn("latency, bf16, 11, t64 = 4, 32x64 tiles 8 < 256 -> 11", 256, 256, 64, 3, "bf16", (GENERIC, 11), latency=True),
    # auto_tile(8192, 64, 12, 2): tiles(20) = 32, tiles(2) = 64, tiles(3) = 128 -> small -> 11; t64 = 128 < 192; 32 x 64 tiles = 256 >= 256 -> 10
    tcn("latency, bf16, 11, t64 = 128, 32x64 tiles = 256 -> 10", 8192, 256, 64, 3, "bf16", (GENERIC, 10), latency=True),
    # 32 x 64 tiles = 255 -> 11
    tcn("latency, bf16, 11, 32x64 tiles = 255 -> 11", 8160, 256, 64, 3, "bf16", (GENERIC, 11), latency=True),
    # auto 6 (nsteps 6): the overrides ask for 10 / 11, or nsteps >= 8
    tcn("latency, nsteps 6 < 8: 6 stays", 256, 64, 64, 3, "f32", (GENERIC, 6), latency=True),
    # auto 1; t128 = 256 < 512 and 64 x 128 tiles = 512 >= 256 -> 4
    gemm("latency, 1, t128 = 256 < 512 -> 4", 32768, 128, 128, "f32", (GENERIC, 4), latency=True),
    # t128 = 512, not < 512 -> 1
    gemm("latency, 1, t128 = 512 -> 1 stays", 65536, 128, 128, "f32", (GENERIC, 1), latency=True),
    # auto 4, nsteps 2: no rule names tile 4
    gemm("latency, auto 4: no override", 16384, 64, 128, "f32", (GENERIC, 4), latency=True),
    # M 2000, N 512, nsteps = 3 * 128 / 8 = 48: tiles(1) = 16 * 4 = 64, tiles(4) = 32 * 4 = 128 < 256; tiles(3) = 32 * 8 = 256 >= 192 -> 9; t64 = 256 -> 40
    tcn("latency, fp32 whole video, 9, t64 = 256 -> 40", 2000, 512, 512, 3, "f32", (GENERIC, 40), latency=True),
    # nsteps 24: tiles(15) = 8 * 2 = 16 < 190, tiles(1) = 64, tiles(4) = 128, 24 < 32; small: 6 (63 * 16 = 1008), nsteps >= 8 -> 11; t64 = 256 -> 41
    tcn("latency, bf16 whole video, 11, t64 = 256 -> 41", 2000, 512, 512, 3, "bf16", (GENERIC, 41), latency=True),
    # auto_tile(12288, 64, 12, 4): tiles(2) = 96, tiles(3) = 192 < 256, 12 < 32 -> small -> 11; tiles(37) = 384 * 2 > 256; t64 = 192 -> 40
    tcn("latency, fp32, 11, t64 = 192 -> 40", 192 * 64, 128, 64, 3, "f32", (GENERIC, 40), latency=True),
    # t64 = 191 < 192 -> 11
    tcn("latency, fp32, 11, t64 = 191 -> 11", 191 * 64, 128, 64, 3, "f32", (GENERIC, 11), latency=True),
    # auto_tile(4032, 512, 12, 4): tiles(1) = 32 * 4 = 128, tiles(4) = 63 * 4 = 252 < 256 -> small -> 11; tiles(37) = 126 * 16 > 256; t64 = 63 * 8 = 504 <= 512 -> 40
    tcn("latency, fp32, 11, t64 = 504 (the most the small tiles see) -> 40", 63 * 64, 128, 512, 3, "f32", (GENERIC, 40), latency=True),
    tcn("the same geometry, tile 0: 11", 2000, 512, 512, 3, "bf16", (GENERIC, 11)),

    # ---- stat_sums.  A generic tile holds them when it has one wave group and waves * BN * 16 <= (BM + BN) * 128; Cout % 8 (fp32 output: % 4)
    # tile 2: 4 * 64 * 16 = 4096 <= 192 * 128
    conv("stat_sums, generic tile 2", 3, 14, 14, 64, 64, 3, 3, "bf16", (GENERIC, 2), pad=(1, 1), tile=2, stats=True),
    conv("stat_sums, generic tile 2, fp32", 3, 14, 14, 64, 64, 3, 3, "f32", (GENERIC, 2), pad=(1, 1), tile=2, stats=True),
    # Cin 24 bf16: 48 bytes, CPT 3: not fast; tile 9: 4 * 64 * 16 <= 128 * 128
    conv("stat_sums, generic tile 9, not fast (Cin 24)", 3, 14, 14, 24, 64, 3, 3, "bf16", (GENERIC, 9), pad=(1, 1), tile=9, stats=True),
    # W 14, one slice: pra = 288, lds = 36864 + 16384: fits
    conv("stat_sums, patch tile 24", 3, 14, 14, 64, 64, 3, 3, "bf16", (PATCH, 24), pad=(1, 1), tile=24, stats=True),
    conv("stat_sums, auto -> patch 24", 21, 56, 56, 64, 64, 3, 3, "bf16", (PATCH, 24), pad=(1, 1), stats=True),
    # M 588: 3 tiles of 256: no patch; auto_tile(588, 64, 9, 2): tiles(2) = 5, tiles(3) = 10 -> small -> 6 -> nsteps 9 >= 8 -> 11: 4 * 32 * 16 <= 64 * 128
    conv("stat_sums, auto -> generic", 3, 14, 14, 64, 64, 3, 3, "bf16", (GENERIC, 11), pad=(1, 1), stats=True),
    conv("stat_sums, K-split tile 35: unsupported", 3, 14, 14, 64, 64, 3, 3, "bf16", MT4_EUNSUPPORTED, pad=(1, 1), tile=35, stats=True),
    # tile 17: 16 * 256 * 16 = 65536 <= 512 * 128 = 65536
    conv("stat_sums, generic tile 17 (16 waves)", 3, 14, 14, 64, 64, 3, 3, "bf16", (GENERIC, 17), pad=(1, 1), tile=17, stats=True),
    # 68 % 8 = 4
    conv("stat_sums, Cout 68: unsupported", 3, 14, 14, 64, 68, 3, 3, "bf16", MT4_EUNSUPPORTED, pad=(1, 1), tile=2, stats=True),
    conv("stat_sums, latency caller: unsupported", 3, 14, 14, 64, 64, 3, 3, "bf16", MT4_EUNSUPPORTED, pad=(1, 1), latency=True, stats=True),

    # ---- the other routes through the entry point
    # nsteps = ceil(9 * 3 / 8) = 4; small: 6 (19 * 2 = 38), nsteps 4 < 8 -> 6
    conv("generic, not fast (Cin 24), tile 0", 3, 14, 14, 24, 64, 3, 3, "bf16", (GENERIC, 6), pad=(1, 1)),
    # fp32 output is not patch3x3_ok; auto_tile(588, 64, 9, 2) -> 11 (as above)
    conv("generic, bf16 in / fp32 out", 3, 14, 14, 64, 64, 3, 3, "bf16", (GENERIC, 11), pad=(1, 1), od="f32"),
]

LATENCY_ROWS = [r for r in DISPATCH if r["tile"] == -1 and not r["stats"] and isinstance(r["expect"], tuple) and r["expect"][0] == GENERIC]


def out_size(h, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1


_DT = {"f32": 0, "bf16": 1}
_anchor = (ctypes.c_char * 64)()
FAKE_PTR = (ctypes.addressof(_anchor) + 15) & ~15     # a 16-byte aligned address of a small live buffer: never dereferenced by the planner


def descriptor(B, H, W, cin, cout, kh, kw, dt, *, tile=0, stride=(1, 1), pad=(0, 0), dil=(1, 1), od=None, run_pixels=1, out_hw=None, act=0,
               x=FAKE_PTR, w=FAKE_PTR, y=FAKE_PTR, bias=FAKE_PTR, residual=None, residual_float=0, stat_sums=None, out_row_map=None,
               out_row_map_len=0, out_rows_per_image=0, y_ld=0, res_ld=0):
    """the `mt4_conv_desc` that `ops.conv_nhwc` builds for these arguments (cin = channels of a K-row: run_pixels pixels of cin / run_pixels)"""
    from computervision_codes_amd import _lib
    ho, wo = out_hw or (out_size(H, kh, stride[0], pad[0], dil[0]), out_size(W, kw, stride[1], pad[1], dil[1]))
    d = _lib.ConvDesc()
    d.x, d.w, d.bias, d.residual, d.y, d.out_row_map = x, w, bias, residual, y, out_row_map
    d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout, d.KH, d.KW = B, H, W, cin, ho, wo, cout, kh, kw
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = stride[0], stride[1], pad[0], pad[1], dil[0], dil[1]
    d.relu, d.dtype, d.out_dtype, d.tile = act, _DT[dt], _DT[od or dt], tile
    d.out_row_map_len, d.y_ld, d.res_ld, d.out_rows_per_image = out_row_map_len, y_ld, res_ld, out_rows_per_image
    d.x_pixel_stride = cin // run_pixels if run_pixels > 1 else 0
    d.residual_float = residual_float
    d.stat_sums = stat_sums
    return d


def probe_descriptor(r):
    return descriptor(r["B"], r["H"], r["W"], r["cin"], r["cout"], r["kh"], r["kw"], r["dt"], tile=r["tile"], stride=r["stride"], pad=r["pad"],
                      dil=r["dil"], od=r["od"], run_pixels=r["run_pixels"], out_hw=r["out_hw"], act=1 if r["relu"] else 0,
                      stat_sums=FAKE_PTR if r["stats"] else None)


def plan(d):
    """`mt4_conv_plan(d)` -> (return code, kind, tile, fast)"""
    from computervision_codes_amd import _lib
    kind, tile, fast = ctypes.c_int32(-9), ctypes.c_int32(-9), ctypes.c_int32(-9)
    rc = _lib.lib.mt4_conv_plan(ctypes.byref(d), ctypes.byref(kind), ctypes.byref(tile), ctypes.byref(fast))
    return rc, kind.value, tile.value, fast.value
