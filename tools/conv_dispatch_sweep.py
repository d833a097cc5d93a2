#!/usr/bin/env python3
"""Which kernel `mt4_conv_nhwc` launches for which descriptor: a flat list of `ops.conv_nhwc` / `ops.conv3x3_expand` calls, one launch each,
with a line per call (index, `ok` or the error).  Run under a kernel trace, the ordered (kernel, grid, workgroup, LDS) list of the conv
kernels is the launch path's fingerprint: a change to the host side of csrc/igemm_conv.hip that is meant to keep every launch must
reproduce it line for line.
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/conv_dispatch_sweep.py > DIR/calls.txt
  python tools/conv_dispatch_sweep.py --list DIR/*/*_kernel_trace.csv >> DIR/calls.txt      (no GPU needed)
The list: every explicit tile id on a bf16 3x3 layer and an fp32 1x3 TCN layer, then `tile=0` / `latency_tiles()` launches on both sides of
every comparison of the tile choice that a descriptor can reach (the branch is named beside each; the sides nothing can reach are listed
at the end), then the `stat_sums`, `second=` and `conv3x3_expand` routes.
The tile (or error) each plain probe must get is asserted without a GPU: `tests/conv_tiles.py` lists the same probes with the expectation derived
by hand, `tests/test_conv_plan_cpu.py` checks them through `mt4_conv_plan`.  A probe added here belongs there too."""
import os
import sys

if len(sys.argv) == 3 and sys.argv[1] == "--list":      # the conv launches of a trace, in dispatch order
    import csv
    for r in sorted(csv.DictReader(open(sys.argv[2])), key=lambda r: int(r["Dispatch_Id"])):
        if any(k in r["Kernel_Name"] for k in ("igemm_conv_kernel", "conv3x3_patch_kernel", "stem_patch_kernel")):
            print(r["Kernel_Name"], "grid", r["Grid_Size_X"], "workgroup", r["Workgroup_Size_X"], "lds", r["LDS_Block_Size"])
    sys.exit(0)

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from computervision_codes_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")
BF, F32 = torch.bfloat16, torch.float32
_n = [0]


def report(what, fn):
    try:
        r = fn()
        torch.cuda.synchronize()
        msg = "ok" if r is not None else "none"
    except RuntimeError as e:       # Mt4Error
        msg = str(e)
    print(f"{_n[0]:3d} {what}: {msg}", flush=True)
    _n[0] += 1


def conv(note, B, H, W, cin, cout, kh, kw, dt, *, tile=0, latency=False, stride=(1, 1), pad=(0, 0), dil=(1, 1), stats=False, od=None):
    x = torch.zeros(B, H, W, cin, device=dev, dtype=dt)
    w = torch.zeros(cout, ops.packed_k(cin, kh, kw, dt), device=dev, dtype=dt)
    bias = torch.zeros(cout, device=dev)
    sums = torch.zeros(ops.STAT_REPLICAS, 2, cout, device=dev, dtype=torch.float64) if stats else None

    def run():
        if latency:
            with ops.latency_tiles():
                return ops.conv_nhwc(x, w, bias, kh=kh, kw=kw, stride=stride, pad=pad, dil=dil, tile=tile, stat_sums=sums, out_dtype=od)
        return ops.conv_nhwc(x, w, bias, kh=kh, kw=kw, stride=stride, pad=pad, dil=dil, tile=tile, stat_sums=sums, out_dtype=od)
    report(f"{note} [{B}x{H}x{W}x{cin}->{cout} {kh}x{kw} {str(dt)[6:]} tile={-1 if latency else tile}]", run)


def gemm(note, M, cin, cout, dt, **kw):      # 1x1: nsteps = cin * es / 128
    conv(note, M // 256 if M % 256 == 0 else 1, 1, 256 if M % 256 == 0 else M, cin, cout, 1, 1, dt, **kw)


def tcn(note, T, cin, cout, kw, dt, **k):    # 1 x kw over one video of T frames, 'same' padding: nsteps = ceil(kw * cin * es / 128)
    conv(note, 1, 1, T, cin, cout, 1, kw, dt, pad=(0, kw // 2), **k)


def stem(note, B, H, W, kh, cout, tile=0):   # the space-to-depth stem: runs of 4 pixels x 16 channels, kh x 1, valid
    x = torch.zeros(B, H, W, 16, device=dev, dtype=BF)
    w = torch.zeros(cout, ops.packed_k(64, kh, 1, BF), device=dev, dtype=BF)
    bias = torch.zeros(cout, device=dev)
    report(f"{note} [stem {B}x{H}x{W} kh={kh} ->{cout} tile={tile}]",
           lambda: ops.conv_nhwc(x, w, bias, kh=kh, kw=1, run_pixels=4, out_hw=(H - kh + 1, W - 3), relu=True, tile=tile))


def expand(note, B, H, W, cout3=512):
    x = torch.zeros(B, H, W, 128, device=dev, dtype=BF)
    w2 = torch.zeros(128, ops.packed_k(128, 3, 3, BF), device=dev, dtype=BF)
    w3 = torch.zeros(cout3, 128, device=dev, dtype=BF)
    res = torch.zeros(B, H, W, cout3, device=dev, dtype=BF)
    report(f"{note} [expand {B}x{H}x{W} ->{cout3}]",
           lambda: ops.conv3x3_expand(x, w2, torch.zeros(128, device=dev), w3, torch.zeros(cout3, device=dev), res))


ntiles = _lib.lib.mt4_conv_tile_count()

# ---- every explicit id (retired ids and ids that refuse the geometry included), and the two ids past the ends of the range
for t in range(1, ntiles + 1):
    conv("explicit, bf16 3x3", 3, 14, 14, 128, 128, 3, 3, BF, tile=t, pad=(1, 1))
for t in range(1, ntiles + 1):
    tcn("explicit, fp32 TCN 1x3", 256, 64, 64, 3, F32, tile=t)
conv("tile > count: EINVAL", 1, 14, 14, 64, 64, 3, 3, BF, tile=ntiles + 1, pad=(1, 1))
conv("tile < -1: EINVAL", 1, 14, 14, 64, 64, 3, 3, BF, tile=-2, pad=(1, 1))

# ---- the stem rule: tile 33 or (tile 0 and stem_patch_ok); a patch past 160 KB of LDS falls back to the generic tiles for tile 0 only
stem("stem_patch_ok, tile 0 -> stem kernel", 2, 67, 115, 4, 64)
stem("stem_patch_ok, tile 33", 2, 67, 115, 4, 64, tile=33)
stem("stem patch > 160 KB, tile 0 -> generic", 1, 8, 453, 8, 64)
stem("stem patch > 160 KB, tile 33 -> unsupported", 1, 8, 453, 8, 64, tile=33)
stem("HoWo < 256: not stem_patch_ok -> generic", 1, 11, 19, 4, 64)

# ---- the patch rule: tile 0, patch3x3_ok and cdiv(M, 256) * cdiv(Cout, 256) >= 256; then Cout <= 64 / <= 128 (W <= 31) / above
conv("patch: 258 tiles, Cout 64 -> 24", 21, 56, 56, 64, 64, 3, 3, BF, pad=(1, 1))
conv("patch: 245 tiles < 256 -> generic", 20, 56, 56, 64, 64, 3, 3, BF, pad=(1, 1))
conv("patch: Cout 72 > 64, W 31 -> 30", 68, 31, 31, 64, 72, 3, 3, BF, pad=(1, 1))
conv("patch: Cout 128, W 32 > 31 -> 32", 64, 32, 32, 64, 128, 3, 3, BF, pad=(1, 1))
conv("patch: Cout 136 > 128 -> 23", 68, 31, 31, 64, 136, 3, 3, BF, pad=(1, 1))
conv("patch: W 448, patch > 160 KB -> generic", 1, 147, 448, 64, 64, 3, 3, BF, pad=(1, 1))
conv("patch: stride 2, not patch3x3_ok -> generic", 84, 56, 56, 64, 64, 3, 3, BF, pad=(1, 1), stride=(2, 2))
conv("patch: fp32, not patch3x3_ok -> generic", 21, 56, 56, 32, 64, 3, 3, F32, pad=(1, 1))
conv("patch: latency caller, the rule holds for tile -1 too -> 24", 21, 56, 56, 64, 64, 3, 3, BF, pad=(1, 1), latency=True)

# ---- auto_tile(M, N, nsteps, es)
gemm("es 2, N >= 256, nsteps 1, tiles(13) = 256 -> 13", 128 * 256, 64, 256, BF)
gemm("tiles(13) = 254 -> on (nsteps 1, tiles(3) >= 1024 -> 3)", 127 * 256, 64, 256, BF)
gemm("es 2, N >= 256, nsteps 2, tiles(15) = 190 -> 17", 190 * 256, 128, 256, BF)
gemm("tiles(15) = 189 -> on (1: nsteps < 4, tiles(4) >= 256 -> 4)", 189 * 256, 128, 256, BF)
gemm("es 4, N >= 256: the 8-wave rules do not apply -> 1", 128 * 256, 128, 256, F32)
gemm("es 2, N 248 < 256 -> 1", 128 * 256, 256, 248, BF)
gemm("es 2, 64 < N <= 128, nsteps 1 < 4, tiles(20) = 2048 -> 20", 1024 * 256, 64, 128, BF)
gemm("tiles(20) = 2046 -> on (nsteps 1, tiles(3) >= 1024 -> 3)", 1023 * 256, 64, 128, BF)
conv("es 2, N 128, nsteps 4, tiles(19) = 2048 -> 19", 2048, 1, 259, 64, 128, 1, 4, BF)
conv("tiles(19) = 2047 -> on (1)", 2047, 1, 259, 64, 128, 1, 4, BF)
conv("es 2, N 128, nsteps 3 < 4, tiles(20) < 2048 -> 4", 512, 1, 258, 64, 128, 1, 3, BF)
gemm("nsteps 1, tiles(3) = 1024 -> 3", 65536, 32, 64, F32)
gemm("nsteps 1, tiles(3) = 1023 -> on (N <= 64, tiles(2) >= 256 -> 2)", 65472, 32, 64, F32)
gemm("N > 64, nsteps 4, tiles(1) = 256 -> 1", 32768, 128, 128, F32)
gemm("N > 64, nsteps 4, tiles(1) = 255, tiles(4) >= 256 -> 4", 32640, 128, 128, F32)
gemm("N > 64, nsteps 2 < 4, tiles(4) = 256 -> 4", 16384, 64, 128, F32)
gemm("N > 64, tiles(4) = 255 -> small tiles, nsteps 2 < 8 -> 6", 16320, 64, 128, F32)
gemm("32 < N <= 64, es 2, tiles(20) = 2048 -> 20", 2048 * 256, 128, 64, BF)
gemm("32 < N <= 64, es 2, tiles(20) = 2047 -> 2", 2047 * 256, 128, 64, BF)
gemm("32 < N <= 64, es 4, tiles(2) = 256 -> 2", 32768, 64, 64, F32)
gemm("32 < N <= 64, tiles(2) = 255, tiles(3) >= 256 -> 3", 32640, 64, 64, F32)
gemm("32 < N <= 64, tiles(3) = 255 -> small tiles -> 6", 16320, 64, 64, F32)
gemm("N 32: neither N block -> 6", 16320, 64, 32, F32)
gemm("nsteps 32, N > 32, tiles(3) = 192 -> 9", 192 * 64, 1024, 64, F32)
gemm("nsteps 32, tiles(3) = 191 -> 11", 191 * 64, 1024, 64, F32)
gemm("nsteps 31 < 32, tiles(3) = 192 -> 11", 192 * 64, 992, 64, F32)
gemm("nsteps 32, N 32 -> 11", 192 * 64, 1024, 32, F32)
tcn("few tiles, nsteps 6 < 8 -> 6", 256, 64, 64, 3, F32)
tcn("few tiles, nsteps 12 >= 8 -> 11", 256, 128, 64, 3, F32)

# ---- the latency overrides (tile -1)
tcn("latency, fast, fp32, 11, tiles(37) = 16 <= 256 -> 37", 256, 128, 64, 3, F32, latency=True)
tcn("latency, fp32, 11, tiles(37) = 256 -> 37", 4096, 128, 64, 3, F32, latency=True)
tcn("latency, fp32, 11, tiles(37) = 258 > 256, t64 = 65 < 192 -> 11", 4128, 128, 64, 3, F32, latency=True)
tcn("latency, not fast (CPT 12), 11 stays", 256, 48, 64, 7, F32, latency=True)
tcn("latency, bf16, 11, t64 = 4, 32x64 tiles 8 < 256 -> 11", 256, 256, 64, 3, BF, latency=True)
tcn("latency, bf16, 11, t64 = 128, 32x64 tiles = 256 -> 10", 8192, 256, 64, 3, BF, latency=True)
tcn("latency, bf16, 11, 32x64 tiles = 255 -> 11", 8160, 256, 64, 3, BF, latency=True)
tcn("latency, nsteps 6 < 8: 6 stays", 256, 64, 64, 3, F32, latency=True)
gemm("latency, 1, t128 = 256 < 512 -> 4", 32768, 128, 128, F32, latency=True)
gemm("latency, 1, t128 = 512 -> 1 stays", 65536, 128, 128, F32, latency=True)
gemm("latency, auto 4: no override", 16384, 64, 128, F32, latency=True)
tcn("latency, fp32 whole video, 9, t64 = 256 -> 40", 2000, 512, 512, 3, F32, latency=True)
tcn("latency, bf16 whole video, 11, t64 = 256 -> 41", 2000, 512, 512, 3, BF, latency=True)
tcn("latency, fp32, 11, t64 = 192 -> 40", 192 * 64, 128, 64, 3, F32, latency=True)
tcn("latency, fp32, 11, t64 = 191 -> 11", 191 * 64, 128, 64, 3, F32, latency=True)
tcn("latency, fp32, 11, t64 = 504 (the most the small tiles see) -> 40", 63 * 64, 128, 512, 3, F32, latency=True)
tcn("the same geometry, tile 0: 11", 2000, 512, 512, 3, BF)

# ---- stat_sums: generic and patch tiles, explicit and automatic; the launches that refuse them
conv("stat_sums, generic tile 2", 3, 14, 14, 64, 64, 3, 3, BF, pad=(1, 1), tile=2, stats=True)
conv("stat_sums, generic tile 2, fp32", 3, 14, 14, 64, 64, 3, 3, F32, pad=(1, 1), tile=2, stats=True)
conv("stat_sums, generic tile 9, not fast (Cin 24)", 3, 14, 14, 24, 64, 3, 3, BF, pad=(1, 1), tile=9, stats=True)
conv("stat_sums, patch tile 24", 3, 14, 14, 64, 64, 3, 3, BF, pad=(1, 1), tile=24, stats=True)
conv("stat_sums, auto -> patch 24", 21, 56, 56, 64, 64, 3, 3, BF, pad=(1, 1), stats=True)
conv("stat_sums, auto -> generic", 3, 14, 14, 64, 64, 3, 3, BF, pad=(1, 1), stats=True)
conv("stat_sums, K-split tile 35: unsupported", 3, 14, 14, 64, 64, 3, 3, BF, pad=(1, 1), tile=35, stats=True)
conv("stat_sums, generic tile 17 (16 waves)", 3, 14, 14, 64, 64, 3, 3, BF, pad=(1, 1), tile=17, stats=True)
conv("stat_sums, Cout 68: unsupported", 3, 14, 14, 64, 68, 3, 3, BF, pad=(1, 1), tile=2, stats=True)
conv("stat_sums, latency caller: unsupported", 3, 14, 14, 64, 64, 3, 3, BF, pad=(1, 1), latency=True, stats=True)

# ---- the other routes through the entry point
conv("generic, not fast (Cin 24), tile 0", 3, 14, 14, 24, 64, 3, 3, BF, pad=(1, 1))
conv("generic, bf16 in / fp32 out", 3, 14, 14, 64, 64, 3, 3, BF, pad=(1, 1), od=F32)


def second():
    x = torch.zeros(4, 14, 14, 256, device=dev, dtype=BF)
    x2 = torch.zeros(4, 28, 28, 128, device=dev, dtype=BF)
    w = torch.zeros(512, ops.packed_k(256, 1, 1, BF) + ops.packed_k(128, 1, 1, BF), device=dev, dtype=BF)
    return ops.conv_nhwc(x, w, torch.zeros(512, device=dev), kh=1, kw=1, relu=True, second=(x2, 2))


report("second K source [4x14x14x256 + 4x28x28x128 /2 -> 512]", second)
expand("fuse_expand: 258 tiles >= 256, W 28 <= 31 -> 128x128", 42, 28, 28)
expand("fuse_expand: 270 tiles, W 56 -> 256x128", 11, 56, 56)
expand("fuse_expand: 50 tiles < 256 -> the caller launches two convs", 8, 28, 28)

# Sides of comparisons that no descriptor reaches (kept as they are; listed so that nobody looks for the missing launches):
#   auto_tile: the third `tiles(1) >= fill` of the N > 64 block (tiles(4) >= tiles(1) always); `best == 5` and `best == 3` after the
#     most-blocks loop (the 32 x 32 tile has strictly the most blocks whenever a wider one is allowed), hence tile 10 from auto_tile and
#     kt = 36 in the first latency override;
#   latency overrides: `t64 >= 256` false with tile 1 (t64 >= t128 >= 256); `t64 <= 512` false (the small tiles are chosen only when
#     tiles(4) < 256, and t64 <= 2 tiles(4)); `tile == 11` false in the bf16 32 x 64 rule (tile 9 always has 192 <= t64 <= 512).
print("done", flush=True)
