"""GPU: `mt4_class_maps` -- the maps against a float64 evaluation under a derived bound, with guard words around the three outputs; range and
regions against `ops.class_regions_host` of the returned maps, to the bit; the hand-drawn maps of tests/class_map_patterns.py through the
device with operands that make every sum exact; and the bits of a frame's outputs in whichever batch and column range it travels."""
import functools

import numpy as np
import pytest
import torch

from class_map_patterns import FRACS, PATTERNS, bfs_region
from computervision_codes_amd import _lib, ops

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
GUARD = 64                                             # words on either side of every output
GUARD_WORD = 0x5A5AA5A5

# (C, H, W, B, ncol, col_lo): every value of C {8, 64, 512, 2048, 2056}, (H, W) {(1, 1), (1, 7), (8, 14), (12, 12), (32, 32)}, B {1, 3, 37},
# ncol {1, 6, 100, 131} and col_lo {0, 31} -- C = 8 and 2056 end in a short K-chunk, 8 x 14 and 12 x 12 in a short pixel tile, 32 x 32 takes the
# four-wave region kernel, 100 and 131 columns leave column slots empty
CASES = [(8, 1, 1, 1, 1, 0), (8, 1, 7, 3, 6, 31), (64, 8, 14, 3, 100, 0), (512, 8, 14, 37, 6, 0), (512, 12, 12, 3, 131, 31), (2048, 8, 14, 3, 100, 31),
         (2056, 12, 12, 1, 131, 0), (2056, 32, 32, 3, 6, 31), (64, 32, 32, 37, 131, 0), (2048, 1, 7, 37, 1, 31), (512, 32, 32, 1, 100, 0),
         (2056, 8, 14, 1, 1, 0)]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _guarded(n, dtype, dev):
    """a buffer of n words between two runs of guard words -> (whole buffer as int32, the view of the n words)"""
    whole = torch.full((n + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + n].view(dtype)


def _guards_untouched(whole, n):
    return bool((whole[:GUARD] == GUARD_WORD).all()) and bool((whole[GUARD + n:] == GUARD_WORD).all())


def _call(feat, w, col_lo, ncol, frac):
    """the entry point itself, outputs between guard words -> (maps, regions, range, guards untouched)"""
    b, h, wd, c = feat.shape
    dev = feat.device
    nm, nr, ng = b * ncol * h * wd, b * ncol * 8, b * ncol * 2
    (wm, maps), (wr, regions), (wg, rng) = _guarded(nm, torch.float32, dev), _guarded(nr, torch.int32, dev), _guarded(ng, torch.float32, dev)
    assert maps.data_ptr() == wm.data_ptr() + 4 * GUARD
    _lib.check(_lib.lib.mt4_class_maps(feat.data_ptr(), ops.dt_code(feat.dtype), w.data_ptr(), col_lo, ncol, b, h, wd, c, frac, maps.data_ptr(),
                                       regions.data_ptr(), rng.data_ptr(), torch.cuda.current_stream().cuda_stream), "mt4_class_maps")
    torch.cuda.synchronize()
    ok = _guards_untouched(wm, nm) and _guards_untouched(wr, nr) and _guards_untouched(wg, ng)
    return maps.view(b, ncol, h, wd), regions.view(b, ncol, 8), rng.view(b, ncol, 2), ok


@functools.lru_cache(maxsize=None)
def _run(case, dt):
    """ONE launch per case and dtype, shared by the tests below; the float64 evaluation runs on the device too"""
    c, h, wd, b, ncol, col_lo = case
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 + 7 * CASES.index(case))
    feat = torch.randn((b, h, wd, c), generator=g).to(DTYPES[dt]).to(dev)
    w = torch.randn((col_lo + ncol + 3, c), generator=g).to(dev)
    maps, regions, rng, ok = _call(feat, w, col_lo, ncol, 0.5)
    f64, w64 = feat.double(), w[col_lo:col_lo + ncol].double()
    ref = torch.einsum("byxk,jk->bjyx", f64, w64)
    mag = torch.einsum("byxk,jk->bjyx", f64.abs(), w64.abs())
    return dict(maps=maps, regions=regions, range=rng, guards=ok, ref=ref, mag=mag, direct=ops.class_maps(feat, w, col_lo, ncol, 0.5))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "C{}_{}x{}_B{}_n{}_lo{}".format(*c))
def test_maps_against_float64(cuda, case, dt):
    """|m - m64| <= gamma_C sum_k |w_k f_k|, gamma_C = C u / (1 - C u), u = 2^-24: the standard bound of a length-C inner product in fp32, which
    holds for ANY summation order and with or without FMA (Higham, Accuracy and Stability, 3.1) -- derived, not measured; the bf16 map is widened
    exactly, so the same bound holds on the widened values"""
    r = _run(case, dt)
    c = case[0]
    gamma = c * U / (1.0 - c * U)
    err = (r["maps"].double() - r["ref"]).abs()
    worst = float((err / r["mag"].clamp_min(1e-300)).max())
    print(f"class_maps {case} {dt}: max |m - m64| / sum|w f| = {worst:.3e}, gamma_C = {gamma:.3e}")
    assert r["guards"], "a word outside maps / regions / range was written"
    assert bool((err <= gamma * r["mag"]).all()), (case, dt, worst, gamma)
    for got, want in zip(r["direct"], (r["maps"], r["regions"], r["range"])):          # `ops.class_maps` allocates its own outputs: the same bits
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "C{}_{}x{}_B{}_n{}_lo{}".format(*c))
def test_regions_and_range_equal_the_host_restatement(cuda, case, dt):
    r = _run(case, dt)
    regions, rng = ops.class_regions_host(r["maps"], 0.5)
    assert torch.equal(r["regions"].cpu(), torch.from_numpy(regions))
    assert torch.equal(r["range"].cpu(), torch.from_numpy(rng))
    assert bool((r["regions"][..., 7] == 0).all())


@pytest.mark.parametrize("frac", [0.0, 0.2, 1.0])
def test_regions_at_other_fractions_equal_the_host_restatement(cuda, frac):
    c, h, wd, b, ncol = 64, 12, 12, 3, 6
    g = torch.Generator().manual_seed(5)
    feat, w = torch.randn((b, h, wd, c), generator=g).to(cuda), torch.randn((ncol, c), generator=g).to(cuda)
    maps, regions, rng = ops.class_maps(feat, w, 0, ncol, frac)
    want_r, want_g = ops.class_regions_host(maps, frac)
    assert torch.equal(regions.cpu(), torch.from_numpy(want_r)) and torch.equal(rng.cpu(), torch.from_numpy(want_g))
    assert torch.equal(maps, ops.class_maps(feat, w, 0, ncol, 0.5)[0])                 # the maps do not depend on frac


@pytest.mark.parametrize("name,dt", [(n, dt) for n in sorted(PATTERNS) for dt in sorted(DTYPES) if PATTERNS[n][1] or dt == "fp32"])
def test_exact_operands_reproduce_the_drawn_maps(cuda, name, dt):
    """one-hot weight rows and small-integer features: every product is the feature or zero and every partial sum is exact, so whatever the
    summation order map j is the drawing times (j + 1) minus j, bit for bit (8 columns from ONE launch; a drawing that is not made of integers
    goes through unscaled, in fp32 only -- bf16 would round it).  Peak, box and area come from the test's own search on the drawing."""
    m, integers = PATTERNS[name]
    h, wd = m.shape
    scale = [(j + 1, j) if integers else (1, 0) for j in range(8)]
    drawn = np.stack([m * a - b for a, b in scale]).astype(np.float32)                 # [8, h, w]: what column j must hold
    feat = torch.from_numpy(np.ascontiguousarray(drawn.transpose(1, 2, 0))[None]).to(DTYPES[dt]).to(cuda)
    assert torch.equal(feat.float().cpu()[0].permute(2, 0, 1), torch.from_numpy(drawn))          # the operands are exact in this dtype
    w = torch.eye(8, device=cuda)
    for frac in FRACS:
        maps, regions, rng = ops.class_maps(feat, w, 0, 8, frac)
        assert np.array_equal(maps[0].cpu().numpy().view(np.uint32), drawn.view(np.uint32)), (name, frac)
        for j in range(8):
            want, (mn, mx) = bfs_region(drawn[j], frac)
            assert tuple(regions[0, j].tolist()) == want, (name, frac, j)
            assert rng[0, j, 0].item() == mn and rng[0, j, 1].item() == mx


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("hw", [(8, 14), (12, 12), (2, 3)])
def test_a_frames_bits_do_not_depend_on_its_batch_or_column_range(cuda, dt, hw):
    c, b, row = 512, 37, 20
    g = torch.Generator().manual_seed(9)
    feat = torch.randn((b,) + hw + (c,), generator=g).to(DTYPES[dt]).to(cuda)
    w = torch.randn((131, c), generator=g).to(cuda)
    alone = ops.class_maps(feat[row:row + 1].contiguous(), w, 0, 100, 0.5)
    batch = ops.class_maps(feat, w, 0, 100, 0.5)
    for a, bt in zip(alone, batch):
        assert torch.equal(a[0], bt[row])
    for lo, n, col in ((33, 1, 33), (31, 6, 33), (0, 131, 33), (2, 64, 33)):               # column 33 alone, and inside other ranges
        part = ops.class_maps(feat, w, lo, n, 0.5)
        for a, bt in zip(part, batch):
            assert torch.equal(a[:, col - lo], bt[:, col]), (lo, n)
