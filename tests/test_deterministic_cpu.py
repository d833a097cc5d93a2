"""CPU: the host side of --deterministic -- the plan queries of the deterministic entry points (host-only: no device is touched) against the
launch rules replicated here from csrc/train_kernels.hip, the workspace refusals of the wrappers, the flag on the four trainers' parsers and the
host fold (`ops.fold_parts_host`) that the GPU tests hold the kernels' fold order against."""
import ctypes

import numpy as np
import pytest
import torch

from computervision_codes_amd import _lib, drivers, ops


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the launch rules, replicated
def wgrad1d_parts(b, t, cout, cin, taps):
    """parts of `mt4_wgrad_conv1d_det_f32` = the row splits of `mt4_wgrad_conv1d_f32` (csrc/train_kernels.hip, `wgrad_conv1d_parts`): about 1024
    workgroups in all, at least 256 rows per split, rows per split rounded up to the 32-row chunk"""
    kpad = _cdiv(taps * _cdiv(cin * 4, 16), 8) * 8 * 4                  # mt4_conv_packed_k(cin, 1, taps, MT4_F32)
    m, tiles = b * t, _cdiv(kpad, 64) * _cdiv(cout, 64)
    splits = max(1, min(_cdiv(1024, tiles), _cdiv(m, 256)))
    rps = _cdiv(_cdiv(m, splits), 32) * 32
    return _cdiv(m, rps), kpad


def colsum_parts(m, c):
    """row slabs of `mt4_colsum_f32` (`colsum_parts`): 64 rows per slab, at most ceil(1024 / column blocks) slabs"""
    return max(1, min(_cdiv(m, 64), _cdiv(1024, _cdiv(c, 64))))


def bce_parts(m):
    return min(_cdiv(m, 64), 64)                                         # `bce_logits_parts`


WGRAD1D_SHAPES = [(1, 1000, 64, 64, 3), (1, 200, 64, 64, 3), (1, 600, 64, 64, 3), (1, 600, 64, 32, 1), (1, 2000, 512, 512, 3), (1, 2000, 132, 512, 1),
                  (5, 500, 200, 100, 3), (3, 700, 40, 20, 3), (10, 2000, 200, 136, 1), (1, 1, 4, 4, 1), (1, 255, 64, 64, 1), (1, 257, 64, 64, 1)]


def test_wgrad_conv1d_plan_matches_the_launch_rule():
    # the two shapes the GPU tests name: 1000 frames split four ways (ceil(1000 / 256) = 4 splits of 256 rows), 200 frames do not split
    assert ops.wgrad_conv1d_plan(1, 1000, 64, 64, 3, True).nparts == 4 and ops.wgrad_conv1d_plan(1, 200, 64, 64, 3, True).nparts == 1
    for b, t, cout, cin, taps in WGRAD1D_SHAPES:
        for bias in (False, True):
            p = ops.wgrad_conv1d_plan(b, t, cout, cin, taps, bias)
            assert p == ops.wgrad_conv1d_plan(b, t, cout, cin, taps, bias)                      # the same answer twice
            nparts, kpad = wgrad1d_parts(b, t, cout, cin, taps)
            assert kpad == ops.packed_k(cin, 1, taps, torch.float32)
            assert (p.form, p.nparts, p.part_elems) == (0, nparts, cout * kpad + (cout if bias else 0)), (b, t, cout, cin, taps, bias, p)
            assert p.bytes == p.nparts * p.part_elems * 4
            assert p.part_elems % 4 == 0                                                          # every part starts 16-byte aligned


def test_colsum_and_bce_plans_match_the_launch_rules():
    assert ops.colsum_plan(1000, 512).nparts == 16 and ops.bce_logits_plan(600, 100).nparts == 10 and ops.bce_logits_plan(200, 131).nparts == 4
    for m, c in [(1000, 512), (333, 68), (40000, 68), (70000, 200), (7, 4), (1, 1), (64, 64), (65, 65)]:
        p = ops.colsum_plan(m, c)
        assert p == ops.colsum_plan(m, c) and (p.form, p.nparts, p.part_elems) == (0, colsum_parts(m, c), c) and p.bytes == p.nparts * c * 4
        q = ops.bce_logits_plan(m, c)
        assert q == ops.bce_logits_plan(m, c) and (q.form, q.nparts, q.part_elems) == (0, bce_parts(m), c) and q.bytes == q.nparts * c * 4


def test_plan_queries_refuse_bad_shapes():
    with pytest.raises(_lib.Mt4Error):
        ops.wgrad_conv1d_plan(1, 0, 64, 64, 3)
    with pytest.raises(_lib.Mt4Error):
        ops.wgrad_conv1d_plan(1, 100, 64, 30, 3)                       # Cin % 4: what the launch itself refuses
    with pytest.raises(_lib.Mt4Error):
        ops.colsum_plan(0, 8)
    with pytest.raises(_lib.Mt4Error):
        ops.bce_logits_plan(5, 0)


def test_temporal_workspace_holds_for_every_length():
    """`TencoTrainer.workspace_bytes` sizes the one workspace from plans at 2^24 frames: the parts of a conv1d weight gradient stop growing at
    ceil(1024 / tiles), so no shorter video needs more.  Layers of the full temporal head (512 maps): dilated 512 -> 512 x 3 taps, 1 x 1, the heads."""
    big = 1 << 24
    worst = 0
    for cout, cin, taps in [(512, 512, 3), (512, 512, 1), (132, 512, 1)]:
        cap = ops.wgrad_conv1d_plan(1, big, cout, cin, taps, True)
        assert cap.nparts == _cdiv(1024, _cdiv(cap.part_elems // cout - 1, 64) * _cdiv(cout, 64))
        for t in [1, 7, 255, 256, 257, 600, 1000, 2000, 2047, 4096, 5000, 12345, 100000, 1 << 20]:
            assert ops.wgrad_conv1d_plan(1, t, cout, cin, taps, True).bytes <= cap.bytes, (cout, cin, taps, t)
        worst = max(worst, cap.bytes)
    assert ops.bce_logits_plan(big, 131).bytes == 64 * 131 * 4 and ops.bce_logits_plan(5000, 131).bytes <= 64 * 131 * 4
    print(f"temporal head, 512 maps: workspace {worst} bytes = {worst / 2 ** 20:.1f} MiB")
    assert worst == 6 * (512 * 1536 + 512) * 4                          # 18.0 MiB: six parts of the dilated layer's dW and bias gradient


# ------------------------------------------------------------------------------------------------ refusals
def test_wrappers_refuse_a_short_workspace_before_any_launch():
    plan = ops.wgrad_conv1d_plan(1, 1000, 64, 64, 3, True)
    with pytest.raises(ValueError, match="workspace"):
        ops.check_workspace(torch.empty(plan.bytes // 4 - 1), plan, "wgrad_conv1d")              # one float short (a CPU tensor: the size comes first)
    with pytest.raises(ValueError, match="workspace"):
        ops.check_workspace(torch.empty(2, plan.bytes // 4)[:, ::2], plan, "wgrad_conv1d")       # not contiguous
    with pytest.raises(_lib.Mt4Error):
        ops.check_workspace(torch.empty(plan.bytes // 4 + 4), plan, "wgrad_conv1d")              # large enough, but not on the device


def test_entry_points_refuse_null_and_short_workspaces_without_a_device():
    """the C entry points return before any launch (no GPU here: a launch would fail differently)"""
    lib, buf = _lib.lib, ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    assert lib.mt4_fold_parts_f32(None, 3, 8, 8, p, 0, None) == -1 and lib.mt4_fold_parts_f32(p, 0, 8, 8, p, 0, None) == -1
    assert lib.mt4_fold_parts_f64(p, 3, 8, 4, p, 0, None) == -1                                  # a stride below n
    assert lib.mt4_fold_parts_chunked_f64(p, 3, 8, 4, p, 0, None) == -1 and lib.mt4_fold_parts_chunked_f32(None, 3, 8, 8, p, 0, None) == -1
    assert lib.mt4_wgrad_conv1d_det_f32(p, p, p, 1, 1000, 64, 64, 3, 2, 2, 1, p, None, 1 << 30, None) == -1          # NULL workspace
    need = ops.wgrad_conv1d_plan(1, 1000, 64, 64, 3, True).bytes
    assert lib.mt4_wgrad_conv1d_det_f32(p, p, p, 1, 1000, 64, 64, 3, 2, 2, 1, p, p, need - 4, None) == -1            # four bytes short
    assert lib.mt4_colsum_det_f32(p, p, 1000, 512, 512, 0, None, 1 << 30, None) == -1
    assert lib.mt4_colsum_det_f32(p, p, 1000, 512, 512, 0, p, ops.colsum_plan(1000, 512).bytes - 4, None) == -1
    assert lib.mt4_bce_logits_det_f32(p, p, p, p, p, 600, 100, 100, 100, None, 1 << 30, None) == -1
    assert lib.mt4_bce_logits_det_f32(p, p, p, p, p, 600, 100, 100, 100, p, ops.bce_logits_plan(600, 100).bytes - 4, None) == -1


def test_spatial_entry_points_refuse_null_and_short_workspaces_without_a_device():
    """the deterministic entries of the spatial stage, at shapes whose plans have several parts: a NULL workspace, one a part element short of the
    plan's bytes and an empty one are all MT4_EINVAL before any launch -- the bytes the plan query names are the bytes the launch asks for"""
    lib, buf = _lib.lib, ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    F32, BF16 = _lib.MT4_F32, _lib.MT4_BF16
    bn, m, c = ops.bn_plan(200, 64), 200, 64
    (wb, wh, ww, wcin, wcout, wk), (_, wparts) = WGRAD2D_TABLE[0]                                 # 2, 24 x 24, 64 -> 64, 3 x 3 (pad 1): 5 parts
    w32 = ops.wgrad_conv2d_plan(wb, wh, ww, wcout, wcin, wk, wk)
    w16 = ops.wgrad_conv2d_bf16_plan(2, 16, 32, 64, 64, 3, 1)                                     # the 3 x 3 base shape of the GPU tests: 16 parts
    assert (bn.nparts, w32.nparts, w16.nparts) == (4, wparts, 16)
    cases = [("mt4_bn_stats_det_f32", bn, (p, p, p, p, None, None, m, c, 0.1, 1e-5)),
             ("mt4_bn_stats_det_t", bn, (p, BF16, p, p, p, None, None, m, c, 0.1, 1e-5)),
             ("mt4_bn_stats_det_t", bn, (p, F32, p, p, p, None, None, m, c, 0.1, 1e-5)),
             ("mt4_bn_backward_det_f32", bn, (p, p, p, p, p, p, p, p, p, None, p, p, m, c, 1)),
             ("mt4_bn_backward_det_t", bn, (p, p, p, BF16, p, p, p, p, p, p, None, p, p, m, c, 1)),
             ("mt4_bn_backward_det_t", bn, (p, p, p, F32, p, p, p, p, p, p, None, p, p, m, c, 2)),
             ("mt4_wgrad_conv2d_det_f32", w32, (p, p, p, wb, wh, ww, wcin, wh, ww, wcout, wk, wk, 1, 1, 1, 1, 1, 1, 0)),
             ("mt4_wgrad_conv2d_det_bf16", w16, (p, p, p, 2, 16, 32, 64, 16, 32, 64, 3, 1, 1)),
             ("mt4_bce_logits_pw_det_f32", ops.bce_logits_pw_plan(130, 100), (p, p, None, p, p, p, 130, 100, 100, 100)),
             ("mt4_distill_kl_det_f32", ops.distill_kl_plan(5, 10), (p, p, p, p, 5, 10, 10, 10, 4.0, 1.0, 1)),
             ("mt4_mse_det_f32", ops.mse_plan(1000), (p, p, p, p, 1000, 1.0))]
    for name, plan, args in cases:
        assert plan.nparts > 1, name                                                              # several parts: the formula matters
        esize = plan.bytes // (plan.nparts * plan.part_elems)
        assert esize == (8 if "_bn_" in name else 4) and plan.bytes == plan.nparts * plan.part_elems * esize
        fn = getattr(lib, name)
        assert fn(*args, None, 1 << 30, None) == -1, name                                         # NULL workspace
        assert fn(*args, p, plan.bytes - esize, None) == -1, name                                 # one element short
        assert fn(*args, p, 0, None) == -1, name                                                  # empty


# ------------------------------------------------------------------------------------------------ the flag
@pytest.mark.parametrize("stage", ["spatial_cnn", "spatial_transformer", "mstct", "tenco"])
def test_deterministic_flag_is_declared_off_by_default_and_refused_where_not_covered(stage, capsys):
    p = drivers._parser(stage, True)
    assert p.parse_known_args([])[0].deterministic is False
    F, rest = p.parse_known_args(["--deterministic"])
    assert F.deterministic is True and rest == []                        # declared: not one of the flags parse_known_args drops in silence
    assert drivers._deterministic(stage, p.parse_known_args([])[0]) is False
    if stage in ("spatial_cnn", "tenco"):
        assert drivers._deterministic(stage, F) is True
        assert capsys.readouterr().out.count("--deterministic") == 1     # said once at start
        return
    with pytest.raises(NotImplementedError, match="sequence trainers' reductions are not covered yet") as e:
        drivers._deterministic(stage, F)
    assert "seq_train_kernels.hip" in str(e.value)


def test_sequence_trainers_refuse_the_flag_before_any_model_is_built():
    """no GPU and no dataset here: anything past the refusal would fail differently"""
    with pytest.raises(NotImplementedError, match="--deterministic"):
        drivers.spatial_transformer_train(["-t", "--deterministic", "--data_dir", "/nonexistent"])
    with pytest.raises(NotImplementedError, match="--deterministic"):
        drivers._mstct_train(drivers._parser("mstct", True).parse_known_args(["-t", "--deterministic", "--data_dir", "/nonexistent"])[0])


# ------------------------------------------------------------------------------------------------ the host fold
def test_fold_parts_host_is_sequential_in_the_element_type():
    """three parts whose three orders give three different fp32 sums: 1, -3 x 2^-25, 2^-24"""
    a, b, c = 1.0, -3 * 2.0 ** -25, 2.0 ** -24
    sums = [float(ops.fold_parts_host(torch.tensor([[x], [y], [z]], dtype=torch.float32))[0]) for x, y, z in ((a, b, c), (a, c, b), (b, c, a))]
    assert [s.hex() for s in sums] == ["0x1.fffffe0000000p-1", "0x1.fffffc0000000p-1", "0x1.0000000000000p+0"]
    f = np.float32
    assert sums == [float(f(f(f(x) + f(y)) + f(z))) for x, y, z in ((a, b, c), (a, c, b), (b, c, a))]
    # fp64 parts are added in fp64: all three orders are exact there
    assert len({float(ops.fold_parts_host(torch.tensor([[x], [y], [z]], dtype=torch.float64))[0]) for x, y, z in ((a, b, c), (a, c, b), (b, c, a))}) == 1
    # accumulate_into: dst + (the folded parts), the parts first
    parts = torch.tensor([[a, 2.0], [b, 3.0], [c, 4.0]], dtype=torch.float32)
    dst = torch.tensor([2.0 ** -24, 1.0])
    got = ops.fold_parts_host(parts, dst)
    assert float(got[0]) == float(f(f(2.0 ** -24) + f(sums[0]))) and float(got[1]) == 10.0
    # the chunked order (`mt4_fold_parts_chunked_*`): 16 chunks of ceil(nparts / 16) parts.  Up to 16 parts it is the sequential fold; 32 parts of
    # (1, -3 x 2^-25, 2^-24, ...) pair up as (a + b), (c + a), (b + c), ... before the pairs are added: another float than the sequential sum
    seq = torch.tensor([[a], [b], [c]] * 5 + [[a]], dtype=torch.float32)
    assert torch.equal(ops.fold_parts_host(seq, chunked=True), ops.fold_parts_host(seq))
    many = torch.tensor([[a], [b], [c]] * 11, dtype=torch.float32)[:32]
    pairs = torch.stack([ops.fold_parts_host(many[k:k + 2]) for k in range(0, 32, 2)])
    assert torch.equal(ops.fold_parts_host(many, chunked=True), ops.fold_parts_host(pairs))
    assert float(ops.fold_parts_host(many, chunked=True)[0]) != float(ops.fold_parts_host(many)[0])
    one = torch.tensor([[5.0, 6.0]])
    assert torch.equal(ops.fold_parts_host(one), one[0]) and ops.fold_parts_host(one) is not one[0]    # one part is valid; a copy


# ------------------------------------------------------------------------------------------------ the spatial stage's plans
# (b, ho, wo, cin, cout, k) -> (form, parts): worked out by hand from the dispatch of `mt4_wgrad_conv2d_f32` (csrc/train2d_kernels.hip, `wgrad32_parts`):
# max_splits = ceil(M / 256), M = b ho wo; a wide form needs tiles x max_splits >= 512; splits = min(ceil(768 | 1024 / tiles), max_splits); rows per
# split rounded up to 32.  Kpad in floats.
#   2, 24 x 24,   64 ->  64, 3 x 3 (Kpad  576): M   1152, max 5; <1,2>: 5 x 1 x 5 = 25 < 512           -> 64 x 64, 9 tiles, min(114, 5)    -> 5 parts
#   4, 30 x 30,  256 -> 256, 3 x 3 (Kpad 2304): M   3600, max 15; <2,2>: 18 x 2 x 15 = 540             -> wide <2,2>, 36 tiles, min(22, 15) -> 15
#   8, 30 x 30,  256 ->  64, 3 x 3 (Kpad 2304): M   7200, max 29; <1,2>: 18 x 1 x 29 = 522             -> wide <1,2>, 18 tiles, min(43, 29) -> 29
#   2, 256 x 256, 16 -> 128, 1 x 1 (Kpad   32): M 131072, max 512; <2,1>: 1 x 1 x 512 = 512            -> wide <2,1>, 1 tile, min(768, 512) -> 512
WGRAD2D_TABLE = [((2, 24, 24, 64, 64, 3), ("64x64", 5)), ((4, 30, 30, 256, 256, 3), ("wide<2,2>", 15)), ((8, 30, 30, 256, 64, 3), ("wide<1,2>", 29)),
                 ((2, 256, 256, 16, 128, 1), ("wide<2,1>", 512))]


def wgrad2d_rule(b, ho, wo, cin, cout, k):
    kpad = _cdiv(k * k * _cdiv(cin * 4, 16), 8) * 8 * 4
    m = b * ho * wo
    max_splits = _cdiv(m, 256)
    fills = lambda bm, bn: _cdiv(kpad, bn) * _cdiv(cout, bm) * max_splits >= 512
    form, bm, bn = "64x64", 64, 64
    if cout > 64 and kpad > 64 and fills(128, 128):
        form, bm, bn = "wide<2,2>", 128, 128
    elif kpad >= 128 and fills(64, 128):
        form, bn = "wide<1,2>", 128
    elif cout > 64 and fills(128, 64):
        form, bm = "wide<2,1>", 128
    tiles = _cdiv(kpad, bn) * _cdiv(cout, bm)
    splits = max(1, min(_cdiv(1024 if form == "64x64" else 768, tiles), max_splits))
    rps = _cdiv(_cdiv(m, splits), 32) * 32
    return form, _cdiv(m, rps), kpad


def test_wgrad_conv2d_plan_holds_the_hand_derived_table():
    for (b, ho, wo, cin, cout, k), (form, parts) in WGRAD2D_TABLE:
        p = ops.wgrad_conv2d_plan(b, ho, wo, cout, cin, k, k)
        assert p == ops.wgrad_conv2d_plan(b, ho, wo, cout, cin, k, k)
        assert (ops.WGRAD2D_FORMS[p.form], p.nparts) == (form, parts), ((b, ho, wo, cin, cout, k), p)
        assert wgrad2d_rule(b, ho, wo, cin, cout, k)[:2] == (form, parts)
        assert p.part_elems == cout * ops.packed_k(cin, k, k, torch.float32) and p.bytes == p.nparts * p.part_elems * 4
    from test_gpu_f32_train_kernels import WGRAD2D_CASES, _out_size                  # the existing kernel test's shapes: the rule, everywhere
    for b, h, w, cin, cout, k, s, pd, d in WGRAD2D_CASES + [(3, 16, 12, 64, 128, 3, (2, 2), (1, 1), (1, 1)), (3, 64, 64, 64, 128, 3, (2, 2), (1, 1), (1, 1))]:
        ho, wo = _out_size(h, k, s[0], pd[0], d[0]), _out_size(w, k, s[1], pd[1], d[1])
        p = ops.wgrad_conv2d_plan(b, ho, wo, cout, cin, k, k)
        form, parts, kpad = wgrad2d_rule(b, ho, wo, cin, cout, k)
        assert (ops.WGRAD2D_FORMS[p.form], p.nparts, p.part_elems) == (form, parts, cout * kpad)


def wgrad_bf16_rule(b, ho, wo, cout, cin, k, stride):
    """`mt4_wgrad_conv2d_bf16`'s dispatch and `launch_wgrad`'s split: spatial tiles of TH x 16 output pixels, 256 x OCC workgroups aimed at"""
    m2, n2 = cout > 64, cin > 64
    if k == 1 and stride == 1:
        form, bmt, bnt = ("1x1s1<2,2>", 2, 2) if (m2 and n2) else ("1x1s1<2,1>", 2, 1) if m2 else ("1x1s1<1,2>", 1, 2) if n2 else ("1x1s1<1,1>", 1, 1)
    elif k == 1:
        form, bmt, bnt = ("1x1s2<2,1>", 2, 1) if m2 else ("1x1s2<1,1>", 1, 1)
    else:
        form, bmt, bnt = ("3x3s1" if stride == 1 else "3x3s2"), 1, 1
    th, occ = (8, 2) if k == 1 else (4, 3)
    ntiles = b * _cdiv(ho, th) * _cdiv(wo, 16)
    pairs = _cdiv(cout, 64 * bmt) * _cdiv(cin, 64 * bnt) * k
    return form, max(1, min(_cdiv(256 * occ, pairs), ntiles))


def test_bf16_wgrad_bn_and_loss_plans_match_their_launch_rules():
    seen = set()
    for cout, cin, k, stride in [(128, 128, 1, 1), (128, 64, 1, 1), (64, 128, 1, 1), (64, 64, 1, 1), (128, 64, 1, 2), (64, 64, 1, 2), (64, 64, 3, 1), (64, 64, 3, 2),
                                 (72, 40, 3, 1), (2048, 512, 1, 1), (512, 512, 3, 1)]:
        for b, ho, wo in [(2, 16, 32), (64, 8, 14), (1, 3, 5)]:
            p = ops.wgrad_conv2d_bf16_plan(b, ho, wo, cout, cin, k, stride)
            assert p == ops.wgrad_conv2d_bf16_plan(b, ho, wo, cout, cin, k, stride)
            form, parts = wgrad_bf16_rule(b, ho, wo, cout, cin, k, stride)
            assert (ops.WGRAD2D_BF16_FORMS[p.form], p.nparts) == (form, parts), (cout, cin, k, stride, b, ho, wo, p)
            assert p.part_elems == cout * ops.packed_k(cin, k, k, torch.float32) and p.bytes == p.nparts * p.part_elems * 4
            seen.add(form)
    assert seen == set(ops.WGRAD2D_BF16_FORMS)                          # all eight forms
    # the base shape of the GPU tests: 2 x 16 x 32 output pixels = 8 tiles of 8 x 16 (1 x 1 forms), 16 tiles of 4 x 16 (3 x 3 forms)
    assert ops.wgrad_conv2d_bf16_plan(2, 16, 32, 64, 64, 1, 1).nparts == 8 and ops.wgrad_conv2d_bf16_plan(2, 16, 32, 64, 64, 3, 1).nparts == 16
    for m, c, slabs in [(200, 64, 4), (1031, 96, 17), (7, 100, 1), (2, 36, 1), (20000, 196, 128), (6000, 64, 94), (64 * 64 * 112, 64, 512)]:
        p = ops.bn_plan(m, c)                                           # 64-row slabs, at most ceil(512 / column blocks); float64 parts [2][C]
        assert p == ops.bn_plan(m, c) and (p.form, p.nparts, p.part_elems, p.bytes) == (0, slabs, 2 * c, slabs * 2 * c * 8), (m, c, p)
        assert slabs == max(1, min(_cdiv(m, 64), _cdiv(512, _cdiv(c, 64))))
    assert ops.bce_logits_pw_plan(200, 131) == ops.DetPlan(0, 4, 131, 4 * 131 * 4)
    assert ops.distill_kl_plan(70, 100) == ops.DetPlan(0, 70, 1, 280) and ops.mse_plan(5000) == ops.DetPlan(0, 20, 1, 80)
    with pytest.raises(_lib.Mt4Error):
        ops.wgrad_conv2d_bf16_plan(2, 16, 32, 64, 60, 1, 1)            # Cin % 8
    with pytest.raises(_lib.Mt4Error):
        ops.distill_kl_plan(4, 129)                                      # K > 128: what the launch itself refuses


def test_student_workspace_stays_far_below_a_gigabyte():
    """the largest workspace over every launch of a ResNet-18 / ResNet-50 step at batch 64, 256 x 448 (and batch 16, 384 x 384), both operand modes.
    By the split rules a launch has about 1 k workgroups with <= 196 KB of partial tile each; the cap is a condition, not a measurement."""
    from computervision_codes_amd.spatial_cnn_train import SpatialCnnTrainer
    for net in ("resnet18", "resnet50"):
        for dt in (torch.float32, torch.bfloat16):
            tr = SpatialCnnTrainer(net, device="cpu", operand_dtype=dt, deterministic=True)       # (no weights, no device: the plans are host-only)
            assert tr.epilogue_stats is False                            # deterministic mode: the statistics come from the separate pass
            for shape in ((64, 256, 448), (16, 384, 384)):
                n = tr.workspace_bytes(*shape)
                print(f"{net} {str(dt).split('.')[1]} batch {shape[0]} {shape[1]} x {shape[2]}: workspace {n} bytes = {n / 2 ** 20:.1f} MiB")
                assert n == tr.workspace_bytes(*shape) and 0 < n < 2 ** 30
    assert SpatialCnnTrainer("resnet50", device="cpu").deterministic is False
