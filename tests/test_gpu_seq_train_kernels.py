"""GPU: the kernels only the two teacher trainers (MS-TCT, Swin + Query2Label) and the hierarchical TeCNO trainer use -- strided batched GEMM,
softmax rows forward / backward, LayerNorm / GELU / depthwise-conv backward, GroupWiseLinear backward, the relative-position table gradient,
the pool / interpolation adjoints, DistillKL, the KD mixing and the derived-weight refresh -- element by element against float64.

Same conventions as test_gpu_f32_train_kernels.py: references are float64 of the same fp32 operands; every assertion is
`bf16_bounds.check_f32` (fp32 half-ulp + sqrt(k) 2^-24 acc64 + a stated allowance) or `check_exact`; operands carry power-of-two scales
(`pow2_ramp`) on an axis that is NOT reduced, so that ragged tail tiles hold the smallest values without the first terms of a sum dominating
every later rounding; each docstring names where the kernel rounds; every refusal that returns before a launch is asserted through `ops.lib`.
Short reductions (below 16 terms) count their roundings: n roundings of up to 2^-24 acc64 each are passed as k = n^2, since sqrt(n) is under
the worst case there and thousands of elements approach it.  The operand builders are shared with test_seq_bounds_cpu.py, which runs fp32
emulations of the kernels' order of operations (and of planted errors) through the same checks.
"""
import ctypes as C
import math

import pytest
import torch

from bf16_bounds import (GELU_APPROX_ERR, GELU_BWD_ERR, check_exact, check_f32, half_ulp_f32, layernorm_bwd_ref64, pow2_ramp, rne_bf16,
                         softmax_bwd_ref64, softmax_ref64)

gpu = pytest.mark.gpu
EPS = 2.0 ** -24
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -4          # include/mt4hip.h
FN_EPS = 4 * EPS                                    # expf / logf of the device library: four fp32 ulps (as test_bce_logits_per_element)
F32_MIN_NORMAL = 2.0 ** -126


def _u(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2 - 1


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _count_k(terms64):
    """per-element factor for `acc64` standing for sqrt(k) of a per-element term count: sqrt(n) from 16 terms on, n below (n roundings of up
    to 2^-24 acc64 each: the worst case, which short sums over thousands of elements approach)"""
    t = terms64.to(torch.float64)
    return torch.where(t < 16, t, torch.sqrt(t))


# ------------------------------------------------------------------------------------------------ strided batched GEMM
def _bview(t, off, nb0, nb1, rows, cols, s):
    return torch.as_strided(t.reshape(-1), (nb1, nb0, rows, cols), (s[1], s[0], s[2], s[3]), off)


def _run_bgemm(cuda, A, a_off, B, b_off, Cbuf, c_off, m, n, k, nb0, nb1, a_s, b_s, c_s, alpha, accumulate, what):
    """A, B, Cbuf: contiguous fp32 CPU buffers; the operands are the strided views at element offsets a_off / b_off / c_off.  A's rows are
    scaled by pow2_ramp(m) and B's columns by pow2_ramp(n) in place (neither is the reduced axis); with `accumulate` the written part of Cbuf
    is a base scaled element by element like the result.  MFMA fp32 chain: one rounding per K step, n = K (+ 1 with accumulate: alpha * acc is
    rounded before it is added) roundings of up to 2^-24 acc64 each: k = n from K = 16 on, and k = n^2 below (short reductions count their
    roundings: 4 x 4 x 4 products, hd = 12 and the 6 queries of the cross attention reach 0.95 to 1.01 of sqrt(K) 2^-24 acc64 on the device)."""
    from computervision_codes_amd import ops
    _bview(A, a_off, nb0, nb1, m, k, a_s).mul_(pow2_ramp(m)[:, None])
    _bview(B, b_off, nb0, nb1, k, n, b_s).mul_(pow2_ramp(n)[None, :])
    A64, B64 = _bview(A.double(), a_off, nb0, nb1, m, k, a_s), _bview(B.double(), b_off, nb0, nb1, k, n, b_s)
    al = _f32(alpha)
    ref, acc, n_round = al * (A64 @ B64), abs(al) * (A64.abs() @ B64.abs()), k + (1 if accumulate else 0)
    kk = n_round if k >= 16 else n_round * n_round
    written = torch.zeros(Cbuf.numel(), dtype=torch.bool)
    widx = _bview(torch.arange(Cbuf.numel()), c_off, nb0, nb1, m, n, c_s)
    written[widx.reshape(-1)] = True
    assert int(written.sum()) == nb0 * nb1 * m * n, "the C views of a case must not overlap"
    if accumulate:
        base = (_u(tuple(ref.shape), 99) * ref.abs()).float()
        Cbuf.reshape(-1)[widx.reshape(-1)] = base.reshape(-1)
        ref, acc = ref + base.double(), acc + base.double().abs()
    ad, bd, cd = A.to(cuda), B.to(cuda), Cbuf.to(cuda)
    ops.bgemm(ad.reshape(-1)[a_off:], bd.reshape(-1)[b_off:], cd.reshape(-1)[c_off:], m=m, n=n, k=k, nb0=nb0, nb1=nb1, a_strides=a_s, b_strides=b_s,
              c_strides=c_s, alpha=alpha, accumulate=accumulate)
    got = cd.cpu()
    check_f32(_bview(got, c_off, nb0, nb1, m, n, c_s), ref, acc64=acc, k=kk, what=what)
    check_exact(got.reshape(-1)[~written], Cbuf.reshape(-1)[~written], what=what + " elements of C outside the views")
    return got


BGEMM_MNK = [(1, 1, 1), (63, 65, 3), (64, 64, 16), (65, 63, 15), (70, 200, 17), (200, 70, 37), (1, 200, 144), (200, 1, 256), (64, 65, 256), (63, 64, 144),
             (65, 70, 1), (70, 63, 16), (200, 200, 37)]


@gpu
@pytest.mark.parametrize("a_kfast", [True, False])
@pytest.mark.parametrize("b_kfast", [True, False])
def test_bgemm_staging_and_ragged_tiles_per_element(cuda, a_kfast, b_kfast):
    """`bgemm_f32_kernel`: the four staging maps (A / B contiguous along k or along m / n), M and N of 1, 63, 64, 65, 70, 200 (ragged 64-tiles), K of
    1 .. 256 (ragged 16-steps, one step, many), 2 x 3 batches, overwrite and accumulate, alpha 1, 0.5 and 12^-0.5"""
    for i, (m, n, k) in enumerate(BGEMM_MNK):
        nb0, nb1 = 2, 3
        a_s = (m * k, nb0 * m * k, k, 1) if a_kfast else (m * k, nb0 * m * k, 1, m)
        b_s = (n * k, nb0 * n * k, 1, k) if b_kfast else (n * k, nb0 * n * k, n, 1)
        c_s = (m * n, nb0 * m * n, n, 1)
        for accumulate, alpha in ((False, 1.0), (True, 0.5), (False, 12 ** -0.5)):
            A, B, Cb = _u((nb1 * nb0 * m * k,), 100 + i), _u((nb1 * nb0 * k * n,), 200 + i), torch.full((nb1 * nb0 * m * n,), 7.0)
            _run_bgemm(cuda, A, 0, B, 0, Cb, 0, m, n, k, nb0, nb1, a_s, b_s, c_s, alpha, accumulate,
                       f"bgemm a_kfast={a_kfast} b_kfast={b_kfast} {(m, n, k)} alpha={alpha:.3f} acc={accumulate}")


@gpu
@pytest.mark.parametrize("hd,H,t,b", [(12, 4, 49, 3), (32, 2, 144, 2), (12, 8, 70, 2)])
def test_bgemm_mstct_call_forms_per_element(cuda, hd, H, t, b):
    """the six calls of `MstctTrainer._attention_fwd / _attention_bwd` with their stride tuples: head slices of q [B*T][C] and the packed kv
    [B*T][2C], scores [B][H][T][T]; results written into head / column slices of wider buffers (the other columns untouched bit for bit)"""
    c = hd * H
    sp, sq, skv = (t * t, H * t * t), (hd, t * c), (hd, t * 2 * c)
    q = lambda s: _u((b * t * c,), s)
    kv = lambda s: _u((b * t * 2 * c,), s)
    P = lambda s: _u((b * H * t * t,), s)
    w = f"mstct hd={hd} H={H} t={t} b={b}: "
    _run_bgemm(cuda, q(1), 0, kv(2), 0, torch.full((b * H * t * t,), 7.0), 0, t, t, hd, H, b, sq + (c, 1), skv + (1, 2 * c), sp + (t, 1), 1.0, False,
               w + "S = Q K^T")
    _run_bgemm(cuda, P(3), 0, kv(4), c, torch.full((b * t * c,), 7.0), 0, t, hd, t, H, b, sp + (t, 1), skv + (2 * c, 1), sq + (c, 1), 1.0, False, w + "O = P V")
    _run_bgemm(cuda, P(5), 0, q(6), 0, _u((b * t * 2 * c,), 7), c, t, hd, t, H, b, sp + (1, t), sq + (c, 1), skv + (2 * c, 1), 1.0, False, w + "dV = P^T dO")
    _run_bgemm(cuda, q(8), 0, kv(9), c, torch.full((b * H * t * t,), 7.0), 0, t, t, hd, H, b, sq + (c, 1), skv + (1, 2 * c), sp + (t, 1), 1.0, False,
               w + "dP = dO V^T")
    _run_bgemm(cuda, P(10), 0, kv(11), 0, torch.full((b * t * c,), 7.0), 0, t, hd, t, H, b, sp + (t, 1), skv + (2 * c, 1), sq + (c, 1), 1.0, False,
               w + "dQ = dS K")
    _run_bgemm(cuda, P(12), 0, q(13), 0, _u((b * t * 2 * c,), 14), 0, t, hd, t, H, b, sp + (1, t), sq + (c, 1), skv + (2 * c, 1), 1.0, False, w + "dK = dS^T Q")


@gpu
@pytest.mark.parametrize("hd,nh,nq,nk,nb,packed", [(32, 3, 49, 49, 4, True), (32, 4, 144, 144, 2, True), (12, 4, 6, 144, 3, False), (32, 8, 6, 144, 2, False)])
def test_bgemm_q2l_call_forms_per_element(cuda, hd, nh, nq, nk, nb, packed):
    """the six calls of `Q2LTrainer._attn_fwd / _attn_bwd`: Swin window attention on the packed qkv buffer [nb*N][3C] (q, k, v and their
    gradients are column slices of pitch 3C) and Query2Label cross attention (nq = 6 queries against nk = 144 memory rows, q of pitch C, k / v
    in a packed [nb*nk][2C]); alpha = hd^-0.5 (no power of two at hd = 12 or 32) on S, dQ and dK"""
    dout = hd * nh
    scale = hd ** -0.5
    sp, so = (nq * nk, nh * nq * nk), (hd, nq * dout)
    if packed:
        sq = sk = sv = 3 * dout
        qo, ko, vo = 0, dout, 2 * dout
        nqbuf = nkbuf = nb * nq * 3 * dout
    else:
        sq, sk, sv = dout, 2 * dout, 2 * dout
        qo, ko, vo = 0, 0, dout
        nqbuf, nkbuf = nb * nq * dout, nb * nk * 2 * dout
    P = lambda s: _u((nb * nh * nq * nk,), s)
    do = lambda s: _u((nb * nq * dout,), s)
    w = f"q2l hd={hd} nh={nh} nq={nq} nk={nk} nb={nb} packed={packed}: "
    _run_bgemm(cuda, _u((nqbuf,), 1), qo, _u((nkbuf,), 2), ko, torch.full((nb * nh * nq * nk,), 7.0), 0, nq, nk, hd, nh, nb, (hd, nq * sq, sq, 1), (hd,
               nk * sk, 1, sk),
               sp + (nk, 1), scale, False, w + "S = scale Q K^T")
    _run_bgemm(cuda, P(3), 0, _u((nkbuf,), 4), vo, torch.full((nb * nq * dout,), 7.0), 0, nq, hd, nk, nh, nb, sp + (nk, 1), (hd, nk * sv, sv, 1), (hd,
               nq * dout, dout, 1),
               1.0, False, w + "O = P V")
    _run_bgemm(cuda, P(5), 0, do(6), 0, _u((nkbuf,), 7), vo, nk, hd, nq, nh, nb, sp + (1, nk), so + (dout, 1), (hd, nk * sv, sv, 1), 1.0, False,
               w + "dV = P^T dO")
    _run_bgemm(cuda, do(8), 0, _u((nkbuf,), 9), vo, torch.full((nb * nh * nq * nk,), 7.0), 0, nq, nk, hd, nh, nb, so + (dout, 1), (hd, nk * sv, 1, sv),
               sp + (nk, 1), 1.0,
               False, w + "dP = dO V^T")
    _run_bgemm(cuda, P(10), 0, _u((nkbuf,), 11), ko, _u((nqbuf,), 12), qo, nq, hd, nk, nh, nb, sp + (nk, 1), (hd, nk * sk, sk, 1), (hd, nq * sq, sq, 1),
               scale, False,
               w + "dQ = scale dS K")
    _run_bgemm(cuda, P(13), 0, _u((nqbuf,), 14), qo, _u((nkbuf,), 15), ko, nk, hd, nq, nh, nb, sp + (1, nk), (hd, nq * sq, sq, 1), (hd, nk * sk, sk, 1),
               scale, False,
               w + "dK = scale dS^T Q")


@gpu
def test_bgemm_batch_limit_and_refusals(cuda):
    """nb0 * nb1 = 65535 (the grid's z limit) is accepted and every 4 x 4 x 4 product is right; 65536 is refused before any launch (C untouched),
    as are null pointers and non-positive sizes"""
    from computervision_codes_amd import ops
    nb0, nb1 = 255, 257
    A, B = _u((nb1 * nb0 * 16,), 1), _u((nb1 * nb0 * 16,), 2)
    _run_bgemm(cuda, A, 0, B, 0, torch.full((nb1 * nb0 * 16,), 7.0), 0, 4, 4, 4, nb0, nb1, (16, nb0 * 16, 4, 1), (16, nb0 * 16, 4, 1), (16, nb0 * 16, 4, 1),
               1.0, False,
               "bgemm 65535 batches")
    i64x4 = C.c_int64 * 4
    st = i64x4(16, 256 * 16, 4, 1)
    a, b = torch.zeros(256 * 256 * 16, device=cuda), torch.zeros(256 * 256 * 16, device=cuda)
    c0 = torch.full((256 * 256 * 16,), 7.0)
    c = c0.to(cuda)
    call = lambda *sz: ops.lib.mt4_bgemm_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), *sz, st, st, st, 1.0, 0, None)
    assert call(4, 4, 4, 256, 256) == EUNSUPPORTED
    assert call(0, 4, 4, 1, 1) == EINVAL and call(4, 0, 4, 1, 1) == EINVAL and call(4, 4, 0, 1, 1) == EINVAL and call(4, 4, 4, 0, 1) == EINVAL
    assert ops.lib.mt4_bgemm_f32(None, b.data_ptr(), c.data_ptr(), 4, 4, 4, 1, 1, st, st, st, 1.0, 0, None) == EINVAL
    torch.cuda.synchronize()
    check_exact(c.cpu(), c0, what="bgemm refusals leave C untouched")


# ------------------------------------------------------------------------------------------------ softmax rows
SOFTMAX_COLS = [1, 7, 40, 49, 63, 64, 65, 144, 256, 1000, 1024]
SOFTMAX_SCALES = [1.0, 0.3, 12 ** -0.5, -0.3, 0.125]
SWIN_MASK = -100.0


def softmax_inputs(rows, cols, amp, seed):
    """logits of amplitude `amp`; from three rows on: row 0 constant, row 1 with Swin's -100 mask on every second entry, row 2 with the mask on
    all but one entry"""
    s = _u((rows, cols), seed) * amp
    if rows >= 3:
        s[0] = 0.75 * amp
        s[1, 1::2] += SWIN_MASK
        s[2, :cols - 1] += SWIN_MASK
    return s


@gpu
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_rows_per_element(cuda, cols):
    """`softmax_rows_kernel`, in place: rounds v = scale s, x = v - max, e = __expf(x), the lane's 16-term sum and the 6-step butterfly, 1 / sum and
    e * inv; pad lanes (-3e38 for the maximum, 0 for the sum) from cols = 1 to the full 64 x 16.  The bound (`softmax_ref64`) is relative to each
    probability.  Negative scale: the maximum is that of the scaled row.  rows = 4097: the last workgroup holds one row.  Logits of amplitude
    4, 30 and 300 (the last meant for the scale 0.125, run at every scale)"""
    from computervision_codes_amd import ops
    for rows, amps, scales in ((1, (4.0, 30.0, 300.0), SOFTMAX_SCALES), (5, (4.0, 30.0, 300.0), SOFTMAX_SCALES), (4097, (30.0,), (12 ** -0.5, -0.3))):
        for amp in amps:
            for scale in scales:
                s = softmax_inputs(rows, cols, amp, 7 * cols + rows)
                p64, extra = softmax_ref64(s, scale)
                got = ops.softmax_rows_(s.to(cuda), scale).cpu()
                assert torch.isfinite(got).all()
                check_f32(got, p64, extra=extra, what=f"softmax_rows rows={rows} cols={cols} amp={amp} scale={scale:.4f}")


@gpu
def test_softmax_refusals(cuda):
    """cols = 1025 (more than 64 lanes x 16) and empty shapes are refused before a launch, forward and backward; the buffers stay as they were"""
    from computervision_codes_amd import ops
    s0 = _u((4, 1025), 1)
    s, d = s0.to(cuda), s0.to(cuda)
    assert ops.lib.mt4_softmax_rows_f32(s.data_ptr(), 4, 1025, 1.0, None) == EUNSUPPORTED
    assert ops.lib.mt4_softmax_bwd_rows_f32(s.data_ptr(), d.data_ptr(), 4, 1025, 1.0, None) == EUNSUPPORTED
    assert ops.lib.mt4_softmax_rows_f32(s.data_ptr(), 0, 64, 1.0, None) == EINVAL and ops.lib.mt4_softmax_rows_f32(s.data_ptr(), 4, 0, 1.0, None) == EINVAL
    assert ops.lib.mt4_softmax_rows_f32(None, 4, 64, 1.0, None) == EINVAL
    assert ops.lib.mt4_softmax_bwd_rows_f32(s.data_ptr(), None, 4, 64, 1.0, None) == EINVAL
    assert ops.lib.mt4_softmax_bwd_rows_f32(s.data_ptr(), d.data_ptr(), 0, 64, 1.0, None) == EINVAL
    torch.cuda.synchronize()
    check_exact(s.cpu(), s0, what="softmax refusals: S")
    check_exact(d.cpu(), s0, what="softmax refusals: dP")


def softmax_bwd_inputs(rows, cols, amp, scale, seed):
    """P: an fp32 softmax made on the CPU (of `softmax_inputs`); dP with a power-of-two scale per row (rows are not reduced)"""
    p = torch.softmax(_f32(scale) * softmax_inputs(rows, cols, amp, seed), -1)
    dp = _u((rows, cols), seed + 1) * pow2_ramp(rows)[:, None]
    return p, dp


@gpu
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_bwd_rows_per_element(cuda, cols):
    """`softmax_bwd_rows_kernel`: dS = scale P (dP - dot) over dP, dot = sum P dP (16 FMAs per lane, the butterfly); then the difference and two
    products.  Bound: `softmax_bwd_ref64`.  In place: the result is dP's buffer; P is bit-identical afterwards"""
    from computervision_codes_amd import ops
    for rows, amps, scales in ((1, (4.0, 30.0), SOFTMAX_SCALES), (5, (4.0, 30.0), SOFTMAX_SCALES), (4097, (4.0,), (12 ** -0.5, -0.3))):
        for amp in amps:
            for scale in scales:
                p, dp = softmax_bwd_inputs(rows, cols, amp, scale, 11 * cols + rows)
                ref, extra = softmax_bwd_ref64(p, dp, scale)
                pd, dpd = p.to(cuda), dp.to(cuda)
                out = ops.softmax_bwd_rows_(pd, dpd, scale)
                assert out.data_ptr() == dpd.data_ptr()
                what = f"softmax_bwd_rows rows={rows} cols={cols} amp={amp} scale={scale:.4f}"
                check_f32(dpd.cpu(), ref, extra=extra, what=what)
                check_exact(pd.cpu(), p, what=what + " P untouched")


# ------------------------------------------------------------------------------------------------ LayerNorm backward
LN_EPS = 1e-5
LN_C = [7, 32, 96, 864, 1024, 1025, 1536, 2048, 2049, 3072]
LN_CASES = [(m, c) for c in LN_C for m in (1, 5, 77)] + [(4097, 96), (4097, 1025), (4097, 2049), (33000, 96)]


def ln_grid(m):
    """(workgroups, waves) `mt4_layernorm_bwd_f32` launches for M rows"""
    blocks = max(1, min(1024, (m + 31) // 32))
    return blocks, blocks * 4


def layernorm_inputs(m, c, mean_over_std, scale_axis, seed):
    """x with row means of `mean_over_std` standard deviations (0.577 for uniform [-1, 1]) that vary by a quarter from row to row; from five rows
    on, row 1 is constant (variance 0: rstd = eps^-1/2); gamma in [0.5, 2.5]; dy scaled by powers of two per row (scale_axis 0: for the dx check,
    whose reductions run over the channels) or per channel (scale_axis 1: for dgamma / dbeta, which reduce over the rows)"""
    x = _u((m, c), seed) + mean_over_std * 0.577 * (1.0 + 0.25 * _u((m, 1), seed + 1))
    if m >= 5:
        x[1] = 3.0
    gamma = _u((c,), seed + 2) + 1.5
    dy = _u((m, c), seed + 3) * (pow2_ramp(m)[:, None] if scale_axis == 0 else pow2_ramp(c)[None, :])
    return x, gamma, dy


@gpu
@pytest.mark.parametrize("mean_over_std", [1.0, 100.0])
@pytest.mark.parametrize("m,c", LN_CASES, ids=lambda v: str(v))
def test_layernorm_bwd_per_element(cuda, m, c, mean_over_std):
    """`layernorm_bwd_kernel<16 / 32 / 48>` (C <= 1024 / 2048 / 3072), one wave per row, rows grid-strided over at most 1024 workgroups (M = 33000
    reaches the cap).  Rounds: the row mean (C additions, x 1/C), the two-pass variance, rsqrtf, xhat, the two row means of g and g xhat, the final
    expression; dgamma / dbeta: a wave's rows in registers, then one float atomic per wave and channel.  Bounds: `layernorm_bwd_ref64`.
    dx on row-scaled dy, also accumulated onto a base scaled like the result (v is rounded, then the sum: v's half ulp joins the allowance);
    dgamma / dbeta on channel-scaled dy, added to a non-zero base (the atomics round at |base| + the partial sum: sqrt(M + 1) 2^-24 |base|)"""
    from computervision_codes_amd import ops
    if m == 33000:
        assert ln_grid(m)[0] == 1024 and (m + 31) // 32 > 1024
    what = f"layernorm_bwd M={m} C={c} mean/std={mean_over_std}"
    x, gamma, dy = layernorm_inputs(m, c, mean_over_std, 0, 31)
    dx64, b_dx, _, _, _, _ = layernorm_bwd_ref64(dy, x, gamma, LN_EPS)
    xd, gd = x.to(cuda), gamma.to(cuda)
    dg, db = torch.zeros(c, device=cuda), torch.zeros(c, device=cuda)
    dx = ops.layernorm_bwd(dy.to(cuda), xd, gd, dg, db, eps=LN_EPS)
    check_f32(dx.cpu(), dx64, extra=b_dx, what=what + " dx")
    base = (_u((m, c), 35) * dx64.abs()).float()
    acc = ops.layernorm_bwd(dy.to(cuda), xd, gd, dg, db, dx=base.to(cuda), accumulate_dx=True, eps=LN_EPS)
    check_f32(acc.cpu(), base.double() + dx64, extra=b_dx + half_ulp_f32(dx64), what=what + " dx accumulate")
    x, gamma, dy = layernorm_inputs(m, c, mean_over_std, 1, 41)
    _, _, dg64, b_dg, db64, b_db = layernorm_bwd_ref64(dy, x, gamma, LN_EPS)
    dg0, db0 = (_u((c,), 45) * dg64.abs()).float(), (_u((c,), 46) * db64.abs()).float()
    dg, db = dg0.to(cuda), db0.to(cuda)
    ops.layernorm_bwd(dy.to(cuda), x.to(cuda), gamma.to(cuda), dg, db, eps=LN_EPS)
    check_f32(dg.cpu(), dg0.double() + dg64, acc64=dg0.double().abs(), k=m + 1, extra=b_dg, what=what + " dgamma")
    check_f32(db.cpu(), db0.double() + db64, acc64=db0.double().abs(), k=m + 1, extra=b_db, what=what + " dbeta")


@gpu
def test_layernorm_bwd_refusals(cuda):
    """C = 3073 (more than 64 lanes x 48) and empty shapes are refused before a launch; dx, dgamma and dbeta stay as they were"""
    from computervision_codes_amd import ops
    c = 3073
    x, o0 = _u((2, c), 1).to(cuda), torch.full((2, c), 7.0)
    g, dx, dg, db = torch.ones(c, device=cuda), o0.to(cuda), o0[0].to(cuda), o0[1].to(cuda)
    f = ops.lib.mt4_layernorm_bwd_f32
    assert f(x.data_ptr(), x.data_ptr(), g.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 2, c, LN_EPS, 0, None) == EUNSUPPORTED
    assert f(x.data_ptr(), x.data_ptr(), g.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, 96, LN_EPS, 0, None) == EINVAL
    assert f(x.data_ptr(), x.data_ptr(), g.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 2, 0, LN_EPS, 0, None) == EINVAL
    assert f(x.data_ptr(), x.data_ptr(), None, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 2, 96, LN_EPS, 0, None) == EINVAL
    torch.cuda.synchronize()
    check_exact(torch.cat([dx.reshape(-1), dg, db]).cpu(), torch.full((4 * c,), 7.0), what="layernorm_bwd refusals")


# ------------------------------------------------------------------------------------------------ GELU forward and backward
GELU_N = [4, 8, 1020, 1024, 1028, 2 ** 20 + 4]
GELU_SPECIAL = [0.0, -0.0, 1e-8, -1e-8, 40.0, -40.0, 1e20, -1e20]


def gelu_inputs(n, seed):
    """x over [-12, 12] with the special values at the front (as many as fit), dy with a power-of-two scale per element"""
    x = _u((n,), seed) * 12.0
    k = min(n, len(GELU_SPECIAL))
    x[:k] = torch.tensor(GELU_SPECIAL[:k])
    return x, _u((n,), seed + 1) * pow2_ramp(n)


def gelu_bwd_ref64(dy, x):
    """float64 dy (Phi(x) + x phi(x))"""
    x64 = x.double()
    return dy.double() * (0.5 * torch.erfc(-x64 / math.sqrt(2.0)) + x64 * torch.exp(-0.5 * x64 * x64) / math.sqrt(2.0 * math.pi))


@gpu
@pytest.mark.parametrize("n", GELU_N)
def test_gelu_and_gelu_bwd_per_element(cuda, n):
    """`gelu_bwd_kernel` (Abramowitz-Stegun erf sharing its __expf with phi; float4 per thread): |err| <= GELU_BWD_ERR |dy| + half an ulp, out of
    place and in place over dy (as both trainers call it); `gelu_fwd_kernel` (gelu_erf): GELU_APPROX_ERR.  Saturated and tiny arguments, +-0,
    n around the 1024-element workgroup and 2^20 + 4"""
    from computervision_codes_amd import ops
    x, dy = gelu_inputs(n, 51)
    ref = gelu_bwd_ref64(dy, x)
    xd, dyd = x.to(cuda), dy.to(cuda)
    got = ops.gelu_bwd(dyd, xd).cpu()
    assert torch.isfinite(got).all()
    check_f32(got, ref, extra=GELU_BWD_ERR * dy.double().abs(), what=f"gelu_bwd n={n}")
    check_exact(dyd.cpu(), dy, what=f"gelu_bwd n={n}: dy untouched out of place")
    out = ops.gelu_bwd(dyd, xd, out=dyd)
    assert out.data_ptr() == dyd.data_ptr()
    check_exact(dyd.cpu(), got, what=f"gelu_bwd n={n}: in place equals out of place")
    check_exact(xd.cpu(), x, what=f"gelu_bwd n={n}: x untouched")
    x64 = x.double()
    y = ops.gelu(xd).cpu()
    assert torch.isfinite(y).all()
    check_f32(y, x64 * 0.5 * torch.erfc(-x64 / math.sqrt(2.0)), extra=GELU_APPROX_ERR, what=f"gelu n={n}")


@gpu
def test_gelu_refusals(cuda):
    """n % 4 != 0 (the kernels move float4) and pointers off a 16-byte boundary are refused before a launch"""
    from computervision_codes_amd import ops
    b0 = torch.full((16,), 7.0)
    x, dy, dx = torch.zeros(16, device=cuda), torch.zeros(16, device=cuda), b0.to(cuda)
    fb, ff = ops.lib.mt4_gelu_bwd_f32, ops.lib.mt4_gelu_f32
    for n in (1, 2, 3, 5, 6, 7, 0, -4):
        assert fb(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), n, None) == EINVAL and ff(x.data_ptr(), dx.data_ptr(), n, None) == EINVAL
    for off in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):
        assert fb(dy.data_ptr() + off[0], x.data_ptr() + off[1], dx.data_ptr() + off[2], 8, None) == EALIGN
    assert ff(x.data_ptr() + 4, dx.data_ptr(), 8, None) == EALIGN and ff(x.data_ptr(), dx.data_ptr() + 4, 8, None) == EALIGN
    assert fb(None, x.data_ptr(), dx.data_ptr(), 8, None) == EINVAL
    torch.cuda.synchronize()
    check_exact(dx.cpu(), b0, what="gelu refusals")


# ------------------------------------------------------------------------------------------------ depthwise Conv1d k = 3 backward
DW_SLAB = 32                                        # rows per workgroup of `mt4_dwconv1d_k3_bwd_f32`
DW_T = [1, 2, 31, 32, 33, 45, 64, 65, 256]
DW_C = [1, 3, 255, 256, 257, 864]


def dwconv_inputs(b, t, c, seed, boundary=True):
    """x, dy [B, T, C] and w [C, 3] with a power-of-two scale per channel (channels are not reduced); with `boundary` the first and the last
    row of every sequence are 2^8 larger, so that a row carried across a sequence boundary (or a boundary row missed at a slab edge) moves the
    result by far more than the bound"""
    x, dy = _u((b, t, c), seed) * pow2_ramp(c), _u((b, t, c), seed + 1) * pow2_ramp(c).flip(0)
    for v in (x, dy) if boundary else ():
        v[:, 0] *= 256.0
        if t > 1:
            v[:, -1] *= 256.0
    w = (_u((c, 3), seed + 2) + 1.5) * pow2_ramp(c)[:, None]
    return x, dy, w


def dwconv_bwd_ref64(x, dy, w):
    """float64 (dx, acc_dx, dw, acc_dw, db, acc_db) of y[t] = sum_k w[k] x[t + k - 1] with zero padding inside every sequence"""
    x64, d64, w64 = x.double(), dy.double(), w.double()
    z = torch.zeros_like(d64[:, :1])
    nxt = lambda v: torch.cat([v[:, 1:], z], 1)
    prv = lambda v: torch.cat([z, v[:, :-1]], 1)
    terms = (w64[:, 0] * nxt(d64), w64[:, 1] * d64, w64[:, 2] * prv(d64))
    dx, adx = sum(terms), sum(v.abs() for v in terms)
    prods = (d64 * prv(x64), d64 * x64, d64 * nxt(x64))
    dw = torch.stack([v.sum((0, 1)) for v in prods], 1)
    adw = torch.stack([v.abs().sum((0, 1)) for v in prods], 1)
    return dx, adx, dw, adw, d64.sum((0, 1)), d64.abs().sum((0, 1))


def dw_k(b, t):
    """k of the dw / db checks: B T products / addends and the base, n = B T + 1 additions; below 16 their roundings are counted (k = n^2)"""
    n = b * t + 1
    return n if n >= 16 else n * n


def _dwconv_run(cuda, b, t, c, boundary):
    from computervision_codes_amd import ops
    x, dy, w = dwconv_inputs(b, t, c, 61 + c, boundary)
    ref = dwconv_bwd_ref64(x, dy, w)
    dw0, db0 = (_u((c, 3), 64) * ref[2].abs()).float(), (_u((c,), 65) * ref[4].abs()).float()
    dw, db = dw0.to(cuda), db0.to(cuda)
    dx = ops.dwconv1d_k3_bwd(dy.to(cuda), x.to(cuda), w.to(cuda), dw, db)
    return ref, dw0, db0, dx.cpu(), dw.cpu(), db.cpu()


@gpu
@pytest.mark.parametrize("t", DW_T)
@pytest.mark.parametrize("b", [1, 3])
def test_dwconv1d_k3_bwd_dx_per_element(cuda, b, t):
    """`dwconv1d_k3_bwd_kernel`: one thread per channel over a slab of 32 rows of one sequence, on operands whose sequence-boundary rows are 2^8
    larger.  dx = w0 dy[t+1] + w1 dy[t] + w2 dy[t-1]: two intermediate roundings of up to 2^-24 acc64 each (k = 4: sqrt(3) is below that worst
    case, 2 is not).  T around the slab (31 .. 33, 64, 65), C around the 256-thread workgroup"""
    for c in DW_C:
        (dx64, adx, _, _, _, _), _, _, dx, _, _ = _dwconv_run(cuda, b, t, c, True)
        check_f32(dx, dx64, acc64=adx, k=4, what=f"dwconv1d_k3_bwd B={b} T={t} C={c} boundary rows x 2^8: dx")


def _dwconv_dw_db_checks(cuda, b, t, boundary):
    for c in DW_C:
        (dx64, adx, dw64, adw, db64, adb), dw0, db0, dx, dw, db = _dwconv_run(cuda, b, t, c, boundary)
        what = f"dwconv1d_k3_bwd B={b} T={t} C={c}" + (" boundary rows x 2^8:" if boundary else "")
        if not boundary:
            check_f32(dx, dx64, acc64=adx, k=4, what=what + " dx")
        check_f32(dw, dw0.double() + dw64, acc64=dw0.double().abs() + adw, k=dw_k(b, t), what=what + " dw")
        check_f32(db, db0.double() + db64, acc64=db0.double().abs() + adb, k=dw_k(b, t), what=what + " db")


@gpu
@pytest.mark.parametrize("t", DW_T)
@pytest.mark.parametrize("b", [1, 3])
def test_dwconv1d_k3_bwd_dw_db_on_boundary_scaled_rows(cuda, b, t):
    """dw / db: a slab's sum in float64 registers, rounded once, then one float atomic per slab onto a non-zero base: k = B T + 1 (counted
    below 16: `dw_k`), on the operands whose sequence-boundary rows are 2^8 larger -- a row carried across a sequence or slab boundary moves
    the result by far more than the bound.  With fp32 slab sums dw[14][0] of B = 1, C = 257 was at 1.66, 1.28 and 1.37 of this bound for T = 31,
    32, 33 (the product 2^8 larger at the head of the slab makes the 29 later additions round at its size; test_seq_bounds_cpu.py reproduces
    those bits): that is why the kernel sums in float64"""
    _dwconv_dw_db_checks(cuda, b, t, True)


@gpu
@pytest.mark.parametrize("t", DW_T)
@pytest.mark.parametrize("b", [1, 3])
def test_dwconv1d_k3_bwd_dw_db_per_element(cuda, b, t):
    """the same bounds (and dx) on operands that carry the per-channel scales only: no term dominates the reduced axis"""
    _dwconv_dw_db_checks(cuda, b, t, False)


@gpu
def test_dwconv1d_k3_bwd_refusals(cuda):
    """empty shapes and more sequences than the grid's z limit are refused before a launch"""
    from computervision_codes_amd import ops
    o0 = torch.full((64,), 7.0)
    x, o = torch.zeros(64, device=cuda), o0.to(cuda)
    f = lambda bb, tt, cc: ops.lib.mt4_dwconv1d_k3_bwd_f32(x.data_ptr(), x.data_ptr(), x.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), bb, tt, cc, None)
    assert f(0, 4, 4) == EINVAL and f(1, 0, 4) == EINVAL and f(1, 4, 0) == EINVAL and f(65536, 1, 1) == EUNSUPPORTED
    assert ops.lib.mt4_dwconv1d_k3_bwd_f32(x.data_ptr(), x.data_ptr(), None, o.data_ptr(), o.data_ptr(), o.data_ptr(), 1, 4, 4, None) == EINVAL
    torch.cuda.synchronize()
    check_exact(o.cpu(), o0, what="dwconv1d_k3_bwd refusals")


# ------------------------------------------------------------------------------------------------ GroupWiseLinear backward
@gpu
@pytest.mark.parametrize("b,k,d", [(1, 6, 768), (3, 15, 768), (64, 10, 1536), (5, 100, 100), (2, 1, 1)])
def test_groupwise_linear_bwd_per_element(cuda, b, k, d):
    """`groupwise_linear_bwd_kernel`: dhs = dy W is ONE product (RNE agreement required).  dW: a sequential FMA chain over the batch, then the
    sum with the non-zero base: B roundings before the store's own, each of up to 2^-24 acc64 -- k = B^2 below 16 terms, B + 1 from there on;
    db likewise.  hs and W scaled per d, dy per k (the batch is the reduced axis)"""
    from computervision_codes_amd import ops
    dy = _u((b, k), 71) * pow2_ramp(k)
    hs = _u((b * k, d), 72) * pow2_ramp(d)
    w = _u((k, d), 73) * pow2_ramp(d).flip(0)
    dy64, hs64 = dy.double(), hs.double().view(b, k, d)
    dw64, adw = (dy64[:, :, None] * hs64).sum(0), (dy64[:, :, None] * hs64).abs().sum(0)
    db64, adb = dy64.sum(0), dy64.abs().sum(0)
    dw0, db0 = (_u((k, d), 74) * dw64.abs()).float(), (_u((k,), 75) * db64.abs()).float()
    dyd, hsd, wd, dw, db = dy.to(cuda), hs.to(cuda), w.to(cuda), dw0.to(cuda), db0.to(cuda)
    dhs = ops.groupwise_linear_bwd(dyd, hsd, wd, dw, db)
    what = f"groupwise_linear_bwd {(b, k, d)}"
    check_f32(dhs.cpu().view(b, k, d), dy64[:, :, None] * w.double()[None], single_rounding=True, what=what + " dhs")
    kk = b * b if b < 16 else b + 1
    got_dw, got_db = dw.cpu(), db.cpu()
    check_f32(got_dw, dw0.double() + dw64, acc64=dw0.double().abs() + adw, k=kk, what=what + " dW")
    check_f32(got_db, db0.double() + db64, acc64=db0.double().abs() + adb, k=kk, what=what + " db")
    f = lambda bb, kk_, dd: ops.lib.mt4_groupwise_linear_bwd_f32(dyd.data_ptr(), hsd.data_ptr(), wd.data_ptr(), dhs.data_ptr(), dw.data_ptr(),
                                                                 db.data_ptr(), bb, kk_,
                                                                  dd, None)
    assert f(0, k, d) == EINVAL and f(b, 0, d) == EINVAL and f(b, k, 0) == EINVAL
    torch.cuda.synchronize()
    check_exact(dw.cpu(), got_dw, what=what + " refusals leave dW")


# ------------------------------------------------------------------------------------------------ relative-position table gradient
RELPOS_CASES = [(7, 3, 8), (12, 4, 1), (12, 4, 3), (7, 1, 5), (4, 2, 64), (7, 3, 1000), (12, 4, 1024), (7, 48, 16), (1, 2, 3)]


def relpos_per(n_windows, heads):
    """the run of windows one workgroup of `mt4_relpos_table_grad_f32` sums (the wrapper's rule)"""
    per = max(4, (n_windows * heads + 511) // 512)
    return min(per, n_windows)


def relpos_index(ws):
    """Swin's relative_position_index for a ws x ws window, flattened [N * N]"""
    co = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0) + (ws - 1)
    return (rel[:, :, 0] * (2 * ws - 1) + rel[:, :, 1]).reshape(-1).to(torch.int32)


def relpos_inputs(ws, heads, n_windows, seed):
    """dS [n_windows, H, N, N] whose (i, j) entries carry the power-of-two scale of the table row they are added to (the windows are reduced)"""
    idx = relpos_index(ws)
    ts, n = (2 * ws - 1) ** 2, ws * ws
    ds = _u((n_windows, heads, n * n), seed) * pow2_ramp(ts)[idx.long()]
    return ds.view(n_windows, heads, n, n), idx, ts


def relpos_ref64(ds, idx, ts):
    """float64 (dtable, acc, terms): the index_add_ of the windows' sum, the same on |dS|, and the number of addends of every table row"""
    nw, h, n, _ = ds.shape
    d64 = ds.double().view(nw, h, n * n)
    ref = torch.zeros(ts, h, dtype=torch.float64).index_add_(0, idx.long(), d64.sum(0).t())
    acc = torch.zeros(ts, h, dtype=torch.float64).index_add_(0, idx.long(), d64.abs().sum(0).t())
    cnt = torch.bincount(idx.long(), minlength=ts).double()
    return ref, acc, (nw * cnt)[:, None].expand(ts, h)


def test_relpos_cases_reach_every_run_shape():
    """RELPOS_CASES make `per` equal to n_windows (one workgroup per head), 4 with a short last workgroup, 6 (the 4-unrolled loop + a tail of 2)
    and 8 (two unrolled rounds)"""
    per = {c: relpos_per(c[2], c[1]) for c in RELPOS_CASES}
    assert any(p == c[2] and p < 4 for c, p in per.items()), per
    assert any(p == 4 and c[2] > 4 and c[2] % 4 for c, p in per.items()), per
    assert per[(7, 3, 1000)] == 6 and per[(12, 4, 1024)] == 8, per


@gpu
@pytest.mark.parametrize("ws,heads,n_windows", RELPOS_CASES)
def test_relpos_table_grad_per_element(cuda, ws, heads, n_windows):
    """`relpos_table_grad_kernel`: per (i, j) four running sums over the workgroup's windows (+ a tail), folded into an LDS column by ds_add_f32,
    the column added to the non-zero table by float atomics.  Every table row sums n_windows x (entries of idx equal to it) addends and the
    base: sqrt of that count times 2^-24 acc64 from 16 addends on, the count itself below (every addition may round by 2^-24 acc64)"""
    from computervision_codes_amd import ops
    ds, idx, ts = relpos_inputs(ws, heads, n_windows, 81)
    ref, acc, terms = relpos_ref64(ds, idx, ts)
    t0 = (_u((ts, heads), 82) * ref.abs()).float()
    tab = t0.to(cuda)
    ops.relpos_table_grad(ds.to(cuda), idx.to(cuda), tab)
    check_f32(tab.cpu(), t0.double() + ref, acc64=(t0.double().abs() + acc) * _count_k(terms + 1), k=1,
              what=f"relpos_table_grad ws={ws} H={heads} windows={n_windows} per={relpos_per(n_windows, heads)}")


@gpu
def test_relpos_table_grad_refusals(cuda):
    """N = 50 is no square window; empty shapes; more heads than a grid dimension holds: refused before a launch, the table untouched"""
    from computervision_codes_amd import ops
    t0 = torch.full((169, 2), 7.0)
    ds, idx, tab = torch.zeros(2 * 2 * 50 * 50, device=cuda), torch.zeros(2500, dtype=torch.int32, device=cuda), t0.to(cuda)
    f = lambda nw, h, n: ops.lib.mt4_relpos_table_grad_f32(ds.data_ptr(), idx.data_ptr(), tab.data_ptr(), nw, h, n, None)
    assert f(2, 2, 50) == EINVAL and f(0, 2, 49) == EINVAL and f(2, 0, 49) == EINVAL and f(2, 2, 0) == EINVAL and f(2, 65536, 49) == EINVAL
    assert ops.lib.mt4_relpos_table_grad_f32(ds.data_ptr(), None, tab.data_ptr(), 2, 2, 49, None) == EINVAL
    torch.cuda.synchronize()
    check_exact(tab.cpu(), t0, what="relpos_table_grad refusals")


# ------------------------------------------------------------------------------------------------ AvgPool1d adjoint
@gpu
@pytest.mark.parametrize("t_in,k,stride", [(301, 7, 3), (99, 7, 3), (31, 7, 3), (10, 7, 3), (7, 7, 3), (2000, 7, 3), (20, 4, 4), (21, 2, 1)])
def test_avgpool1d_rows_bwd_per_element(cuda, t_in, k, stride):
    """`avgpool1d_rows_bwd_kernel`: dx[t] = (sum of dy[w] over the windows w that contain t) / k -- up to ceil(k / stride) terms and one
    division: k_check = kernel + 1.  dy scaled per channel.  Rows beyond the last window's reach are exactly zero"""
    from computervision_codes_amd import ops
    t_out = (t_in - k) // stride + 1
    for c in (4, 8, 64, 512):
        for b in (1, 3):
            dy = _u((b, t_out, c), 91) * pow2_ramp(c)
            ref, acc = torch.zeros(b, t_in, c, dtype=torch.float64), torch.zeros(b, t_in, c, dtype=torch.float64)
            for w in range(t_out):
                ref[:, w * stride:w * stride + k] += dy.double()[:, w:w + 1] / k
                acc[:, w * stride:w * stride + k] += dy.double().abs()[:, w:w + 1] / k
            dx = ops.avgpool1d_rows_bwd(dy.to(cuda), t_in, k, stride).cpu()
            what = f"avgpool1d_rows_bwd {(t_in, k, stride)} C={c} B={b}"
            check_f32(dx, ref, acc64=acc, k=k + 1, what=what)
            reach = (t_out - 1) * stride + k
            check_exact(dx[:, reach:], torch.zeros(b, t_in - reach, c), what=what + " rows no window reaches")
    dyd, o0 = torch.zeros(64, device=cuda), torch.full((64,), 7.0)
    o = o0.to(cuda)
    f = lambda bb, tt, cc, kk, ss, off=0: ops.lib.mt4_avgpool1d_rows_bwd_f32(dyd.data_ptr() + off, o.data_ptr(), bb, tt, cc, kk, ss, None)
    assert f(1, 6, 4, 7, 3) == EINVAL and f(0, 8, 4, 7, 3) == EINVAL and f(1, 8, 4, 0, 3) == EINVAL and f(1, 8, 4, 7, 0) == EINVAL
    assert f(1, 8, 6, 7, 3) == EALIGN and f(1, 8, 4, 7, 3, off=4) == EALIGN
    torch.cuda.synchronize()
    check_exact(o.cpu(), o0, what="avgpool1d_rows_bwd refusals")


# ------------------------------------------------------------------------------------------------ linear interpolation adjoint
INTERP_CASES = [(9, 31), (31, 99), (99, 301), (5, 5), (1, 4), (20, 7), (301, 99), (667, 2000), (2000, 667)]


def _r4(v):
    return (v + 3) // 4 * 4


@gpu
@pytest.mark.parametrize("t_in,t_out", INTERP_CASES)
def test_interp_linear_rows_bwd_is_the_forwards_transpose(cuda, t_in, t_out):
    """(i) the weight matrix of `interp_linear_rows` (the forward on an identity) and that of `interp_linear_rows_bwd` (the backward on an
    identity) are each other's transpose BIT FOR BIT: both kernels compute the source index by the same expression, and a product with 1 and
    sums with 0 are exact.  (ii) that matrix against float64 weights from the fp32 `scale`: every weight within two fp32 ulps of its source
    index (computed in fp32, up to 2000; taken at src + 0.5, the intermediate scale (w + 0.5)).  (iii) a general dy, scaled per channel: float64
    W^T dy with the device's own W; an input row sums (output rows touching it) FMAs: that count + 1 roundings below 16, sqrt from there on"""
    from computervision_codes_amd import ops
    ci, co = _r4(t_in), _r4(t_out)
    eye_in = torch.zeros(1, t_in, ci)
    eye_in[0, torch.arange(t_in), torch.arange(t_in)] = 1.0
    eye_out = torch.zeros(1, t_out, co)
    eye_out[0, torch.arange(t_out), torch.arange(t_out)] = 1.0
    wf = ops.interp_linear_rows(eye_in.to(cuda), t_out).cpu()[0]                     # [t_out, ci]: W[w][t]
    wb = ops.interp_linear_rows_bwd(eye_out.to(cuda), t_in).cpu()[0]                # [t_in, co]: W[w][t] at [t][w]
    what = f"interp_linear_rows {(t_in, t_out)}"
    check_exact(wb[:, :t_out], wf[:, :t_in].t(), what=what + " backward weights == forward weights transposed")
    check_exact(wf[:, t_in:], torch.zeros(t_out, ci - t_in), what=what + " forward padding")
    check_exact(wb[:, t_out:], torch.zeros(t_in, co - t_out), what=what + " backward padding")
    scale = float(torch.tensor(float(t_in), dtype=torch.float32) / torch.tensor(float(t_out), dtype=torch.float32))
    src = torch.clamp(scale * (torch.arange(t_out, dtype=torch.float64) + 0.5) - 0.5, min=0.0)
    i0 = torch.floor(src).long().clamp(max=t_in - 1)
    i1 = torch.where(i0 < t_in - 1, i0 + 1, i0)
    l1 = src - i0.double()
    w64 = torch.zeros(t_out, t_in, dtype=torch.float64)
    w64[torch.arange(t_out), i0] += 1.0 - l1
    w64[torch.arange(t_out), i1] += l1
    two_ulp = 4.0 * half_ulp_f32(src + 0.5)                                          # 2 ulps = 4 half-ulps
    check_f32(wf[:, :t_in], w64, extra=two_ulp[:, None].expand(t_out, t_in), what=what + " weights vs float64")
    wdev = wf[:, :t_in].double()
    nnz = (wdev != 0).sum(0).double()                                                # output rows touching every input row
    for c in (4, 64):
        for b in (1, 3):
            dy = _u((b, t_out, c), 95) * pow2_ramp(c)
            ref = torch.einsum("wt,bwc->btc", wdev, dy.double())
            acc = torch.einsum("wt,bwc->btc", wdev.abs(), dy.double().abs())
            dx = ops.interp_linear_rows_bwd(dy.to(cuda), t_in).cpu()
            check_f32(dx, ref, acc64=acc * _count_k(nnz + 1)[None, :, None], k=1, what=what + f" bwd C={c} B={b}")


@gpu
def test_interp_linear_rows_bwd_refusals(cuda):
    """empty shapes, C % 4 != 0 and a pointer off a 16-byte boundary are refused before a launch"""
    from computervision_codes_amd import ops
    dyd, o0 = torch.zeros(64, device=cuda), torch.full((64,), 7.0)
    o = o0.to(cuda)
    f = lambda bb, ti, to, cc, off=0: ops.lib.mt4_interp_linear_rows_bwd_f32(dyd.data_ptr() + off, o.data_ptr(), bb, ti, to, cc, None)
    assert f(0, 4, 4, 4) == EINVAL and f(1, 0, 4, 4) == EINVAL and f(1, 4, 0, 4) == EINVAL and f(1, 4, 4, 0) == EINVAL
    assert f(1, 4, 4, 6) == EALIGN and f(1, 4, 4, 4, off=4) == EALIGN
    torch.cuda.synchronize()
    check_exact(o.cpu(), o0, what="interp_linear_rows_bwd refusals")


# ------------------------------------------------------------------------------------------------ DistillKL
def distill_kl_ref64(ys, tp, temp, grad_scale):
    """float64 of `distill_kl_kernel` on fp32 logits ys [B, K], teacher logits tp [B, K] and the fp32 temp / grad_scale:
        p_t = softmax(sigmoid(tp) / T), log p_s = log_softmax(ys / T), row loss = sum_k p_t (log p_t - log p_s), g = grad_scale T / B (p_s - p_t)
    Returns (g, extra_g, acc_g, row_loss, extra_row, acc_row) per row, without the T^2 / B of the loss.  Bound, u = 2^-24, e = FN_EPS per expf /
    logf call; for either softmax with arguments a_k (absolute error da_k), m = max a, x = a - m, z = sum exp(x), lp = x - log z:
        student a = ys / T: da = u |a| (the division);  teacher a = sigmoid(tp) / T: da = (e + 3 u) |a| (expf, 1 + ., 1 / ., / T)
        rho_k  = da_k + da_max + u |x_k| + e                      relative error of exp(x_k)
        dlz    = sum_k p_k rho_k + (sqrt(K) + 1) u + e |log z|    absolute error of log z: the sum's terms, its additions, logf
        dlp_k  = da_k + da_max + u |x_k| + u |lp_k| + dlz         absolute error of lp_k (two subtractions)
        p_k    = expf(lp_k): relative error dlp_k + e
        g:   |c| (p_s (dlp_s + e) + p_t (dlp_t + e)) + the roundings of c = grad_scale T / B (two), of the difference and of the product:
             acc_g = |c| (p_s + p_t), k = 16 (four roundings of up to u acc_g each); + |c| 2^-126 (an expf result below the smallest normal)
        row: sum_k [ p_t (dlp_t + e) |lp_t - lp_s| + p_t (dlp_t + dlp_s) ] + 2 u acc_row, acc_row = sum_k p_t |lp_t - lp_s| (the difference and
             the product round; the K additions are counted by the caller with sqrt(K) u acc_row)"""
    u, e = EPS, FN_EPS
    temp, grad_scale = _f32(temp), _f32(grad_scale)
    b, k = ys.shape

    def lsm(a, da):
        m = a.max(-1, keepdim=True)
        x = a - m.values
        da_max = torch.gather(da, -1, m.indices)
        z = torch.exp(x).sum(-1, keepdim=True)
        lp = x - torch.log(z)
        p = torch.exp(lp)
        rho = da + da_max + u * x.abs() + e
        dlz = (p * rho).sum(-1, keepdim=True) + (math.sqrt(k) + 1.0) * u + e * torch.log(z).abs()
        return lp, p, da + da_max + u * x.abs() + u * lp.abs() + dlz

    a_s = ys.double() / temp
    a_t = torch.sigmoid(tp.double()) / temp
    lps, ps, dlps = lsm(a_s, u * a_s.abs())
    lpt, pt, dlpt = lsm(a_t, (e + 3.0 * u) * a_t.abs())
    c = grad_scale * temp / b
    g = c * (ps - pt)
    extra_g = abs(c) * (ps * (dlps + e) + pt * (dlpt + e) + F32_MIN_NORMAL)
    acc_g = abs(c) * (ps + pt)
    diff = lpt - lps
    acc_row = (pt * diff.abs()).sum(-1)
    extra_row = (pt * (dlpt + e) * diff.abs() + pt * (dlpt + dlps)).sum(-1) + 2.0 * u * acc_row
    return g, extra_g, acc_g, (pt * diff).sum(-1), extra_row, acc_row


@gpu
@pytest.mark.parametrize("k", [1, 6, 10, 15, 64, 65, 100, 128])
def test_distill_kl_per_element(cuda, k):
    """`distill_kl_kernel` (one wave per row, two columns per lane; accurate expf / logf): gradient and loss against `distill_kl_ref64`, y and dy
    as column slices of wider buffers (ld_y, ld_dy > K; the neighbouring columns untouched bit for bit), accumulate on and off, temperatures 1
    and 4, student logits of amplitude 3 and 50, teacher logits of amplitude 2 and 30.  The loss is B float atomics of row losses onto a
    non-zero value: k = B + 1 on acc = |loss0| + T^2 / B sum_b acc_row, plus the rows' own bounds and sqrt(K) 2^-24 acc_row for their sums"""
    from computervision_codes_amd import ops
    for b in (1, 64, 1000):
        for temp, amp_s, amp_t, accumulate in ((1.0, 3.0, 2.0, True), (4.0, 50.0, 30.0, False), (4.0, 3.0, 30.0, True), (1.0, 50.0, 2.0, False)):
            ld_y, ld_dy, o_y, o_dy = k + 9, k + 6, 4, 3
            ybuf = _u((b, ld_y), 101) * amp_s
            tp = _u((b, k), 102) * amp_t
            gs = 0.7 / 3.0
            g64, ex_g, acc_g, row64, ex_row, acc_row = distill_kl_ref64(ybuf[:, o_y:o_y + k], tp, temp, gs)
            dy0 = _u((b, ld_dy), 103)
            dy0[:, o_dy:o_dy + k] *= g64.abs().float()
            loss0 = torch.tensor([0.37])
            yd, dyd, ls = ybuf.to(cuda), dy0.to(cuda), loss0.to(cuda)
            ops.distill_kl(yd[:, o_y:o_y + k], tp.to(cuda), dyd[:, o_dy:o_dy + k], ls, temp, gs, accumulate=accumulate)
            got = dyd.cpu()
            what = f"distill_kl K={k} B={b} T={temp} amp={amp_s}/{amp_t} acc={accumulate}"
            assert torch.isfinite(got).all()
            base = dy0[:, o_dy:o_dy + k].double() if accumulate else torch.zeros_like(g64)
            check_f32(got[:, o_dy:o_dy + k], base + g64, acc64=acc_g + base.abs(), k=16, extra=ex_g + half_ulp_f32(g64), what=what + " dy")
            check_exact(torch.cat([got[:, :o_dy], got[:, o_dy + k:]], 1), torch.cat([dy0[:, :o_dy], dy0[:, o_dy + k:]], 1), what=what + " dy neighbours")
            check_exact(yd.cpu(), ybuf, what=what + " y untouched")
            t2b = _f32(temp) ** 2 / b
            extra_l = t2b * (ex_row + (math.sqrt(k) + 2.0) * EPS * acc_row).sum().reshape(1)      # + 2: l T T / B rounds twice
            check_f32(ls.cpu(), loss0.double() + t2b * row64.sum().reshape(1), acc64=loss0.double().abs() + t2b * acc_row.sum().reshape(1), k=b + 1,
                      extra=extra_l, what=what + " loss")
    y, o0 = torch.zeros(4 * 140, device=cuda), torch.full((4 * 140,), 7.0)
    o = o0.to(cuda)
    f = lambda bb, kk, ly, ld: ops.lib.mt4_distill_kl_f32(y.data_ptr(), y.data_ptr(), o.data_ptr(), o.data_ptr(), bb, kk, ly, ld, 4.0, 1.0, 1, None)
    assert f(4, 129, 140, 140) == EINVAL and f(0, 8, 8, 8) == EINVAL and f(4, 0, 8, 8) == EINVAL and f(4, 8, 7, 8) == EINVAL and f(4, 8, 8, 7) == EINVAL
    torch.cuda.synchronize()
    check_exact(o.cpu(), o0, what="distill_kl refusals")
    with pytest.raises(AssertionError):
        ops.distill_kl(y.view(4, 140)[:, :8], y.view(4, 140)[:, :8], o.view(4, 140)[:, :8], o[:1], 4.0, 1.0)      # t_pred must be dense [B, K]


# ------------------------------------------------------------------------------------------------ KD mixing, forward and backward
def kd_mix_ref64(s, teas, gs=None, tau_f32_sum=False):
    """float64 of `kd_mix_kernel` / `kd_mix_bwd_kernel` on fp32 s [B, C], three teacher features [B, C] and (backward) three gradients [B, C]:
        tau_n = sum_d tea_n[b][d];  l_n = s tau_n / sqrt(C);  a = softmax_n(l);  out_n = s a_n
        q_n = g_n s;  dot = sum_n a_n q_n;  dl_n = a_n (q_n - dot);  ds = sum_n g_n a_n + sum_n dl_n tau_n / sqrt(C);  dtau_n = sum_c dl_n s / sqrt(C)
    Bounds, u = 2^-24, e = FN_EPS (accurate expf), all first order:
        dl_n   = 5 u |l_n| (+ |z| sqrt(C) u sum|tea_n| in the forward, whose tau is an fp32 sum; the backward's is a float64 sum rounded once):
                 rsqrtf(C) (2 u), z = s inv, z tau, tau's own rounding -- l reaches hundreds at C = 2048, so this is what every a_n feels
        rho_n  = dl_n + dl_max + u |l_n - max| + e                       relative error of exp(l_n - max)
        ra_n   = rho_n + sum_m a_m rho_m + 4 u                           relative error of a_n (two additions, 1 / ., the product)
        out_n: |s| a_n (ra_n + 2 u)
        ddot   = sum_n |a_n q_n| (ra_n + 4 u)                            absolute: dot is a difference-free sum, but dl_n is not --
        ddl_n  = a_n (u |q_n| + ddot + u |q_n - dot|) + |dl_n| (ra_n + u)    -- absolute in a_n (|q_n| + |dot|), as the terms nearly cancel
        ds:    sum_n |g_n a_n| ra_n + inv sum_n ddl_n |tau_n| + 8 u acc_ds,  acc_ds = sum_n |g_n a_n| + inv sum_n |dl_n tau_n|   (k = 64)
        dtau_n (accumulated in float64, stored once): sum_c ddl_n |z| + 3 u sum_c |dl_n z|
    Returns a dict of float64 tensors"""
    u, e = EPS, FN_EPS
    b, c = s.shape
    s64 = s.double()
    t64 = [t.double() for t in teas]
    tau = torch.stack([t.sum(-1) for t in t64], -1)[:, None, :]                      # [B, 1, 3]
    inv = 1.0 / math.sqrt(c)
    z = (s64 * inv)[:, :, None]                                                       # [B, C, 1]
    l = z * tau                                                                       # [B, C, 3]
    dl_err = 5.0 * u * l.abs()
    if tau_f32_sum:
        dl_err = dl_err + z.abs() * math.sqrt(c) * u * torch.stack([t.abs().sum(-1) for t in t64], -1)[:, None, :]
    mx = l.max(-1, keepdim=True)
    x = l - mx.values
    a = torch.softmax(l, -1)
    rho = dl_err + torch.gather(dl_err, -1, mx.indices) + u * x.abs() + e
    ra = rho + (a * rho).sum(-1, keepdim=True) + 4.0 * u
    out = dict(out=s64[:, :, None] * a, out_extra=(s64[:, :, None] * a).abs() * (ra + 2.0 * u) + F32_MIN_NORMAL * s64[:, :, None].abs())
    if gs is None:
        return out
    g = torch.stack([v.double() for v in gs], -1)
    q = g * s64[:, :, None]
    dot = (a * q).sum(-1, keepdim=True)
    dl = a * (q - dot)
    ddot = ((a * q).abs() * (ra + 4.0 * u)).sum(-1, keepdim=True)
    ddl = a * (u * q.abs() + ddot + u * (q - dot).abs()) + dl.abs() * (ra + u)
    out["ds"] = (g * a).sum(-1) + (dl * tau).sum(-1) * inv
    out["ds_acc"] = (g * a).abs().sum(-1) + (dl * tau).abs().sum(-1) * inv
    out["ds_extra"] = ((g * a).abs() * ra).sum(-1) + inv * (ddl * tau.abs()).sum(-1)
    out["dtau"] = (dl * z).sum(1)
    out["dtau_extra"] = (ddl * z.abs()).sum(1) + 3.0 * u * (dl * z).abs().sum(1)
    return out


@gpu
@pytest.mark.parametrize("b,c", [(1, 64), (3, 100), (64, 512), (8, 2048), (5, 1000)])
def test_kd_mix_and_kd_mix_bwd_per_element(cuda, b, c):
    """`kd_mix_kernel` and `kd_mix_bwd_kernel` (one workgroup per batch row) against `kd_mix_ref64`: teacher features of amplitude 0.2 (mixing
    logits of order 1) and 2 (hundreds at C = 2048: saturated mixing).  ds on gradients scaled per channel; dtau, which sums over the
    channels, on gradients scaled per batch row"""
    from computervision_codes_amd import ops
    for amp in (0.2, 2.0):
        s = _u((b, c), 111)
        teas = [_u((b, c), 112 + n) * amp + amp * 0.25 * (n - 1) for n in range(3)]
        what = f"kd_mix B={b} C={c} teacher amplitude {amp}"
        r = kd_mix_ref64(s, teas, tau_f32_sum=True)
        sd, td = s.to(cuda), [t.to(cuda) for t in teas]
        outs = torch.stack([o.cpu() for o in ops.kd_mix(sd, *td)], -1)
        assert torch.isfinite(outs).all()
        check_f32(outs, r["out"], extra=r["out_extra"], what=what + " forward")
        for axis in (1, 0):
            ramp = pow2_ramp(c)[None, :] if axis == 1 else pow2_ramp(b)[:, None]
            gs = [_u((b, c), 121 + n) * ramp for n in range(3)]
            r = kd_mix_ref64(s, teas, gs)
            ds, dtau = ops.kd_mix_bwd(sd, td, [g.to(cuda) for g in gs])
            assert torch.isfinite(ds).all() and torch.isfinite(dtau).all()
            if axis == 1:
                check_f32(ds.cpu(), r["ds"], acc64=r["ds_acc"], k=64, extra=r["ds_extra"], what=what + " ds")
            else:
                check_f32(dtau.cpu(), r["dtau"], extra=r["dtau_extra"], what=what + " dtau")
    o0 = torch.full((b, c), 7.0)
    o = o0.to(cuda)
    p = sd.data_ptr()
    assert ops.lib.mt4_kd_mix_bwd_f32(p, p, p, p, p, p, p, o.data_ptr(), o.data_ptr(), 0, c, None) == EINVAL
    assert ops.lib.mt4_kd_mix_bwd_f32(p, p, p, p, p, p, p, o.data_ptr(), o.data_ptr(), b, 0, None) == EINVAL
    assert ops.lib.mt4_kd_mix_bwd_f32(p, p, p, None, p, p, p, o.data_ptr(), o.data_ptr(), b, c, None) == EINVAL
    assert ops.lib.mt4_kd_mix(p, p, p, p, o.data_ptr(), o.data_ptr(), o.data_ptr(), 0, c, None) == EINVAL
    torch.cuda.synchronize()
    check_exact(o.cpu(), o0, what="kd_mix refusals")


# ------------------------------------------------------------------------------------------------ derived-weight refresh
REFRESH_TILES_PER_BLOCK = 4
REFRESH_SHAPES = [(64, 64), (72, 36), (100, 20), (4, 4), (200, 136), (33, 65)]
_PHASE_SEL = {0: [1], 1: [2, 0]}                    # stride-2 3x3, pad 1: phase parity -> original taps (SpatialCnnTrainer._refresh_transposed)
PHASE_MAPS = [([_PHASE_SEL[ph][a] * 3 + _PHASE_SEL[pw][b] for a in range(len(_PHASE_SEL[ph])) for b in range(len(_PHASE_SEL[pw]))],
               (len(_PHASE_SEL[ph]), len(_PHASE_SEL[pw]))) for ph in (0, 1) for pw in (0, 1)]


def refresh_entries():
    """(cout, cin, src_taps, bf16, transposed, tap_map, (kh, kw)) of one table: fp32 and bf16, plain and transposed, identity maps of 1 and 9
    taps, the 180-degree flip, the four sub-pixel phase kernels (1, 2, 2 and 4 taps); the single-tile (4, 4) entries sit between large ones (the
    block search), and tile counts that are no multiple of REFRESH_TILES_PER_BLOCK give short last blocks"""
    out = []
    for i, (cout, cin) in enumerate(REFRESH_SHAPES):
        bf = bool(i % 2)
        out.append((cout, cin, 1, bf, False, [0], (1, 1)))
        out.append((cout, cin, 9, not bf, False, list(range(9)), (3, 3)))
        out.append((cout, cin, 1, not bf, True, [0], (1, 1)))
        out.append((cout, cin, 9, bf, True, [8 - t for t in range(9)], (3, 3)))
        for j, (tm, sh) in enumerate(PHASE_MAPS):
            out.append((cout, cin, 9, bool((i + j) % 2), True, tm, sh))
    return out


def refresh_tiles(cout, cin, ntaps):
    return ntaps * ((cout + 31) // 32) * ((cin + 31) // 32)


def refresh_master(cout, cin, taps, seed):
    """packed fp32 master [cout][taps x roundup(cin, 4), rounded up to 32 words]: random values; in every row, elements that are exact ties of
    the bf16 rounding (low half-word 0x8000) under an even and under an odd upper half-word, and their neighbours one fp32 ulp either side; the
    padding columns hold garbage (they must not be copied)"""
    tw = _r4(cin)
    kpad = (taps * tw + 31) // 32 * 32
    src = _u((cout, kpad), seed) * 100.0
    bits = src.view(torch.int32)
    pat = torch.tensor([0x8000, 0x18000, 0x7FFF, 0x8001, 0x17FFF, 0x18001], dtype=torch.int32)
    n = min(len(pat), cin)
    bits[:, :n] = (bits[:, :n] & ~0x1FFFF) | pat[:n]
    return src


def refresh_want(src, cout, cin, bf16, transposed, tap_map, kpad_dst):
    """host construction of one destination (float64 values exactly representable in the destination type): [cout][taps x cin] or, transposed,
    [cin][taps x cout], taps of roundup(cols, 4 fp32 / 8 bf16) elements, destination tap t = master tap tap_map[t], padding zero"""
    tw_s = _r4(cin)
    rows, cols = (cin, cout) if transposed else (cout, cin)
    tw_d = (cols + 7) // 8 * 8 if bf16 else _r4(cols)
    want = torch.zeros(rows, kpad_dst, dtype=torch.float64)
    for t, st in enumerate(tap_map):
        blk = src[:, st * tw_s:st * tw_s + cin].double()
        want[:, t * tw_d:t * tw_d + cols] = blk.t() if transposed else blk
    return rne_bf16(want) if bf16 else want


@gpu
def test_refresh_weights_exact(cuda):
    """`refresh_weights_kernel` only moves and rounds: every destination of one 48-entry table equals the host construction bit for bit (RNE to
    bf16, ties to even), padding columns stay zero, and a second run after the masters changed rewrites every valid element"""
    from computervision_codes_amd import ops
    ents = refresh_entries()
    tiles = [refresh_tiles(co, ci, len(tm)) for co, ci, _, _, _, tm, _ in ents]
    assert any(t == 1 for t in tiles[1:-1]) and any(t % REFRESH_TILES_PER_BLOCK for t in tiles if t > REFRESH_TILES_PER_BLOCK) and len(ents) >= 8
    assert ops.REFRESH_TILES_PER_BLOCK == REFRESH_TILES_PER_BLOCK
    tab = ops.RefreshTable(cuda)
    masters, dsts = [], []
    for i, (co, ci, taps, bf, tr, tm, sh) in enumerate(ents):
        src = refresh_master(co, ci, taps, 200 + i)
        sd = src.to(cuda)
        assert sd.shape[1] >= taps * _r4(ci)
        masters.append((src, sd))
        dsts.append(tab.add(sd, co, ci, torch.bfloat16 if bf else torch.float32, tr, tm, sh))
    for rnd in range(2):
        tab.run()
        for (co, ci, taps, bf, tr, tm, sh), (src, sd), dst in zip(ents, masters, dsts):
            want = refresh_want(src, co, ci, bf, tr, tm, dst.shape[1])
            check_exact(dst.cpu(), want, what=f"refresh_weights run {rnd} cout={co} cin={ci} bf16={bf} transposed={tr} taps={tm}")
        for i, (src, sd) in enumerate(masters):          # new masters for the second run: every valid element changes
            src.copy_(refresh_master(src.shape[0], ents[i][1], ents[i][2], 300 + i) * 1.5)
            sd.copy_(src)
    assert ops.lib.mt4_refresh_weights(None, 1, 1, None) == EINVAL and ops.lib.mt4_refresh_weights(tab._table.data_ptr(), 0, 1, None) == EINVAL
    assert ops.lib.mt4_refresh_weights(tab._table.data_ptr(), 1, 0, None) == EINVAL
