"""GPU: the fp32 training kernels (the parity path of all four trainers) element by element against float64.

Operands carry per-channel (or per-row) power-of-two scales from 2^8 down to 2^-8, descending with the index, so that the ragged tail tiles
hold the smallest values and a small-magnitude region has to be right on its own; the scales add no rounding.  References are float64 of the
same fp32 operands; `acc64` is the same operation on absolute values.  Each check is `bf16_bounds.check_f32` (fp32 half-ulp + sqrt(k) 2^-24
acc64 + a stated allowance) or `check_exact` for kernels that only move data.  `test_f32_bounds_cpu.py` shows on CPU emulations that these
checks see errors the max-scaled tolerances of the older tests accept.
"""
import pytest
import torch

from bf16_bounds import check_exact, check_f32, pow2_ramp, sgd_ref64

gpu = pytest.mark.gpu
EPS = 2.0 ** -24


def _u(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2 - 1


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ conv2d weight gradient (fp32)
def wgrad2d_variant(b, ho, wo, cout, cin, kh, kw):
    """the kernel `mt4_wgrad_conv2d_f32` launches, replicated from its dispatch (computervision_codes_amd/csrc/train2d_kernels.hip,
    `mt4_wgrad_conv2d_f32`: the `fills` lambda and the three `launch_wgrad32_wide` branches after it)"""
    kpad = _cdiv(kh * kw * _cdiv(cin * 4, 16), 8) * 8 * 4                # mt4_conv_packed_k(cin, kh, kw, MT4_F32)
    max_splits = _cdiv(b * ho * wo, 256)
    fills = lambda bm, bn: _cdiv(kpad, bn) * _cdiv(cout, bm) * max_splits >= 512
    if cout > 64 and kpad > 64 and fills(128, 128):
        return "128x128"
    if kpad >= 128 and fills(64, 128):
        return "64x128"
    if cout > 64 and fills(128, 64):
        return "128x64"
    return "64x64"


def _out_size(h, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1


# (b, h, w, cin, cout, k, stride, pad, dil): Cin 4 (the 7x7 stem, packed K 196 -> 224), 20 (180 -> 192) and 36 (324 -> 352: ends inside a 64- and a
# 128-column tile); ragged Cout 40, 72, 100, 200; pixel counts where the fill rule flips the kernel (its max_splits = ceil(pixels / 256) moves by
# one): 32512 = 127 x 256 and 32513 just above it, 65280 = 255 x 256 and 65536 = 256 x 256, and 65279 just below a multiple; one split (198 pixels)
# and hundreds; a dilated case on a wide kernel; unequal stride and padding per axis
WGRAD2D_CASES = [
    (2, 9, 11, 36, 72, 3, (1, 1), (1, 1), (1, 1)),
    (2, 38, 38, 4, 64, 7, (2, 2), (3, 3), (1, 1)),
    (4, 100, 80, 4, 132, 7, (2, 2), (3, 3), (1, 1)),
    (1, 127, 256, 20, 200, 3, (1, 1), (1, 1), (1, 1)),
    (1, 533, 61, 20, 200, 3, (1, 1), (1, 1), (1, 1)),
    (1, 537, 65, 20, 100, 3, (1, 1), (3, 3), (3, 3)),
    (1, 171, 256, 36, 40, 3, (1, 1), (1, 1), (1, 1)),
    (1, 255, 256, 36, 200, 1, (1, 1), (0, 0), (1, 1)),
    (1, 256, 256, 36, 200, 1, (1, 1), (0, 0), (1, 1)),
    (1, 2251, 29, 36, 200, 1, (1, 1), (0, 0), (1, 1)),
    (2, 61, 50, 20, 72, 3, (2, 1), (1, 0), (1, 1)),
    (2, 60, 64, 36, 100, 3, (1, 1), (2, 2), (2, 2)),
]


def _case_variant(c):
    b, h, w, cin, cout, k, s, p, d = c
    return wgrad2d_variant(b, _out_size(h, k, s[0], p[0], d[0]), _out_size(w, k, s[1], p[1], d[1]), cout, cin, k, k)


def test_wgrad2d_cases_reach_every_kernel():
    """the dispatch table of WGRAD2D_CASES: each of the four fp32 weight-gradient kernels is reached by at least one case"""
    table = {c: _case_variant(c) for c in WGRAD2D_CASES}
    assert set(table.values()) == {"64x64", "128x128", "64x128", "128x64"}, table
    # both sides of the multiples of 256 flip the kernel (max_splits changes by one)
    assert _case_variant(WGRAD2D_CASES[3]) == "64x128" and _case_variant(WGRAD2D_CASES[4]) == "128x128"
    assert _case_variant(WGRAD2D_CASES[7]) == "64x64" and _case_variant(WGRAD2D_CASES[8]) == "128x64"


def wgrad2d_ref64(x, dy, k, s, p, d):
    """x [B,H,W,Cin], dy [B,Ho,Wo,Cout] (fp32) -> float64 dW and sum |dy| |x| in the packed column order [Cout][(kh, kw, ci)]"""
    def one(xx, gg):
        g = torch.nn.grad.conv2d_weight(xx.permute(0, 3, 1, 2), (gg.shape[-1], xx.shape[-1], k, k), gg.permute(0, 3, 1, 2), s, p, d)
        return g.permute(0, 2, 3, 1).reshape(gg.shape[-1], -1)
    x64, dy64 = x.double(), dy.double()
    return one(x64, dy64), one(x64.abs(), dy64.abs())


@gpu
@pytest.mark.parametrize("case", WGRAD2D_CASES, ids=lambda c: "x".join(map(str, c[:6])) + f"_s{c[6][0]}{c[6][1]}p{c[7][0]}{c[7][1]}d{c[8][0]}")
def test_wgrad_conv2d_f32_per_element(cuda, case):
    from computervision_codes_amd import ops
    b, h, w, cin, cout, k, s, p, d = case
    ho, wo = _out_size(h, k, s[0], p[0], d[0]), _out_size(w, k, s[1], p[1], d[1])
    x = _u((b, h, w, cin), 1) * pow2_ramp(cin)
    dy = _u((b, ho, wo, cout), 2) * pow2_ramp(cout)
    ref64, acc64 = wgrad2d_ref64(x, dy, k, s, p, d)
    kk, kp, m = k * k * cin, ops.packed_k(cin, k, k, torch.float32), b * ho * wo
    what = f"wgrad_conv2d_f32[{_case_variant(case)}] {case}"
    xd, dyd = x.to(cuda), dy.to(cuda)
    dw = torch.full((cout, kp), 7.0, device=cuda)                    # zeroed by the wrapper, padding columns included
    ops.wgrad_conv2d(dyd, xd, dw, k, k, s, p, d)
    got = dw.cpu()
    check_f32(got[:, :kk], ref64, acc64=acc64, k=m, what=what)
    check_exact(got[:, kk:], torch.zeros(cout, kp - kk), what=what + " padding columns")
    base = _u((cout, kp), 3)                                         # zero=False: accumulate into a non-zero buffer, scaled per element like
    base[:, :kk] *= ref64.abs().float()                              # the result so that the check stays sharp in the small corner tiles
    dw = base.to(cuda)
    ops.wgrad_conv2d(dyd, xd, dw, k, k, s, p, d, zero=False)
    got = dw.cpu()
    check_f32(got[:, :kk], base[:, :kk].double() + ref64, acc64=base[:, :kk].double().abs() + acc64, k=m + 1, what=what + " accumulate")
    check_exact(got[:, kk:], base[:, kk:], what=what + " accumulate padding columns")


# ------------------------------------------------------------------------------------------------ conv1d weight gradient (fp32)
@gpu
@pytest.mark.parametrize("b,t,cout,cin,taps,dil", [(2, 100, 72, 36, 3, 1), (2, 100, 72, 36, 3, 4), (5, 500, 200, 100, 3, 4), (9, 256, 192, 128, 3, 1),
                                                   (3, 700, 40, 20, 3, 1), (10, 2000, 200, 136, 1, 1)])
def test_wgrad_conv1d_per_element(cuda, b, t, cout, cin, taps, dil):
    """`mt4_wgrad_conv1d_f32`: tap shifts across sequence boundaries (dil 1 and 4), the single-split overwrite path (200 rows) and the split
    path (zero-fill + atomics), accumulate, and the fused bias gradient (k = B * T)"""
    from computervision_codes_amd import ops
    pad = dil * (taps - 1) // 2
    x = _u((b, t, cin), 11) * pow2_ramp(cin)
    dy = _u((b, t, cout), 12) * pow2_ramp(cout)
    w = torch.nn.grad.conv1d_weight
    ref64 = w(x.double().permute(0, 2, 1), (cout, cin, taps), dy.double().permute(0, 2, 1), 1, pad, dil).permute(0, 2, 1).reshape(cout, -1)
    acc64 = w(x.double().abs().permute(0, 2, 1), (cout, cin, taps), dy.double().abs().permute(0, 2, 1), 1, pad, dil).permute(0, 2, 1).reshape(cout, -1)
    kk, kp, m = taps * cin, ops.packed_k(cin, 1, taps, torch.float32), b * t
    what = f"wgrad_conv1d_f32 {(b, t, cout, cin, taps, dil)}"
    xd, dyd = x.to(cuda), dy.to(cuda)
    dw = torch.full((cout, kp), 7.0, device=cuda)                    # overwritten, padding columns included
    ops.wgrad_conv1d(dyd, xd, dw, batch=b, t=t, taps=taps, dil=dil, pad=pad)
    got = dw.cpu()
    check_f32(got[:, :kk], ref64, acc64=acc64, k=m, what=what)
    check_exact(got[:, kk:], torch.zeros(cout, kp - kk), what=what + " padding columns")
    base = _u((cout, kp), 13)                                        # scaled per element like the result (see the conv2d test)
    base[:, :kk] *= ref64.abs().float()
    base[:, kk:] = 0.0
    gb0 = _u((cout,), 14) * pow2_ramp(cout)
    dw, gb = base.to(cuda), gb0.to(cuda)
    ops.wgrad_conv1d(dyd, xd, dw, batch=b, t=t, taps=taps, dil=dil, pad=pad, accumulate=True, bias_grad=gb)
    got = dw.cpu()
    check_f32(got[:, :kk], base[:, :kk].double() + ref64, acc64=base[:, :kk].double().abs() + acc64, k=m + 1, what=what + " accumulate")
    check_exact(got[:, kk:], base[:, kk:], what=what + " accumulate padding columns")
    dy2 = dy.double().reshape(m, cout)
    check_f32(gb.cpu(), gb0.double() + dy2.sum(0), acc64=gb0.double().abs() + dy2.abs().sum(0), k=m + 1, what=what + " bias_grad")


# ------------------------------------------------------------------------------------------------ column sums
@gpu
@pytest.mark.parametrize("m,c,ld,off", [(333, 68, 68, 0), (333, 68, 72, 1), (40000, 68, 72, 2), (70000, 200, 204, 3), (7, 4, 8, 0)])
def test_colsum_and_sum_over_batch_per_element(cuda, m, c, ld, off):
    """`mt4_colsum_f32`: more rows than slabs x 64 (the slab count is capped at 1024 / column blocks), ld > C, overwrite and accumulate, outputs
    at any float offset (the neighbours untouched bit for bit); `mt4_sum_over_batch_f32` (sequential fp32 sum over the batch)"""
    from computervision_codes_amd import ops
    full = _u((m, ld), 21) * pow2_ramp(ld)[None] * pow2_ramp(m).flip(0)[:, None]       # per-channel and per-row scales
    x = full[:, :c]
    ref64, acc64 = x.double().sum(0), x.double().abs().sum(0)
    flat0 = torch.full((off + c + 5,), 7.0)
    flat = flat0.to(cuda)
    xd = full.to(cuda)[:, :c]
    ops.colsum(xd, flat[off:off + c])
    got = flat.cpu()
    what = f"colsum {(m, c, ld, off)}"
    check_f32(got[off:off + c], ref64, acc64=acc64, k=m, what=what)
    check_exact(torch.cat([got[:off], got[off + c:]]), torch.cat([flat0[:off], flat0[off + c:]]), what=what + " neighbours")
    base = _u((c,), 22) * pow2_ramp(c)
    flat[off:off + c] = base.to(cuda)
    ops.colsum(xd, flat[off:off + c], accumulate=True)
    got = flat.cpu()
    check_f32(got[off:off + c], base.double() + ref64, acc64=base.double().abs() + acc64, k=m + 1, what=what + " accumulate")
    check_exact(torch.cat([got[:off], got[off + c:]]), torch.cat([flat0[:off], flat0[off + c:]]), what=what + " accumulate neighbours")
    if m % 7 == 0 or m % 5 == 0:                                      # sum over the batch: [batch * L, C] -> [L, C]
        nb = 7 if m % 7 == 0 else 5
        xs = full.contiguous()
        ref = xs.double().view(nb, -1, ld).sum(0)
        acc = xs.double().abs().view(nb, -1, ld).sum(0)
        out = torch.empty(m // nb, ld, device=cuda)
        ops.sum_over_batch(xs.to(cuda), out, nb)
        check_f32(out.cpu(), ref, acc64=acc, k=nb, what=f"sum_over_batch {(nb, m // nb, ld)}")
        o0 = _u((m // nb, ld), 23) * pow2_ramp(ld)
        out = o0.to(cuda)
        ops.sum_over_batch(xs.to(cuda), out, nb, accumulate=True)
        check_f32(out.cpu(), o0.double() + ref, acc64=o0.double().abs() + acc, k=nb + 1, what=f"sum_over_batch accumulate {(nb, m // nb, ld)}")


# ------------------------------------------------------------------------------------------------ BCE with logits (the TeCNO loss)
# expf and log1pf of the device library are accurate to a few ulps; FN_EPS allows four fp32 ulps of every term of a loss sum (so a sum of M terms
# gets 4 x 2^-24 x sum |term|, whatever the sign of the errors) and of every sigmoid.  A sigmoid below the smallest normal fp32 value comes out as
# 0 from the saturated branch (expf(90) = inf, 1 / inf = 0): it is allowed up to 2^-126.
FN_EPS = 4 * EPS
F32_MIN_NORMAL = 2.0 ** -126


@gpu
@pytest.mark.parametrize("m,n,ld_y,ld_dy", [(7, 100, 100, 100), (300, 15, 16, 20), (5000, 6, 8, 12), (4097, 70, 72, 70)])
def test_bce_logits_per_element(cuda, m, n, ld_y, ld_dy):
    """`mt4_bce_logits_f32`: per-column losses (added to what is there) and per-element gradients; row pitches of y and dy above N (the padding
    of dy untouched bit for bit); more rows than the 64-slab cap (64 x 64); logits of +-30 and +-90 (saturated expf: finite and correct)"""
    from computervision_codes_amd import ops
    yfull = _u((m, ld_y), 31) * 8.0
    yfull[0, :n] = torch.tensor([30.0, -30.0, 90.0, -90.0] * n)[:n]
    yfull[m - 1, :n] = torch.tensor([-90.0, 90.0, -30.0, 30.0] * n)[:n]
    z = (_u((m, n), 32) > 0).float()
    sc = pow2_ramp(n) / (m * n)
    cl0 = _u((n,), 33)
    dy0 = torch.full((m, ld_dy), 5.0)
    dyd, cl = dy0.to(cuda), cl0.to(cuda)
    ops.bce_logits(yfull.to(cuda)[:, :n], z.to(cuda), sc.to(cuda), dyd[:, :n], cl)
    y64, z64 = yfull[:, :n].double(), z.double()
    terms = y64.clamp(min=0) - y64 * z64 + torch.log1p(torch.exp(-y64.abs()))
    absterms = y64.clamp(min=0) + (y64 * z64).abs() + torch.log1p(torch.exp(-y64.abs()))
    what = f"bce_logits {(m, n, ld_y, ld_dy)}"
    got_l = cl.cpu()
    check_f32(got_l, cl0.double() + terms.sum(0), acc64=cl0.double().abs() + absterms.sum(0), k=m + 1, extra=FN_EPS * absterms.sum(0),
              what=what + " col_loss")
    s64 = torch.sigmoid(y64)
    sc64 = sc.double()[None]
    got = dyd.cpu()
    assert torch.isfinite(got).all()
    check_f32(got[:, :n], (s64 - z64) * sc64, acc64=(s64 + z64) * sc64, k=2, extra=(FN_EPS * s64 + F32_MIN_NORMAL) * sc64, what=what + " dy")
    check_exact(got[:, n:], dy0[:, n:], what=what + " dy padding")


# ------------------------------------------------------------------------------------------------ SGD and element-wise pieces
@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 1027, 4096 * 33 + 2])
@pytest.mark.parametrize("lr,wd,gs", [(0.05, 1e-5, 1.0), (0.1, 5e-4, 0.25), (0.02, 0.0, 3.0)])
def test_sgd_step_per_element(cuda, n, lr, wd, gs):
    """`mt4_sgd_step_f32`: p -= lr (g gs + wd p) -- float4 body and the scalar tail (n % 4 in 0..3, n < 4); the elements beyond n in a
    larger buffer untouched bit for bit.  Up to four fp32 roundings inside the bracket (hipcc contracts some into FMAs), each a relative 2^-24
    of a term of acc64 = lr (|g gs| + wd |p|): k = 16; the store's own rounding is the half-ulp"""
    from computervision_codes_amd import ops
    guard = 9
    p0 = _u(n + guard, 41) * pow2_ramp(n + guard)
    g0 = _u(n + guard, 42) * pow2_ramp(n + guard) * 2.0 ** -6        # an update small next to p: a wrong weight decay is not hidden by lr |g|
    pb, gb = p0.to(cuda), g0.to(cuda)
    ops.sgd_step(pb[:n], gb[:n], lr, wd, gs)
    ref64, acc64 = sgd_ref64(p0[:n], g0[:n], lr, wd, gs)
    got = pb.cpu()
    what = f"sgd_step n={n} lr={lr} wd={wd} gs={gs}"
    check_f32(got[:n], ref64, acc64=acc64, k=16, what=what)
    check_exact(got[n:], p0[n:], what=what + " beyond n")
    check_exact(gb.cpu(), g0, what=what + " gradient untouched")


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 1000, 65537])
def test_mul_add_and_axpby_per_element(cuda, n):
    """`mt4_mul_add_f32` y = a b (+ c): compiled to one v_fmac_f32 per element (c absent: the addend is 0), so ONE rounding -- RNE agreement
    required.  `mt4_axpby_f32` y = a x + b y (n % 4 == 0 only, by its contract): b = 0 is one rounding (y is not read); otherwise two"""
    from computervision_codes_amd import ops
    a, b, c = (_u(n, 50 + i) * pow2_ramp(n) for i in range(3))
    b = b.flip(0)
    ad, bd, cd = a.to(cuda), b.to(cuda), c.to(cuda)
    ab64 = a.double() * b.double()
    check_f32(ops.mul_add(ad, bd).cpu(), ab64, single_rounding=True, what=f"mul_add n={n}")
    check_f32(ops.mul_add(ad, bd, cd).cpu(), ab64 + c.double(), acc64=ab64.abs() + c.double().abs(), single_rounding=True,
              what=f"mul_add +c n={n}")
    n4 = n - n % 4
    if n4 == 0:
        return
    for alpha, beta in ((3.0, 0.0), (1.0, 1.0), (0.75, -2.5)):
        y0 = torch.full((n4,), float("nan")) if beta == 0.0 else c[:n4].clone()
        yd = y0.to(cuda)
        ops.axpby_(ad[:n4].contiguous(), yd, alpha, beta)
        if beta == 0.0:
            check_f32(yd.cpu(), alpha * a[:n4].double(), single_rounding=True, what=f"axpby a={alpha} b=0 n={n4}")
        else:
            ref = alpha * a[:n4].double() + beta * y0.double()
            acc = abs(alpha) * a[:n4].double().abs() + abs(beta) * y0.double().abs()
            check_f32(yd.cpu(), ref, acc64=acc, k=4, what=f"axpby a={alpha} b={beta} n={n4}")


@gpu
@pytest.mark.parametrize("cout,cin,taps", [(72, 36, 3), (100, 20, 1), (10, 6, 3), (200, 136, 3), (4, 4, 5)])
def test_transpose_pack_conv1d_exact(cuda, cout, cin, taps):
    """`mt4_transpose_pack_conv1d_f32`: the data-gradient weight of the 1-D trainers, [Cin][taps x roundup(Cout, 4)] with taps reversed, equals the
    plain PyTorch construction bit for bit, padding zero -- even when the source's own padding columns hold garbage"""
    from computervision_codes_amd import ops
    kp, kt = ops.packed_k(cin, 1, taps, torch.float32), ops.packed_k(cout, 1, taps, torch.float32)
    tw_s, tw_d = _cdiv(cin, 4) * 4, _cdiv(cout, 4) * 4
    src = _u((cout, kp), 61) * 100.0                                    # padding columns of the source too
    want = torch.zeros(cin, kt)
    for tp in range(taps):
        want[:, tp * tw_d:tp * tw_d + cout] = src[:, (taps - 1 - tp) * tw_s:(taps - 1 - tp) * tw_s + cin].t()
    out = torch.full((cin, kt), 9.0, device=cuda)
    wt = ops.transpose_pack_conv1d(src.to(cuda), cout, cin, taps, out=out)
    check_exact(wt.cpu(), want, what=f"transpose_pack_conv1d {(cout, cin, taps)}")


# ------------------------------------------------------------------------------------------------ conv2d data gradient (SpatialCnnTrainer._dgrad, fp32)
@gpu
@pytest.mark.parametrize("b,h,w,cin,cout,k,s,p", [(2, 14, 18, 64, 96, 3, 1, 1), (2, 9, 11, 256, 64, 1, 1, 0), (3, 16, 12, 64, 136, 3, 2, 1),
                                                  (2, 18, 14, 128, 64, 3, 2, 1), (2, 16, 16, 136, 256, 1, 2, 0), (2, 14, 10, 64, 128, 1, 2, 0)])
def test_dgrad_f32_per_element(cuda, b, h, w, cin, cout, k, s, p):
    """the data gradient of a convolution as the fp32 trainer takes it: stride 1 through the transposed, flipped weight (3x3 and 1x1); stride 2
    3x3 through the four sub-pixel phase kernels and their row maps; stride 2 1x1 into the even positions, with and without a residual.  dy
    carries per-output-channel and the weight per-input-channel power-of-two scales; positions no stride-2 1x1 phase writes hold the residual
    (or zero) bit for bit"""
    from computervision_codes_amd import ops
    from computervision_codes_amd.spatial_cnn_train import SpatialCnnTrainer, _Unit
    ho, wo = _out_size(h, k, s, p, 1), _out_size(w, k, s, p, 1)
    wt = _u((cout, cin, k, k), 71) * pow2_ramp(cin)[None, :, None, None]
    dy = _u((b, ho, wo, cout), 72) * pow2_ramp(cout)
    u = _Unit()
    u.name, u.bn, u.cin, u.cout, u.k, u.stride, u.pad = "c", "b", cin, cout, k, s, p
    u.w = ops.pack_conv_weight(wt.to(cuda), None, torch.float32)
    u.gw = torch.empty_like(u.w)
    u.wt = u.phase_w = None
    tr = SpatialCnnTrainer.__new__(SpatialCnnTrainer)
    tr.units, tr.lin, tr._row_maps, tr.dev = {"c": u}, {}, {}, cuda
    tr._refresh_transposed()
    gx = lambda ww, gg: torch.nn.grad.conv2d_input((b, cin, h, w), ww, gg.permute(0, 3, 1, 2), s, p).permute(0, 2, 3, 1)
    dx64, dxa64 = gx(wt.double(), dy.double()), gx(wt.double().abs(), dy.double().abs())
    for residual in (None, _u((b, h, w, cin), 73) * pow2_ramp(cin)):
        what = f"_dgrad f32 {(b, h, w, cin, cout, k, s, p)} residual={residual is not None}"
        r64 = residual.double() if residual is not None else torch.zeros_like(dx64)
        dx = tr._dgrad(u, dy.to(cuda), (b, h, w, cin), residual.to(cuda) if residual is not None else None).cpu()
        # the reduction runs over the output channels, whose dy scales fall from 2^8 to 2^-8: the partial sum reaches the size of the result
        # after the first terms and every later addition rounds at that size, so the errors add up like a walk of cout k k steps of up to
        # half an ulp of acc64 -- not of the smaller random-walk partial sums sqrt(K) 2^-24 was measured on.  Measured worst err/bound 1.125 at
        # k = cout k k + 1 (a 1x1 layer of 64 -> 256 channels); k is raised 4x (the allowance 2x)
        check_f32(dx, dx64 + r64, acc64=dxa64 + r64.abs(), k=4 * (cout * k * k + 1), what=what)
        if s == 2 and k == 1:
            odd = torch.ones(b, h, w, cin, dtype=torch.bool)
            odd[:, ::2, ::2] = False
            check_exact(dx[odd], r64[odd], what=what + " unwritten positions")


# ------------------------------------------------------------------------------------------------ BatchNorm (fp32), per-channel scales
@gpu
@pytest.mark.parametrize("m,c,relu,res,mean_over_std", [(7, 100, True, False, 1.0), (300, 36, True, True, 1.0), (20000, 196, False, True, 1.0),
                                                        (5000, 68, True, False, 1e3), (2, 4, False, False, 1e3)])
def test_batchnorm_f32_per_element(cuda, m, c, relu, res, mean_over_std):
    """`mt4_bn_stats_f32` / `bn_apply_f32` / `bn_backward_f32` on per-channel power-of-two scales, C not a multiple of 64, M of 2 and 7 and many
    row slabs, channel means 1e3 x the standard deviation; the same bounds and rounding counts as test_gpu_train2d.py::test_batchnorm_train_fwd_bwd,
    and the recomputed-gate path (beta passed) equal to the stored-output gate bit for bit"""
    from computervision_codes_amd import ops
    sc = pow2_ramp(c)
    x = _u((m, c), 81) * sc + mean_over_std * sc * (1.0 + 0.25 * _u((c,), 82))
    g, bt = (_u((c,), 83) + 1.5) * sc.flip(0), _u((c,), 84) * sc
    r = _u((m, c), 85) * sc if res else None
    dy = _u((m, c), 86) * sc.flip(0)
    xd = x.to(cuda)
    mean, invstd = ops.bn_stats(xd)
    y = ops.bn_apply(xd, mean, invstd, g.to(cuda), bt.to(cuda), r.to(cuda) if res else None, relu)
    x64, g64, b64 = x.double(), g.double(), bt.double()
    mu64 = x64.mean(0)
    is64 = 1.0 / torch.sqrt(((x64 - mu64) ** 2).mean(0) + 1e-5)
    xh64 = (x64 - mu64) * is64
    y64 = xh64 * g64 + b64
    acc_y = (x64.abs() + mu64.abs()) * is64 * g64.abs() + b64.abs()
    if res:
        y64, acc_y = y64 + r.double(), acc_y + r.double().abs()
    what = f"bn f32 ramp {(m, c, relu, res, mean_over_std)}"
    check_f32(y.cpu(), torch.relu(y64) if relu else y64, acc64=acc_y, k=25, what=what + " bn_apply")     # (k: see the test below)
    dg, db = torch.zeros(c, device=cuda), torch.zeros(c, device=cuda)
    dx, dres = ops.bn_backward(dy.to(cuda), y if relu else None, xd, mean, invstd, g.to(cuda), dg, db, relu=relu, want_dres=res)
    gate = (y.cpu() > 0) if relu else torch.ones(m, c, dtype=torch.bool)
    dy64 = torch.where(gate, dy.double(), torch.zeros((), dtype=torch.float64))
    m1, m2 = dy64.mean(0), (dy64 * xh64).mean(0)
    acc_dx = g64.abs() * is64 * (dy64.abs() + m1.abs() + (xh64.abs() + (x64.abs() + mu64.abs()) * is64) * (m2.abs() + (dy64 * xh64).abs().mean(0)))
    check_f32(dx.cpu(), g64 * is64 * (dy64 - m1 - xh64 * m2), acc64=acc_dx, k=11, what=what + " bn_backward dx")
    check_f32(db.cpu(), dy64.sum(0), acc64=dy64.abs().sum(0), k=m, what=what + " bn_backward dbeta")
    check_f32(dg.cpu(), (dy64 * xh64).sum(0), acc64=(dy64.abs() * (xh64.abs() + (x64.abs() + mu64.abs()) * is64)).sum(0), k=m,
              what=what + " bn_backward dgamma")
    if res:
        check_exact(dres.cpu(), dy64, what=what + " bn_backward dres")
    if relu and not res:
        dg2, db2 = torch.zeros(c, device=cuda), torch.zeros(c, device=cuda)
        dx2, _ = ops.bn_backward(dy.to(cuda), None, xd, mean, invstd, g.to(cuda), dg2, db2, relu=True, beta=bt.to(cuda))
        check_exact(dx2.cpu(), dx.cpu(), what=what + " recomputed gate dx")
        check_exact(torch.cat([dg2, db2]).cpu(), torch.cat([dg, db]).cpu(), what=what + " recomputed gate dgamma, dbeta")


# ------------------------------------------------------------------------------------------------ pooling backward and the spatial losses (fp32)
@gpu
@pytest.mark.parametrize("b,h,w,c", [(2, 13, 10, 8), (3, 16, 16, 64), (1, 7, 9, 100)])
def test_maxpool3x3s2_bwd_f32_exact_with_ties(cuda, b, h, w, c):
    """`mt4_maxpool3x3s2_bwd_f32`: inputs on a grid of quarters (ties inside most windows: the gradient goes to the first maximum in scan order,
    like torch); dy are multiples of 1/8 times a per-channel power of two, so the (atomic) sums of up to four windows are exact in any order and
    the result must equal torch's bit for bit"""
    from computervision_codes_amd import ops
    x = torch.round(_u((b, c, h, w), 91) * 4) / 4
    xt = x.clone().requires_grad_()
    y = torch.nn.functional.max_pool2d(xt, 3, 2, 1)
    dy = torch.round(_u(tuple(y.shape), 92) * 8) / 8 * pow2_ramp(c)[None, :, None, None]
    y.backward(dy)
    dx = ops.maxpool3x3s2_bwd(x.permute(0, 2, 3, 1).contiguous().to(cuda), dy.permute(0, 2, 3, 1).contiguous().to(cuda))
    check_exact(dx.cpu(), xt.grad.permute(0, 2, 3, 1), what=f"maxpool3x3s2_bwd_f32 {(b, h, w, c)}")


@gpu
@pytest.mark.parametrize("m,n,ld_y,ld_dy", [(5, 12, 12, 12), (300, 100, 104, 100), (4097, 15, 16, 20)])
def test_bce_logits_pw_per_element(cuda, m, n, ld_y, ld_dy):
    """`mt4_bce_logits_pw_f32` (BCEWithLogits with pos_weight): per-column losses added to what is there, per-element gradients, row pitches
    above N, logits up to +-90.  The kernel's roundings per element: 1 - z, pw - 1, lw, log1pf(expf), the max, the sums, 1 + expf, the division,
    lw s, the two subtractions: k = 12 terms of acc64, plus FN_EPS for the device library's expf / log1pf and the underflow of a sigmoid below 2^-126"""
    from computervision_codes_amd import ops
    yfull = _u((m, ld_y), 101) * 8.0
    yfull[0, :n] = torch.tensor([30.0, -30.0, 90.0, -90.0] * n)[:n]
    z = (_u((m, n), 102) > 0).float()
    pw = (_u((n,), 103) + 1.5) * 2.0
    sc = pow2_ramp(n) / (m * n)
    cl0, dy0 = _u((n,), 104), torch.full((m, ld_dy), 5.0)
    dyd, cl = dy0.to(cuda), cl0.to(cuda)
    ops.bce_logits_pw(yfull.to(cuda)[:, :n], z.to(cuda), pw.to(cuda), sc.to(cuda), dyd[:, :n], cl)
    y64, z64, p64 = yfull[:, :n].double(), z.double(), pw.double()[None]
    lw = 1.0 + (p64 - 1.0) * z64
    sp = torch.log1p(torch.exp(-y64.abs())) + (-y64).clamp(min=0)
    terms = (1 - z64) * y64 + lw * sp
    absterms = ((1 - z64) * y64).abs() + lw * sp
    what = f"bce_logits_pw {(m, n, ld_y, ld_dy)}"
    check_f32(cl.cpu(), cl0.double() + terms.sum(0), acc64=cl0.double().abs() + absterms.sum(0), k=m + 1, extra=FN_EPS * absterms.sum(0),
              what=what + " col_loss")
    s64 = torch.sigmoid(y64)
    sc64 = sc.double()[None]
    got = dyd.cpu()
    assert torch.isfinite(got).all()
    check_f32(got[:, :n], ((1 - z64) - lw + lw * s64) * sc64, acc64=((1 - z64) + lw + lw * s64) * sc64, k=12,
              extra=(FN_EPS * lw * s64 + lw * F32_MIN_NORMAL) * sc64, what=what + " dy")
    check_exact(got[:, n:], dy0[:, n:], what=what + " dy padding")


@gpu
@pytest.mark.parametrize("n", [1, 33, 256 * 7 + 5, 100000])
def test_mse_per_element(cuda, n):
    """`mt4_mse_f32`: da = scale 2 d / n (d = a - b: one rounding; then three) and the loss sum of d^2 / n over n elements (wave, block and
    atomic sums), on operands with per-element power-of-two scales"""
    from computervision_codes_amd import ops
    a = _u(n, 111) * pow2_ramp(n)
    bb = _u(n, 112) * pow2_ramp(n)
    scale = 0.3
    ls = torch.zeros(1, device=cuda)
    da = ops.mse(a.to(cuda), bb.to(cuda), ls, scale)
    d64 = a.double() - bb.double()
    acc_d = a.double().abs() + bb.double().abs()
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    check_f32(da.cpu(), s32 * 2.0 * d64 / n, acc64=s32 * 2.0 * acc_d / n, k=16, what=f"mse da n={n}")
    check_f32(ls.cpu(), (d64 * d64 / n).sum().reshape(1), acc64=(acc_d * acc_d / n).sum().reshape(1), k=n + 4, what=f"mse loss n={n}")
