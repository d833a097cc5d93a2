"""CPU: the per-element bounds of test_gpu_seq_train_kernels.py on fp32 emulations of the kernels' own order of operations.

Each emulation (torch on the CPU, fp32 step by step, FMAs where hipcc contracts, a correctly rounded exp / rsqrt in place of the hardware's)
runs through the SAME helper and operand builders as the GPU test and must stay at err/bound <= 0.5: the reference arithmetic alone uses at
most half of a bound, the other half is for what the device does differently (FMA contraction, v_exp / v_rsq / v_rcp, the order of atomics).
The GELU derivative is the exception the bound's own budget names: GELU_BWD_ERR = 5e-7 is 3.2e-7 of formula error + 1.3e-7 of fast-exponential
error, so its emulation may use (5e-7 - 1.3e-7) = 3.7e-7 per unit of |dy|.  Each planted error must fail the check; every test states whether the
assertion of the older GPU tests (a tolerance scaled by the tensor's largest value, or an absolute one) accepts it on the same data.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bf16_bounds import (GELU_BWD_ERR, GELU_BWD_FORMULA_ERR, check_exact, check_f32, half_ulp_f32, layernorm_bwd_ref64, rne_bf16,  # noqa: E402
                         softmax_bwd_ref64, softmax_ref64)
import test_gpu_seq_train_kernels as G  # noqa: E402

F32, F64 = torch.float32, torch.float64
HALF = 0.5
XOR = [torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64, the sum rounds there once (53 bits) and once more to fp32"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _pad(v, width, fill=0.0):
    out = torch.full(v.shape[:-1] + (width,), fill, dtype=v.dtype)
    out[..., :v.shape[-1]] = v
    return out


def _butterfly(lanes):
    """the 6-step __shfl_xor reduction of a wave: [rows, 64] fp32 -> [rows] (every lane ends with the same value: fp32 addition commutes)"""
    for ix in XOR:
        lanes = lanes + lanes[:, ix]
    return lanes[:, 0]


def _wave_sum(v, fma_with=None):
    """[rows, 64 * NI] -> [rows]: lane l sums (or FMAs with `fma_with`) its elements l, l + 64, ... in order, then the butterfly"""
    lanes = torch.zeros(v.shape[0], 64, dtype=F32)
    for i in range(v.shape[1] // 64):
        blk = v[:, 64 * i:64 * (i + 1)]
        lanes = lanes + blk if fma_with is None else _fma(blk, fma_with[:, 64 * i:64 * (i + 1)], lanes)
    return _butterfly(lanes)


def _exp32(x):
    return torch.exp(x.to(F64)).to(F32)


# ------------------------------------------------------------------------------------------------ softmax forward
def softmax_emu(s, scale, bug=None):
    rows, cols = s.shape
    sc = torch.tensor(scale, dtype=F32)
    valid = _pad(torch.ones(rows, cols, dtype=torch.bool), 1024, False)
    v = torch.where(valid, _pad(s, 1024) * sc, torch.tensor(-3.0e38))
    mx = v.max(-1, keepdim=True).values
    if bug == "max_before_scale":
        mx = (s.max(-1, keepdim=True).values * sc)
    e = torch.where(valid, _exp32(v - mx), torch.zeros(()))
    if bug == "pad_lanes_exp":
        e = torch.where(valid, e, _exp32(0.0 - mx).expand(rows, 1024))
    inv = 1.0 / _wave_sum(e)[:, None]
    p = (e * inv)[:, :cols]
    if bug == "small_off":
        p = torch.where(p < 1e-6, p * (1.0 + 2.0 ** -10), p)
    return p


def _old_softmax_accepts(got, ref64):
    """test_softmax_layernorm_gelu_dwconv_backward_vs_autograd: max |err| < 1e-6, absolute (forward and backward)"""
    return bool((got.double() - ref64).abs().max() < 1e-6)


@pytest.mark.parametrize("cols", G.SOFTMAX_COLS)
def test_softmax_emulation_within_half_the_bound(cols):
    worst = 0.0
    for rows in (1, 5):
        for amp in (4.0, 30.0, 300.0):
            for scale in G.SOFTMAX_SCALES:
                s = G.softmax_inputs(rows, cols, amp, 7 * cols + rows)
                p64, extra = softmax_ref64(s, scale)
                worst = max(worst, check_f32(softmax_emu(s, scale), p64, extra=extra, what=f"softmax emulation {(rows, cols, amp, scale)}")["worst_ratio"])
    assert worst <= HALF, worst


@pytest.mark.parametrize("bug,amp,scale,old_accepts", [
    ("max_before_scale", 300.0, -0.3, False),      # exp overflows: inf / NaN, which the old assertion rejects too -- but it has no negative scale at all
    ("pad_lanes_exp", 4.0, 0.3, False),            # 959 pad lanes of a 65-column row add exp(-max) each: every probability shrinks several times
    ("small_off", 30.0, 1.0, True),                # probabilities below 1e-6 off by 2^-10 relative: 1e-9 absolute
])
def test_softmax_planted_errors_rejected(bug, amp, scale, old_accepts):
    s = G.softmax_inputs(5, 65, amp, 460)
    p64, extra = softmax_ref64(s, scale)
    check_f32(softmax_emu(s, scale), p64, extra=extra, what="softmax correct")
    got = softmax_emu(s, scale, bug)
    assert _old_softmax_accepts(got, p64) == old_accepts
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(got, p64, extra=extra, what="softmax " + bug)


def test_softmax_max_before_negative_scale_is_invisible_at_small_logits():
    """softmax is shift invariant: with the maximum taken before a negative scale the shift is the row's minimum, and nothing shows until
    exp(v - min) overflows -- which is why the GPU test runs amplitude 300 at scale -0.3"""
    s = G.softmax_inputs(5, 65, 4.0, 460)
    p64, extra = softmax_ref64(s, -0.3)
    check_f32(softmax_emu(s, -0.3, "max_before_scale"), p64, extra=extra, what="softmax max before scale, amplitude 4")


# ------------------------------------------------------------------------------------------------ softmax backward
def softmax_bwd_emu(p, dp, scale, bug=None):
    rows, cols = p.shape
    sc = torch.tensor(scale, dtype=F32)
    pv, dv = _pad(p, 1024), _pad(dp, 1024)
    dot = _wave_sum(pv, fma_with=dv)[:, None]
    dots = dot.expand(rows, 1024).clone()
    if bug == "dot_missing_in_last_group":
        g0 = (cols - 1) // 64 * 64
        dots[:, g0:] = 0.0
    return (sc * pv * (dv - dots))[:, :cols]


@pytest.mark.parametrize("cols", G.SOFTMAX_COLS)
def test_softmax_bwd_emulation_within_half_the_bound(cols):
    worst = 0.0
    for rows in (1, 5):
        for amp in (4.0, 30.0):
            for scale in G.SOFTMAX_SCALES:
                p, dp = G.softmax_bwd_inputs(rows, cols, amp, scale, 11 * cols + rows)
                ref, extra = softmax_bwd_ref64(p, dp, scale)
                worst = max(worst, check_f32(softmax_bwd_emu(p, dp, scale), ref, extra=extra,
                                             what=f"softmax_bwd emulation {(rows, cols, amp, scale)}")["worst_ratio"])
    assert worst <= HALF, worst


def test_softmax_bwd_dot_left_out_of_the_last_column_group_rejected():
    """columns 128 .. 143 of a 144-column row computed as scale P dP.  The old absolute 1e-6 rejects it on this data too -- but the old test
    has 40 columns: one group of 64, where the planted error and the right code are the same program"""
    p, dp = G.softmax_bwd_inputs(5, 144, 4.0, 0.3, 1589)
    ref, extra = softmax_bwd_ref64(p, dp, 0.3)
    got = softmax_bwd_emu(p, dp, 0.3, "dot_missing_in_last_group")
    assert not _old_softmax_accepts(got, ref)
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(got, ref, extra=extra, what="softmax_bwd dot missing")
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(got[4:], ref[4:], extra=extra[4:], what="softmax_bwd dot missing, smallest row")


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def layernorm_bwd_emu(dy, x, gamma, eps, bug=None, dg0=None, db0=None):
    """(dx, dgamma, dbeta) in the kernel's order: per row the wave reductions; dgamma / dbeta per wave over its grid-strided rows, the waves'
    partial sums then added one after another (the atomics) onto dg0 / db0"""
    m, c = x.shape
    ni = 16 if c <= 1024 else 32 if c <= 2048 else 48
    wd = 64 * ni
    valid = _pad(torch.ones(1, c, dtype=torch.bool), wd, False)
    xv, dv, gm = _pad(x, wd), _pad(dy, wd), _pad(gamma[None], wd)
    inv_c = torch.tensor(1.0, dtype=F32) / torch.tensor(float(c), dtype=F32)
    mean = (_wave_sum(xv) * inv_c)[:, None]
    if bug == "one_pass_variance":
        var = _fma(_wave_sum(xv, fma_with=xv)[:, None], inv_c, -(mean * mean))
        rstd = (1.0 / torch.sqrt(var.to(F64) + float(torch.tensor(eps, dtype=F32)))).to(F32)
    else:
        d = torch.where(valid, xv - mean, torch.zeros(()))
        var = _wave_sum(d, fma_with=d)[:, None]
        rstd = (1.0 / torch.sqrt(_fma(var, inv_c, torch.tensor(eps, dtype=F32)).to(F64))).to(F32)
    xh = (xv - mean) * rstd
    g = dv * gm
    sg = (_wave_sum(g) * (torch.tensor(1.0 / wd, dtype=F32) if bug == "mean_over_lanes" else inv_c))[:, None]
    sgx = (_wave_sum(g, fma_with=xh) * inv_c)[:, None]
    dx = (rstd * _fma(-xh, sgx, _fma(dv, gm, -sg)))[:, :c]
    nw = G.ln_grid(m)[1]
    rounds = -(-m // nw)
    pg, pb = torch.zeros(nw, wd, dtype=F32), torch.zeros(nw, wd, dtype=F32)
    for r in range(rounds - (1 if bug == "dgamma_last_round_missing" else 0)):
        rows = slice(r * nw, min(m, (r + 1) * nw))
        n = rows.stop - rows.start
        pg[:n] = _fma(dv[rows], xh[rows], pg[:n])
        pb[:n] = pb[:n] + dv[rows]
    dg = torch.zeros(c, dtype=F32) if dg0 is None else dg0.clone()
    db = torch.zeros(c, dtype=F32) if db0 is None else db0.clone()
    for w in range(min(nw, m)):
        dg += pg[w, :c]
        db += pb[w, :c]
    return dx, dg, db


def _ln_check(m, c, ratio, bug=None):
    """the checks of test_layernorm_bwd_per_element on the emulation; returns the worst ratios (dx, dgamma, dbeta)"""
    what = f"layernorm_bwd emulation M={m} C={c} mean/std={ratio} bug={bug}"
    x, gamma, dy = G.layernorm_inputs(m, c, ratio, 0, 31)
    dx64, b_dx, _, _, _, _ = layernorm_bwd_ref64(dy, x, gamma, G.LN_EPS)
    dx, _, _ = layernorm_bwd_emu(dy, x, gamma, G.LN_EPS, bug)
    r_dx = check_f32(dx, dx64, extra=b_dx, what=what + " dx")["worst_ratio"]
    x, gamma, dy = G.layernorm_inputs(m, c, ratio, 1, 41)
    _, _, dg64, b_dg, db64, b_db = layernorm_bwd_ref64(dy, x, gamma, G.LN_EPS)
    dg0, db0 = (G._u((c,), 45) * dg64.abs()).float(), (G._u((c,), 46) * db64.abs()).float()
    _, dg, db = layernorm_bwd_emu(dy, x, gamma, G.LN_EPS, bug, dg0, db0)
    r_dg = check_f32(dg, dg0.double() + dg64, acc64=dg0.double().abs(), k=m + 1, extra=b_dg, what=what + " dgamma")["worst_ratio"]
    r_db = check_f32(db, db0.double() + db64, acc64=db0.double().abs(), k=m + 1, extra=b_db, what=what + " dbeta")["worst_ratio"]
    return r_dx, r_dg, r_db


@pytest.mark.parametrize("ratio", [1.0, 100.0])
@pytest.mark.parametrize("m,c", [(1, 7), (5, 32), (77, 96), (77, 1024), (5, 1025), (77, 2049), (5, 3072), (4097, 96), (33000, 96)])
def test_layernorm_bwd_emulation_within_half_the_bound(m, c, ratio):
    assert max(_ln_check(m, c, ratio)) <= HALF


def _old_ln_accepts(got, ref64):
    """test_softmax_layernorm_gelu_dwconv_backward_vs_autograd: max |err| < 2e-5 max(1, max |grad|)"""
    return bool((got.double() - ref64).abs().max() < 2e-5 * max(1.0, ref64.abs().max().item()))


def test_layernorm_bwd_one_pass_variance_rejected():
    """E[x^2] - mean^2 at mean / std = 100 loses 1e4 x 2^-24 of the variance: about 3e-4 relative in rstd, which the old tolerance (2e-5 of the
    largest gradient) rejects as well where it looks -- but its inputs have mean / std = 0 only.  Here every row is held to its own size"""
    m, c = 77, 96
    x, gamma, dy = G.layernorm_inputs(m, c, 100.0, 0, 31)
    dx64, b_dx, _, _, _, _ = layernorm_bwd_ref64(dy, x, gamma, G.LN_EPS)
    dx, _, _ = layernorm_bwd_emu(dy, x, gamma, G.LN_EPS, "one_pass_variance")
    lo = m // 2 + 1
    assert not _old_ln_accepts(dx, dx64)
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(dx, dx64, extra=b_dx, what="one-pass variance")
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(dx[lo:], dx64[lo:], extra=b_dx[lo:], what="one-pass variance, rows scaled 1 and below")


def test_layernorm_bwd_mean_over_lanes_rejected():
    """mean(g) divided by the 1024 lanes x registers instead of C = 96: wrong by 10x in every row (the old tolerance rejects it as well)"""
    x, gamma, dy = G.layernorm_inputs(77, 96, 1.0, 0, 31)
    dx64, b_dx, _, _, _, _ = layernorm_bwd_ref64(dy, x, gamma, G.LN_EPS)
    dx, _, _ = layernorm_bwd_emu(dy, x, gamma, G.LN_EPS, "mean_over_lanes")
    assert not _old_ln_accepts(dx, dx64)
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(dx, dx64, extra=b_dx, what="mean over lanes")


def test_layernorm_bwd_dgamma_last_round_missing_rejected():
    """33000 rows over 4096 waves: the ninth round (rows 32768 ..) left out of dgamma / dbeta.  The old tolerance, scaled by the largest
    channel's gradient, accepts it in the channels scaled 2^-4 and below"""
    m, c = 33000, 96
    x, gamma, dy = G.layernorm_inputs(m, c, 1.0, 1, 41)
    _, _, dg64, b_dg, db64, b_db = layernorm_bwd_ref64(dy, x, gamma, G.LN_EPS)
    _, dg, db = layernorm_bwd_emu(dy, x, gamma, G.LN_EPS, "dgamma_last_round_missing")
    tol = 2e-5 * max(1.0, dg64.abs().max().item())
    assert bool(((dg.double() - dg64).abs()[72:] < tol).all()) and not _old_ln_accepts(dg, dg64)
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(dg[72:], dg64[72:], extra=b_dg[72:], what="dgamma last round missing, small channels")
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(db[72:], db64[72:], extra=b_db[72:], what="dbeta last round missing, small channels")


# ------------------------------------------------------------------------------------------------ GELU derivative
def gelu_bwd_emu(dy, x, phi_const=0.3989422804014327):
    v = x.to(F32)
    c = lambda f: torch.tensor(f, dtype=F32)
    ax = v.abs() * c(0.70710678118654752440)
    t = (1.0 / _fma(c(0.3275911), ax, c(1.0)).to(F64)).to(F32)
    pl = _fma(c(1.061405429), t, c(-1.453152027))
    pl = _fma(pl, t, c(1.421413741))
    pl = _fma(pl, t, c(-0.284496736))
    pl = _fma(pl, t, c(0.254829592))
    ex = _exp32(-(ax * ax))
    erfa = _fma(-(pl * t), ex, c(1.0))
    phi_ = c(0.5) * (c(1.0) + torch.copysign(erfa, v))
    return dy.to(F32) * _fma(v * c(phi_const), ex, phi_)


def test_gelu_bwd_formula_error():
    """the Abramowitz-Stegun form in fp32 against the exact derivative over 2 x 10^6 points of [-12, 12]: at most GELU_BWD_FORMULA_ERR (measured
    3.2e-7, at x = 0.06), which leaves 1.3e-7 of GELU_BWD_ERR for the hardware exponential"""
    x = torch.linspace(-12.0, 12.0, 2_000_001, dtype=F64).to(F32)
    one = torch.ones_like(x)
    err = (gelu_bwd_emu(one, x).double() - G.gelu_bwd_ref64(one, x)).abs()
    worst = err.max().item()
    print(f"gelu_bwd formula error {worst:.3e} at x = {x[int(err.argmax())].item():.4f}")
    assert worst <= GELU_BWD_FORMULA_ERR and GELU_BWD_FORMULA_ERR + 1.3e-7 <= GELU_BWD_ERR + 1e-12


@pytest.mark.parametrize("n", [4, 8, 1028, 2 ** 20 + 4])
def test_gelu_bwd_emulation_within_its_share_of_the_bound(n):
    x, dy = G.gelu_inputs(n, 51)
    st = check_f32(gelu_bwd_emu(dy, x), G.gelu_bwd_ref64(dy, x), extra=GELU_BWD_ERR * dy.double().abs(), what=f"gelu_bwd emulation n={n}")
    assert st["worst_ratio"] <= GELU_BWD_FORMULA_ERR / GELU_BWD_ERR


def test_gelu_bwd_truncated_phi_constant_rejected():
    """phi's 1 / sqrt(2 pi) truncated to 0.39894: 2.3e-6 |x| exp(-x^2 / 2), up to 1.4e-6 |dy| -- inside the old absolute 2e-6 for |dy| <= 1"""
    g = torch.Generator().manual_seed(18)
    x, dy = (torch.rand(3200, generator=g) * 2 - 1) * 4.0, torch.rand(3200, generator=g) * 2 - 1
    ref = G.gelu_bwd_ref64(dy, x)
    check_f32(gelu_bwd_emu(dy, x), ref, extra=GELU_BWD_ERR * dy.double().abs(), what="gelu_bwd correct")
    got = gelu_bwd_emu(dy, x, phi_const=0.39894)
    assert (got.double() - ref).abs().max() < 2e-6
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_f32(got, ref, extra=GELU_BWD_ERR * dy.double().abs(), what="gelu_bwd truncated phi constant")


# ------------------------------------------------------------------------------------------------ depthwise Conv1d backward
def dwconv_bwd_emu(x, dy, w, dw0, db0, bug=None):
    """slabs of 32 rows per sequence, one thread per channel (vectorised over channels); a slab's sums run in float64 and are rounded to fp32
    once, then added to dw / db one after another (the atomics).  bug "slab_sums_in_f32": the fp32 FMA chain the kernel had before"""
    b, t, c = x.shape
    w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
    zero = torch.zeros(c, dtype=F32)
    f32_sums = bug == "slab_sums_in_f32"
    dx, dw, db = torch.empty_like(x), dw0.clone(), db0.clone()
    for s in range(b):
        for t0 in range(0, t, G.DW_SLAB):
            t1 = min(t, t0 + G.DW_SLAB)
            a0, a1, a2, ab = (torch.zeros(c, dtype=F32 if f32_sums else F64) for _ in range(4))
            dprev = dy[s, t0 - 1] if t0 > 0 else zero
            xprev = x[s, t0 - 1] if t0 > 0 else zero
            if bug == "xprev_across_sequences" and t0 == 0 and s > 0:
                xprev = x[s - 1, t - 1]
            if bug == "dprev_zero_at_slab_start":
                dprev = zero
            dcur, xcur = dy[s, t0], x[s, t0]
            for tt in range(t0, t1):
                dnext = dy[s, tt + 1] if tt + 1 < t else zero
                xnext = x[s, tt + 1] if tt + 1 < t else zero
                dx[s, tt] = _fma(w2, dprev, _fma(w1, dcur, w0 * dnext))
                if f32_sums:
                    a0, a1, a2, ab = _fma(dcur, xprev, a0), _fma(dcur, xcur, a1), _fma(dcur, xnext, a2), ab + dcur
                else:
                    dc = dcur.double()
                    a0, a1, a2, ab = a0 + dc * xprev.double(), a1 + dc * xcur.double(), a2 + dc * xnext.double(), ab + dc
                dprev, dcur, xprev, xcur = dcur, dnext, xcur, xnext
            dw[:, 0] += a0.to(F32)
            dw[:, 1] += a1.to(F32)
            dw[:, 2] += a2.to(F32)
            db += ab.to(F32)
    return dx, dw, db


def _dw_check(b, t, c, boundary, bug=None, assert_dw=True):
    """the checks of the GPU tests on the emulation: dx (k = 4), dw / db at k = `dw_k`; returns the ratios [dx, dw, db]"""
    x, dy, w = G.dwconv_inputs(b, t, c, 61 + c, boundary)
    dx64, adx, dw64, adw, db64, adb = G.dwconv_bwd_ref64(x, dy, w)
    dw0, db0 = (G._u((c, 3), 64) * dw64.abs()).float(), (G._u((c,), 65) * db64.abs()).float()
    dx, dw, db = dwconv_bwd_emu(x, dy, w, dw0, db0, bug)
    what = f"dwconv1d_k3_bwd emulation B={b} T={t} C={c} boundary={boundary} bug={bug}"
    r_dx = check_f32(dx, dx64, acc64=adx, k=4, what=what + " dx")["worst_ratio"]
    if assert_dw:
        check_f32(dw, dw0.double() + dw64, acc64=dw0.double().abs() + adw, k=G.dw_k(b, t), what=what + " dw")
        check_f32(db, db0.double() + db64, acc64=db0.double().abs() + adb, k=G.dw_k(b, t), what=what + " db")
    bound = lambda ref, acc: half_ulp_f32(ref) + math.sqrt(G.dw_k(b, t)) * 2.0 ** -24 * acc
    r_dw = ((dw.double() - dw0.double() - dw64).abs() / bound(dw0.double() + dw64, dw0.double().abs() + adw)).max().item()
    r_db = ((db.double() - db0.double() - db64).abs() / bound(db0.double() + db64, db0.double().abs() + adb)).max().item()
    return [r_dx, r_dw, r_db]


DW_EMU_CASES = [(1, 1, 3), (3, 2, 1), (3, 33, 257), (1, 65, 255), (3, 64, 3), (3, 256, 4), (1, 31, 257), (1, 32, 257), (1, 45, 257)]


@pytest.mark.parametrize("b,t,c", DW_EMU_CASES)
def test_dwconv_bwd_emulation_dw_db_within_half_the_bound(b, t, c):
    """dw / db: half the bound, with and without the 2^8 larger boundary rows.  dx is the exception: its bound COUNTS the worst case of its two
    intermediate roundings (k = 4) instead of estimating a random walk, and holds for the contracted (2 FMAs) and the plain (3 products, 2
    sums) compilation alike, so among thousands of elements a correct kernel comes close to it; dx has to stay inside"""
    for boundary in (True, False):
        r_dx, r_dw, r_db = _dw_check(b, t, c, boundary)
        assert r_dx <= 1.0 and max(r_dw, r_db) <= HALF, (boundary, r_dx, r_dw, r_db)


def test_dwconv_bwd_emulation_exceeds_sqrt_k_on_boundary_scaled_rows():
    """why the kernel sums a slab in float64: with an fp32 FMA chain, dy[1] x[0] -- 2^8 larger than the 29 products that follow it in the slab --
    makes every later addition round at its size, and dw[14][0] of B = 1, T = 31, C = 257 ends at 1.66 of sqrt(B T + 1) 2^-24 acc64 (the
    device returned the same bits, -140.7445831298828 against -140.74468020086883, before the kernel was changed)"""
    r_dx, r_dw, r_db = _dw_check(1, 31, 257, True, "slab_sums_in_f32", assert_dw=False)
    assert r_dx <= 1.0 and 1.5 < r_dw < 1.8, (r_dx, r_dw, r_db)
    with pytest.raises(AssertionError, match=r"dw: f32 bound exceeded.*worst element \(14, 0\)"):
        _dw_check(1, 31, 257, True, "slab_sums_in_f32")


@pytest.mark.parametrize("bug", ["xprev_across_sequences", "dprev_zero_at_slab_start"])
def test_dwconv_bwd_planted_errors_rejected(bug):
    """a row carried across a sequence boundary into dw's first tap (seen by dw); dy[t0 - 1] missing from dx at the first row of every slab but
    the first (seen by dx, k = 4).  The boundary rows are 2^8 larger, so the old tolerances reject both on this data as well -- the old
    test's own data (one T = 45, |x| <= 1) has a single slab edge and no scaled boundary rows"""
    _dw_check(3, 65, 257, True)
    with pytest.raises(AssertionError, match="bound exceeded"):
        _dw_check(3, 65, 257, True, bug)
    if bug == "xprev_across_sequences":                  # ... and without the larger boundary rows
        _dw_check(3, 65, 257, False)
        with pytest.raises(AssertionError, match="dw: f32 bound exceeded"):
            _dw_check(3, 65, 257, False, bug)


# ------------------------------------------------------------------------------------------------ relative-position table gradient
def relpos_emu(ds, idx, ts, t0, bug=None):
    """per head and run of `per` windows: four strided running sums + a tail into the first, (s0 + s1) + (s2 + s3), folded into the LDS column in
    (i, j) order, the column added to the table run after run"""
    nw, h, n, _ = ds.shape
    nn = n * n
    d = ds.reshape(nw, h, nn)
    per = G.relpos_per(nw, h)
    ix = idx.long()
    rank = torch.zeros(nn, dtype=torch.long)                 # the r-th (i, j) of its table row: one vector ds_add per rank
    seen = {}
    for ij in range(nn):
        r = int(ix[ij])
        rank[ij] = seen.get(r, 0)
        seen[r] = rank[ij] + 1
    tab_out = t0.clone()
    for w0 in range(0, nw, per):
        w1 = min(nw, w0 + per)
        s = [torch.zeros(h, nn, dtype=F32) for _ in range(4)]
        w = w0
        while w + 4 <= w1:
            for j in range(4):
                s[j] = s[j] + d[w + j]
            w += 4
        if bug != "tail_skipped":
            while w < w1:
                s[0] = s[0] + d[w]
                w += 1
        tot = (s[0] + s[1]) + (s[2] + s[3])
        col = torch.zeros(ts, h, dtype=F32)
        for r in range(int(rank.max()) + 1):
            sel = rank == r
            col[ix[sel]] = col[ix[sel]] + tot[:, sel].t()
        tab_out += col
    return tab_out


def _relpos_check(ws, heads, nw, bug=None):
    ds, idx, ts = G.relpos_inputs(ws, heads, nw, 81)
    ref, acc, terms = G.relpos_ref64(ds, idx, ts)
    t0 = (G._u((ts, heads), 82) * ref.abs()).float()
    got = relpos_emu(ds, idx, ts, t0, bug)
    old = bool((got.double() - t0.double() - ref).abs().max() < 1e-5 * ref.abs().max())
    return old, check_f32(got, t0.double() + ref, acc64=(t0.double().abs() + acc) * G._count_k(terms + 1), k=1,
                          what=f"relpos emulation {(ws, heads, nw)} bug={bug}")["worst_ratio"]


@pytest.mark.parametrize("ws,heads,nw", [(7, 3, 8), (12, 4, 1), (12, 4, 3), (7, 1, 5), (4, 2, 64), (7, 3, 1000), (1, 2, 3)])
def test_relpos_emulation_within_half_the_bound(ws, heads, nw):
    assert _relpos_check(ws, heads, nw)[1] <= HALF


def test_relpos_tail_windows_skipped_rejected():
    """a run of 6 windows = one 4-unrolled round + a tail of 2 (and the 1-window last run of 5 windows at per = 4): the tail left out"""
    for case in ((7, 3, 1000), (7, 1, 5)):
        assert G.relpos_per(case[2], case[1]) % 4 or case[2] % 4
        with pytest.raises(AssertionError, match="bound exceeded"):
            _relpos_check(*case, bug="tail_skipped")


# ------------------------------------------------------------------------------------------------ derived-weight refresh
def refresh_emu(src, cout, cin, bf16, transposed, tap_map, kpad_dst, bug=None):
    """the kernel's walk over 32 x 32 tiles of one entry: only valid elements are written into the zeroed destination; bf16 by RNE"""
    tw_s = G._r4(cin)
    rows, cols = (cin, cout) if transposed else (cout, cin)
    tw_d = (cols + 7) // 8 * 8 if bf16 else G._r4(cols)
    dst = torch.zeros(rows * kpad_dst, dtype=F64)
    for tp, st in enumerate(tap_map):
        for n0 in range(0, cout, 32):
            for c0 in range(0, cin, 32):
                nn, cc = torch.arange(n0, min(cout, n0 + 32)), torch.arange(c0, min(cin, c0 + 32))
                v = src[nn][:, st * tw_s + cc].double()                                    # [n, c]
                ragged = n0 + 32 > cout or c0 + 32 > cin
                if transposed and not (bug == "plain_pitch_in_ragged_tile" and ragged):
                    o = cc[None, :] * kpad_dst + tp * tw_d + nn[:, None]
                else:
                    o = nn[:, None] * kpad_dst + tp * tw_d + cc[None, :]
                ok = o < dst.numel()
                dst[o[ok]] = v[ok]
    dst = dst.view(rows, kpad_dst)
    if not bf16:
        return dst
    if bug == "truncate":
        return (dst.float().view(torch.int32) & ~0xFFFF).view(F32).double()
    return rne_bf16(dst)


def test_refresh_emulation_exact_and_planted_errors_rejected():
    """the tile walk equals the host construction of the GPU test for every entry of its table; truncation to bf16 and a transposed destination
    written with the plain pitch in its ragged tiles are both seen by check_exact"""
    ents = G.refresh_entries()
    tiles = [G.refresh_tiles(co, ci, len(tm)) for co, ci, _, _, _, tm, _ in ents]
    assert any(t == 1 for t in tiles[1:-1]) and any(t % G.REFRESH_TILES_PER_BLOCK for t in tiles if t > G.REFRESH_TILES_PER_BLOCK) and len(ents) >= 8
    seen_trunc = seen_pitch = 0
    for i, (co, ci, taps, bf, tr, tm, sh) in enumerate(ents):
        src = G.refresh_master(co, ci, taps, 200 + i)
        rows, cols = (ci, co) if tr else (co, ci)
        kpad = (len(tm) * ((cols + 7) // 8 * 8 if bf else G._r4(cols)) + (63 if bf else 31)) // (64 if bf else 32) * (64 if bf else 32)
        want = G.refresh_want(src, co, ci, bf, tr, tm, kpad)
        cast = (lambda v: v.to(torch.bfloat16)) if bf else (lambda v: v.float())
        check_exact(cast(refresh_emu(src, co, ci, bf, tr, tm, kpad)), want, what=f"refresh emulation entry {i}")
        if bf:
            seen_trunc += 1
            with pytest.raises(AssertionError, match="exact copy differs"):
                check_exact(cast(refresh_emu(src, co, ci, bf, tr, tm, kpad, "truncate")), want, what="refresh truncating")
        if tr and (co % 32 or ci % 32) and co != ci:
            seen_pitch += 1
            with pytest.raises(AssertionError, match="exact copy differs"):
                check_exact(cast(refresh_emu(src, co, ci, bf, tr, tm, kpad, "plain_pitch_in_ragged_tile")), want, what="refresh plain pitch")
    assert seen_trunc >= 8 and seen_pitch >= 8


def test_refresh_master_holds_bf16_ties():
    """the masters of the refresh test hold exact ties under an even and an odd upper half-word: RNE keeps the even one, rounds the odd one up"""
    src = G.refresh_master(4, 8, 1, 1)
    bits = src.view(torch.int32)
    assert (bits[:, 0] & 0x1FFFF).tolist() == [0x8000] * 4 and (bits[:, 1] & 0x1FFFF).tolist() == [0x18000] * 4
    r = rne_bf16(src[:, :2]).float().view(torch.int32)
    assert torch.equal(r[:, 0], bits[:, 0] & ~0xFFFF) and torch.equal(r[:, 1], (bits[:, 1] & ~0xFFFF) + 0x10000)
