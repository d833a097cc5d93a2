"""Per-element error bounds for kernels that read bf16 operands, accumulate in fp32 and round once when they store.

A correct kernel of that kind is, on every element, within half a bf16 ulp of the exact (float64) result of the operation on the same bf16
operands, plus a small term for its fp32 accumulation.  A single tolerance scaled by the tensor's largest value allows several ulps at the largest
element and far more near zero, so a truncating store, a bias read as bf16 or a K-split partial sum rounded to bf16 all pass it; these bounds
do not (`test_bf16_bounds_cpu.py` shows both on CPU emulations of those bugs).

`check_bf16` asserts, for every element,

    |got - ref64| <= half_ulp_bf16(|ref64| + slack) + slack,   slack = sqrt(k) * ACC_EPS * acc64 + extra

(the half ulp of the store belongs to the value the kernel rounds, up to `slack` away from ref64: next to a power of two that is the next binade) and, when the reference rounds in exactly the places the kernel does (`single_rounding`), that the outputs equal the round-to-nearest-even of the
float64 result almost everywhere and that their signed error has no bias (these two catch truncation and one-sided errors at long K, where the
accumulation term is loose).  `check_f32` is the same bound for fp32 outputs (of bf16 or of fp32 operands), with an fp32 half-ulp in place of the
bf16 one; its `single_rounding` asks the same of RNE-to-fp32.  `check_exact` is for kernels that only move data: every element bit for bit.

This is a plain module imported by the GPU tests (`tests/` is on sys.path while pytest runs them), not a conftest.
"""
import json
import math
import os

import numpy as np
import torch

# fp32 accumulation term per sqrt(K), times sum |a * b| (acc64).  The fp32 MFMA chain was measured at about 1-3.5e-7 * sum |a * b| for
# K <= 4096 (one fp32 rounding per step, errors of random sign): sqrt(K) * 2^-24 is about ten times that.  How the bf16 MFMA sums inside one
# instruction has not been measured here; if a correct kernel exceeds this term, and the fp32-output form of the same kernel does too, it is
# raised here, once, with the measured worst ratio.
ACC_EPS = 2.0 ** -24

# gelu_erf (computervision_codes_amd/csrc/mt4_common.h): |gelu_erf - exact| < 9e-7 over [-10, 10] in fp32, documented in the header; and the
# accumulation error of the argument reaches the output through gelu', whose largest value is 1.129 (at x = sqrt 2).
GELU_APPROX_ERR = 1e-6
GELU_MAX_SLOPE = 1.13

# `__expf(x)` (one v_exp_f32 of x * log2(e)): the relative error allowed to it.  The product x * log2(e) is rounded once and the constant
# log2(e) is itself rounded to fp32: each moves the argument of 2^y by up to |x| log2(e) 2^-24, i.e. the result by |x| 2^-24 relative
# (d 2^y / 2^y = ln 2 dy): 2 |x| 2^-24 together.  The hardware exponential is ASSUMED good to one ulp (2^-23 relative = 2 x 2^-24) and as much
# again is allowed for its input denormal handling and range reduction: the constant 4.  Not measured on this part; if a correct kernel
# exceeds a bound because of it, the constant becomes 1.5 x the measured worst error and the measured value is written here.
def FAST_EXP(x):
    """relative error bound of `__expf(x)`: (4 + 2 |x|) 2^-24 (float64 tensor in, float64 tensor out)"""
    return (4.0 + 2.0 * x.to(torch.float64).abs()) * ACC_EPS


# gelu_bwd_kernel (csrc/seq_train_kernels.hip): dy * (Phi(x) + x phi(x)) with Phi from the Abramowitz-Stegun 7.1.26 erf.  Per unit of |dy|:
# an fp32 emulation of that form against the exact derivative over 2 x 10^6 points of [-12, 12] is off by at most 3.2e-7 (at x = 0.06;
# re-measured by test_seq_bounds_cpu.py::test_gelu_bwd_formula_error), and FAST_EXP reaches the result through 0.5 pl t + 0.399 |x|
# (both multiply exp(-x^2 / 2), whose relative error is (4 + x^2) 2^-24) as at most 1.3e-7 (at |x| about 1.6).  3.2e-7 + 1.3e-7 -> 5e-7.
GELU_BWD_ERR = 5e-7
GELU_BWD_FORMULA_ERR = 3.7e-7          # = GELU_BWD_ERR - 1.3e-7: what the emulated formula alone may use

# single-rounding statistics, over the outputs where the documented approximation (`extra`) is at most 1/16 ulp -- it cannot move their rounding
# much (GELU: every output of magnitude >= 2^-9; below that gelu_erf's 9e-7 spans ulps, and outputs of x < -5 are all off by most of it):
# at least this fraction of them equals RNE(float64) ...
MIN_MATCH = 0.99
# ... and the mean signed error (in ulps, towards larger magnitude) stays below this.  For n nonzero outputs the mean of n independent rounding
# errors (uniform, sigma = 0.29 ulp) has a standard deviation of 0.29 / sqrt(n): below n = 576 the threshold is four of those, 1.2 / sqrt(n).
MAX_MEAN_SIGNED = 0.05

BF16_MIN_NORMAL_EXP = -126


def _floor_log2(t64):
    """floor(log2 |t|) of a float64 tensor, floored at the smallest normal exponent (0 maps there too)"""
    _, e = torch.frexp(t64)                 # t = m * 2^e, 0.5 <= |m| < 1
    e = torch.where(t64 == 0, torch.full_like(e, BF16_MIN_NORMAL_EXP + 1), e)
    return torch.clamp(e.to(torch.float64) - 1.0, min=BF16_MIN_NORMAL_EXP)


def half_ulp_bf16(ref):
    """half a bf16 ulp of each element of `ref`: 2^(floor(log2 |ref|) - 8), floored at the smallest normal"""
    return torch.pow(2.0, _floor_log2(ref.to(torch.float64)) - 8.0)


def half_ulp_f32(ref):
    """half an fp32 ulp of each element of `ref`: 2^(floor(log2 |ref|) - 24), floored at the smallest normal"""
    return torch.pow(2.0, _floor_log2(ref.to(torch.float64)) - 24.0)


def rne_f32(t):
    """round to fp32 with round-to-nearest-even, directly from float64, widened back to float64 (torch's float64 -> float32 cast is RNE)"""
    return t.to(torch.float64).to(torch.float32).to(torch.float64)


def rne_bf16(t):
    """round to bf16 with round-to-nearest-even, directly from float64 (no intermediate fp32 rounding), widened back to float64"""
    t64 = t.to(torch.float64)
    ulp = torch.pow(2.0, _floor_log2(t64) - 7.0)
    return torch.round(t64 / ulp) * ulp     # torch.round: halves to even; t / ulp is exact (power-of-two scale)


def pow2_ramp(n):
    """operand scales 2^8 .. 2^-8 (powers of two: they add no rounding), descending with the index -- per channel or per row of a test operand, so
    that the ragged tail tiles of a kernel hold the smallest values and a small-magnitude region has to be right on its own"""
    return torch.pow(2.0, torch.round(torch.linspace(8.0, -8.0, n)))


def sgd_ref64(p, g, lr, wd, gs):
    """float64 of `p - lr * (g * gs + wd * p)` (mt4_sgd_step_f32) on fp32 p, g and the fp32 values of the scalars (the kernel's arguments are
    floats); returns (ref64, acc64) with acc64 = lr (|g gs| + wd |p|), the terms inside the bracket whose roundings reach the result"""
    lr, wd, gs = (float(torch.tensor(v, dtype=torch.float32)) for v in (lr, wd, gs))
    p64, g64 = p.double(), g.double()
    return p64 - lr * (g64 * gs + wd * p64), lr * (g64.abs() * abs(gs) + abs(wd) * p64.abs())


def softmax_ref64(s, scale):
    """`softmax_rows_kernel`: p = softmax(scale * s) over the last axis, float64 of the fp32 logits and the fp32 value of `scale`.
    Returns (p64, extra): `extra` is the bound below without its half ulp, which `check_f32(extra=...)` adds itself.  The bound is RELATIVE
    TO EACH p_i (not to the row maximum).  With u = 2^-24, v = scale s, x_i = v_i - max v:
      rho_i = u (|v_i| + |max v| + |x_i|) + FAST_EXP(x_i)   -- the roundings of v_i, of max v and of their difference are absolute errors of
              the exponent, i.e. relative errors of e_i = exp(x_i); then `__expf` itself
      the sum of the e_j carries sum_j p_j rho_j (relative, propagated) and sqrt(cols) u of its own additions (16 strided terms per lane and
      a 6-step butterfly: positive terms, so acc64 is the sum itself); 1 / sum, the product e_i * inv and slack: 4 u
      bound_i = p_i (rho_i + sum_j p_j rho_j + (sqrt(cols) + 4) u) + half_ulp_f32(p_i) + 2^-126
    (2^-126: an e_i below the smallest normal is flushed to zero by the hardware exponential)"""
    scale = float(torch.tensor(scale, dtype=torch.float32))
    v = scale * s.to(torch.float64)
    mx = v.max(-1, keepdim=True).values
    x = v - mx
    e = torch.exp(x)
    p = e / e.sum(-1, keepdim=True)
    rho = ACC_EPS * (v.abs() + mx.abs() + x.abs()) + FAST_EXP(x)
    rel = rho + (p * rho).sum(-1, keepdim=True) + (math.sqrt(s.shape[-1]) + 4.0) * ACC_EPS
    return p, p * rel + 2.0 ** -126


def softmax_bwd_ref64(p, dp, scale):
    """`softmax_bwd_rows_kernel`: ds = scale p (dp - dot), dot = sum_j p_j dp_j, float64 of the fp32 p and dp.  Returns (ds64, extra), extra
    being the bound without the half ulp that `check_f32` adds:
      dot: sqrt(cols) u sum_j |p_j dp_j| (its additions) -- an ABSOLUTE error, which reaches ds_i multiplied by |scale| p_i
      dp_i - dot: u |dot| covers the rounding of dot's own last additions seen from the difference, and the difference, the product with p_i
      and the product with scale are three roundings relative to the result: 3 u |dp_i - dot|
      bound_i = |scale| p_i (sqrt(cols) u sum_j |p_j dp_j| + u |dot| + 3 u |dp_i - dot|) + half_ulp_f32(ds_i) + 2^-149 (1 + |dp_i - dot|)
    The last term is gradual underflow, which the relative terms do not model: a product below the smallest normal (a masked probability of
    1e-42 times anything) lands on the denormal grid, off by up to 2^-150 whatever its size; scale p_i does, and is then multiplied by
    dp_i - dot, and the final product does.  Taken twice (2^-149), because results ON that grid are off by up to the whole of the worst case."""
    scale = float(torch.tensor(scale, dtype=torch.float32))
    p64, d64 = p.to(torch.float64), dp.to(torch.float64)
    dot = (p64 * d64).sum(-1, keepdim=True)
    adot = (p64 * d64).abs().sum(-1, keepdim=True)
    ref = scale * p64 * (d64 - dot)
    bound = abs(scale) * p64.abs() * (math.sqrt(p.shape[-1]) * ACC_EPS * adot + ACC_EPS * dot.abs() + 3.0 * ACC_EPS * (d64 - dot).abs())
    return ref, bound + 2.0 ** -149 * (1.0 + (d64 - dot).abs())


def layernorm_bwd_ref64(dy, x, gamma, eps):
    """`layernorm_bwd_kernel`: g = dy gamma; dx = rstd (g - mean(g) - xhat mean(g xhat)); dgamma = sum_rows dy xhat; dbeta = sum_rows dy, in
    float64 on the fp32 dy [M, C], x [M, C], gamma [C] and the fp32 value of eps.  Returns (dx, bound_dx, dgamma, bound_dgamma, dbeta,
    bound_dbeta); the bounds are `extra` arguments of `check_f32`, which adds the output's own half ulp.  First-order propagation, u = 2^-24,
    s = sqrt(C) (the random-walk factor of a C-term fp32 sum), d = x - mean, xh = d rstd, sg = mean(g), sgx = mean(g xh):
      A     = s u mean|x| + u |mean|                      the row mean: its C additions, and the product with 1 / C
      rho   = (s + 8) u + 2 A mean|d| / (var + eps)       rstd, relative: half the relative error of var + eps (s u from the additions of
                                                          d^2, 2 u from squaring rounded d's, the error A of the mean entering through
                                                          d var = 2 A mean|d|) plus rsqrtf, ASSUMED good to one ulp, 1 / C and eps: the 8
      dxh   = rstd (A + u |d|) + |xh| (rho + u)           xhat, absolute: the mean's error and the rounding of d, scaled; rstd's; the product
      Esg   = s u mean|g| + 2 u |sg|                      mean(g): additions; g's own rounding and the product with 1 / C
      Esgx  = s u mean|g xh| + mean(|g| dxh) + 2 u |sgx|  mean(g xh): the same, plus xhat's error through every term
      inner = |g| + |sg| + |xh sgx|
      bound_dx     = rstd (Esg + dxh |sgx| + |xh| Esgx + 4 u inner) + rho rstd inner     (4: g, xh sgx, the two subtractions ... and rstd x)
      bound_dgamma = sqrt(M) u sum|dy xh| + sum(|dy| dxh) + u sum|dy xh|                 (additions over the rows; xhat's error; the products)
      bound_dbeta  = (sqrt(M) + 2) u sum|dy|             (+ 2: a wave's own rows are few -- below 16 terms sqrt(n) is under the worst case --
                                                          and the waves' partial sums are then added by atomics in any order)"""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    u = ACC_EPS
    dy64, x64, g64 = dy.to(torch.float64), x.to(torch.float64), gamma.to(torch.float64)
    m, c = x64.shape
    s = math.sqrt(c)
    mean = x64.mean(-1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = d * rstd
    g = dy64 * g64
    sg = g.mean(-1, keepdim=True)
    sgx = (g * xh).mean(-1, keepdim=True)
    dx = rstd * (g - sg - xh * sgx)
    dgamma, dbeta = (dy64 * xh).sum(0), dy64.sum(0)
    A = s * u * x64.abs().mean(-1, keepdim=True) + u * mean.abs()
    rho = (s + 8.0) * u + 2.0 * A * d.abs().mean(-1, keepdim=True) / (var + eps)
    dxh = rstd * (A + u * d.abs()) + xh.abs() * (rho + u)
    esg = s * u * g.abs().mean(-1, keepdim=True) + 2.0 * u * sg.abs()
    esgx = s * u * (g * xh).abs().mean(-1, keepdim=True) + (g.abs() * dxh).mean(-1, keepdim=True) + 2.0 * u * sgx.abs()
    inner = g.abs() + sg.abs() + (xh * sgx).abs()
    b_dx = rstd * (esg + dxh * sgx.abs() + xh.abs() * esgx + 4.0 * u * inner) + rho * rstd * inner
    adx = (dy64 * xh).abs().sum(0)
    b_dg = math.sqrt(m) * u * adx + (dy64.abs() * dxh).sum(0) + u * adx
    b_db = (math.sqrt(m) + 2.0) * u * dy64.abs().sum(0)
    return dx, b_dx, dgamma, b_dg, dbeta, b_db


def _acc_term(acc64, k, ref64):
    if acc64 is None:
        return torch.zeros_like(ref64)
    return math.sqrt(k) * ACC_EPS * acc64.to(torch.float64).cpu()


def _log(stats):
    """append the statistics of one check as a JSON line to $BF16_BOUNDS_LOG (when set): the measured ratios of a suite run in one file"""
    path = os.environ.get("BF16_BOUNDS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(stats) + "\n")


def _check(got, ref64, bound_base, acc64, k, extra, single_rounding, what, kind, rne=rne_bf16):
    got64 = got.detach().to(torch.float64).cpu()
    ref64 = ref64.detach().to(torch.float64).cpu()
    assert got64.shape == ref64.shape, (what, tuple(got64.shape), tuple(ref64.shape))
    extra = extra.to(torch.float64).cpu() if torch.is_tensor(extra) else extra
    # the store rounds the value the kernel computed, which may lie `slack` away from ref64 and then in the next binade, where half an ulp is twice as
    # large: the half ulp is taken at |ref64| + slack.  (Seen on mha_mfma_kernel<8, 256>, 125 keys, scale 1: ref 0.24989, the allowed bf16 rounding of P
    # put the fp32 result at 0.25103, stored as 0.25195 = 0.25 + 2^-9; a torch emulation of the correct kernel stores the same value.  With the half ulp
    # of ref64's own binade that was 1.04 of the bound; test_attn_bounds_cpu.py::test_store_rounding_across_a_binade_edge)
    slack = _acc_term(acc64, k, ref64) + extra
    bound = bound_base(ref64.abs() + slack) + slack
    err = (got64 - ref64).abs()
    ratio = err / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)   # NaN output: worst possible
    flat = int(torch.argmax(ratio.reshape(-1)))
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(ref64.shape))) if ref64.dim() else ()
    worst = float(ratio.reshape(-1)[flat]) if ratio.numel() else 0.0
    stats = dict(what=what, kind=kind, n=int(ref64.numel()), k=k, worst_ratio=worst)
    ok = worst <= 1.0
    if single_rounding:
        ulp = 2.0 * bound_base(ref64)
        sel = (extra <= ulp / 16) if torch.is_tensor(extra) or extra else torch.ones_like(ref64, dtype=torch.bool)
        g_s, r_s, u_s = got64[sel], ref64[sel], ulp[sel]
        n_nz = int((r_s != 0).sum())
        mism = int((g_s != rne(r_s)).sum())
        match = 1.0 - mism / max(1, r_s.numel())
        signed = ((g_s - r_s) * torch.sign(r_s) / u_s).sum().item() / max(1, n_nz)
        lim = max(MAX_MEAN_SIGNED, 1.2 / math.sqrt(max(1, n_nz)))
        stats.update(match=match, mean_signed_ulp=signed)
        ok = ok and (match >= MIN_MATCH or mism <= 1) and abs(signed) < lim
    _log(stats)
    if not ok:
        gv, rv = got64.reshape(-1)[flat].item(), ref64.reshape(-1)[flat].item()
        msg = (f"{what}: {kind} bound exceeded or biased; worst element {idx}: got {gv!r}, ref {rv!r}, |err| {abs(gv - rv):.3e}, "
               f"bound {bound.reshape(-1)[flat].item():.3e}; worst err/bound {worst:.3f}")
        if single_rounding:
            msg += f"; outputs equal to RNE(ref) {stats['match']:.4f} (>= {MIN_MATCH}); mean signed error {stats['mean_signed_ulp']:+.4f} ulp (|.| < {lim:.3f})"
        raise AssertionError(msg)
    return stats


def check_bf16(got, ref64, *, acc64=None, k=1, extra=0.0, single_rounding=True, what=""):
    """bf16 output `got` against the float64 result `ref64` of the same operation on the same bf16 operands.

    acc64: the same operation on absolute values (sum |a * b| of a GEMM, |bias|, |residual| ...), float64; k: the reduction length;
    extra: an allowance (scalar or per element) for an approximation the kernel documents; single_rounding: the kernel rounds once, where the
    reference does not round at all -- also require RNE agreement and no signed bias.  Returns the statistics (also logged, see `_log`)."""
    return _check(got, ref64, half_ulp_bf16, acc64, k, extra, single_rounding, what, "bf16")


def check_f32(got, ref64, *, acc64=None, k=1, extra=0.0, single_rounding=False, what=""):
    """fp32 output (of bf16 or fp32 operands): bound = fp32 half-ulp + the same accumulation term + extra.

    single_rounding: the kernel computes the element with exactly ONE fp32 rounding (one multiply, one FMA, or a sum of two values one of which
    is exact in the other's ulp), so it must equal RNE-to-fp32 of the float64 result almost everywhere, with no signed bias.  hipcc contracts
    `a * b + c` into an FMA by default; each call site says why one rounding holds."""
    return _check(got, ref64, half_ulp_f32, acc64, k, extra, single_rounding, what, "f32", rne=rne_f32)


def check_exact(got, want, *, what=""):
    """kernels that only move data (transposes, packing, gathers, zero padding): every element equal to `want` bit for bit -- the bit patterns
    are compared in `got`'s dtype, so -0.0 differs from +0.0 and a NaN never matches.  `want` may be wider (float64) but must hold values of
    `got`'s dtype exactly.  Logged with kind "exact"; the failure message names the first differing element in the format of the other checks."""
    g = got.detach().cpu().contiguous()
    w = want.detach().cpu()
    assert g.shape == w.shape, (what, tuple(g.shape), tuple(w.shape))
    wn = w.to(g.dtype).contiguous()
    assert torch.equal(wn.to(torch.float64).isnan(), w.to(torch.float64).isnan()) and \
        bool(((wn.to(torch.float64) == w.to(torch.float64)) | w.to(torch.float64).isnan()).all()), (what, "want is not representable in", g.dtype)
    ibits = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[g.element_size()]
    bad = (g.view(ibits) != wn.view(ibits)) | g.to(torch.float64).isnan()
    nbad = int(bad.sum())
    _log(dict(what=what, kind="exact", n=int(w.numel()), mismatches=nbad))
    if nbad:
        flat = int(torch.nonzero(bad.reshape(-1))[0])
        idx = tuple(int(i) for i in np.unravel_index(flat, tuple(w.shape))) if w.dim() else ()
        gv, wv = g.reshape(-1)[flat].item(), wn.reshape(-1)[flat].item()
        raise AssertionError(f"{what}: exact copy differs at {nbad} element(s); first differing element {idx}: got {gv!r}, want {wv!r}")
