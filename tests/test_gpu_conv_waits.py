"""GPU: the bias forms of `igemm_conv_kernel` and the pass boundaries of its staged epilogue.

* The accumulators start at the bias (K-split tiles: group 0 only); lanes of a column tile at or beyond Cout, a Cout that is no multiple of 4
  (scalar loads) and a launch without bias each take their own path through the prologue.  A bias that is lost, doubled or read for the wrong
  channel is of order 1 here, far outside any rounding bound.
* The staged epilogue of the bf16 forms without a row map requests the residual rows of pass p + 1 before the read-back of pass p and stores
  through a range-checked descriptor.  The cases put M on and next to every pass boundary of the 256-row tiles (16-wave passes cover 16 rows of
  each 64-row wave group; the 8-wave tiles 64 rows per pass), use a Cout with a second, mostly empty column tile, and run every residual form
  -- the forms on the new path and the forms that stay on the general one -- into a sentinel-filled buffer with guard rows and guard columns.

Every element is checked against float64 (`bf16_bounds`), as `test_gpu_kernels.py::_conv_case` does."""
import functools

import pytest
import torch
import torch.nn.functional as F
from bf16_bounds import GELU_APPROX_ERR, GELU_MAX_SLOPE, check_bf16, check_f32

pytestmark = pytest.mark.gpu

TILE_BN = {1: 128, 3: 64, 13: 128, 15: 256, 17: 256, 19: 128, 35: 32}
K_STEP_BYTES = 128


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _launch(cuda, x, w, bias, dtype, tile, **kw):
    """one 1x1 launch on rows: x [M, K], w [Cout, K] (values already representable in `dtype`)"""
    from computervision_codes_amd import ops
    m, k = x.shape
    wp = ops.pack_conv_weight(w[:, :, None, None].to(cuda), None, dtype)
    return ops.conv_nhwc(x.to(cuda, dtype).view(m, 1, 1, k), wp, None if bias is None else bias.to(cuda), kh=1, kw=1, tile=tile, **kw)


# ------------------------------------------------------------------------------------------------ bias forms
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("tile", [3, 1, 15, 17, 19, 35])
def test_bias_forms(cuda, tile, dt):
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    bn, m = TILE_BN[tile], 70
    kstep = K_STEP_BYTES // (2 if dt == "bf16" else 4)
    # (has bias, Cout): no bias; a second column tile whose lanes mostly lie beyond Cout; the scalar path (Cout % 4 != 0); a ragged first tile
    forms = [(False, bn + 8), (True, bn + 8), (True, 131), (True, 40)]
    for fi, (has_bias, cout) in enumerate(forms):
        for steps in (1, 5):
            k = kstep * steps
            seed = 1000 * tile + 100 * fi + steps
            x = _rand((m, k), seed).to(dtype).float()
            w = _rand((cout, k), seed + 1, scale=(3.0 / k) ** 0.5).to(dtype).float()
            bias = _rand((cout,), seed + 2, scale=2.0) + 0.5 if has_bias else None
            y = _launch(cuda, x, w, bias, dtype, tile)
            torch.cuda.synchronize()
            ref64 = x.double() @ w.double().t()
            acc64 = x.double().abs() @ w.double().abs().t()
            if has_bias:
                ref64, acc64 = ref64 + bias.double(), acc64 + bias.double().abs()
            check = check_bf16 if dt == "bf16" else check_f32
            check(y.view(m, cout).float().cpu(), ref64, acc64=acc64, k=k + 1, what=f"bias form tile {tile} {dt} bias={has_bias} Cout={cout} K-steps={steps}")


# ------------------------------------------------------------------------------------------------ pass boundaries
PASS_M = [255, 257, 272, 273, 335, 511]
PASS_COUT, PASS_K = 264, 128
RES_FORMS = ["res", "res_ld", "res_f32", "relu_gate", "gelu", "row_map", "y_ld"]
GUARD_ROWS, SENTINEL = 5, -768.0          # (exactly representable in bf16)


@functools.lru_cache(maxsize=None)
def _pass_reference(m):
    """bf16 operands, the float64 product + bias and its absolute-value twin, one residual (bf16 values) and a row permutation: computed once per M
    and shared, unchanged, by every tile and residual form"""
    x = _rand((m, PASS_K), 7 * m).bfloat16().float()
    w = _rand((PASS_COUT, PASS_K), 7 * m + 1, scale=(3.0 / PASS_K) ** 0.5).bfloat16().float()
    bias = _rand((PASS_COUT,), 7 * m + 2, scale=2.0) + 0.5
    pre64 = x.double() @ w.double().t() + bias.double()
    acc64 = x.double().abs() @ w.double().abs().t() + bias.double().abs()
    res = _rand((m, PASS_COUT), 7 * m + 3).bfloat16().float()
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(7 * m + 4))
    return x, w, bias, pre64, acc64, res, perm


@pytest.mark.parametrize("form", RES_FORMS)
@pytest.mark.parametrize("tile", [15, 17, 13])
def test_pass_boundaries(cuda, tile, form):
    C = PASS_COUT
    for m in PASS_M:
        x, w, bias, pre64, acc64, res, perm = _pass_reference(m)
        od = torch.float32 if form == "res_f32" else torch.bfloat16
        y_ld, y_off = (C + 24, 8) if form == "y_ld" else (C, 0)
        rv = res.double()
        kw, extra, slope = {}, 0.0, 1.0
        if form == "relu_gate":       # the residual operand is the forward activation: the result passes where it was positive
            ref64, a64 = torch.where(rv > 0, pre64, torch.zeros_like(pre64)), torch.where(rv > 0, acc64, torch.zeros_like(acc64))
            kw["act"] = "relu_gate"
        elif form == "gelu":
            ref64, a64, extra, slope = F.gelu(pre64 + rv), acc64 + rv.abs(), GELU_APPROX_ERR, GELU_MAX_SLOPE
            kw["act"] = "gelu"
        else:
            ref64, a64 = F.relu(pre64 + rv), acc64 + rv.abs()
            kw["relu"] = True
        if form == "row_map":         # result and residual of pixel i live in row perm[i]
            kw["out_row_map"] = perm.to(torch.int32).to(cuda)
            rows = perm
        else:
            rows = torch.arange(m)
        if form == "res_ld":          # the residual is a column slice of a wider buffer
            rwide = _rand((m, C + 40), 7 * m + 5).bfloat16()
            rwide[:, 16:16 + C] = res.bfloat16()
            rd = rwide.to(cuda)[:, 16:16 + C]
            kw["res_ld"] = C + 40
        else:
            rdense = torch.empty((m, C), dtype=torch.float32 if form == "res_f32" else torch.bfloat16)
            rdense[rows] = res.to(rdense.dtype)
            rd = rdense.to(cuda).view(m, 1, 1, C)
        if form == "y_ld":
            kw["y_ld"] = y_ld
        outs = []
        for _ in range(3):            # a determinism check at a fixed count
            wide = torch.full((m + GUARD_ROWS, y_ld), SENTINEL, dtype=od, device=cuda)
            out = wide[:m, y_off:y_off + C] if form == "y_ld" else wide[:m].view(m, 1, 1, C)
            _launch(cuda, x, w, bias, torch.bfloat16, tile, residual=rd, out=out, out_dtype=od, **kw)
            torch.cuda.synchronize()
            outs.append(wide.cpu())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (tile, form, m)
        got_all = outs[0].float()
        got = got_all[:m, y_off:y_off + C][rows]
        check = check_f32 if form == "res_f32" else check_bf16
        check(got, ref64, acc64=a64 * slope, k=PASS_K + 1, extra=extra, what=f"pass boundary tile {tile} {form} M={m}")
        guard = torch.ones_like(got_all, dtype=torch.bool)
        guard[:m, y_off:y_off + C] = False
        assert bool((got_all[guard] == SENTINEL).all()), (tile, form, m, "a guard row or guard column was written")
