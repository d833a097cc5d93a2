"""GPU: randomised shapes through `mt4_conv_nhwc` (fixed seed): every tile instantiation, FAST and generic staging, strides, dilations,
paddings, ragged M / N, residual, activations, fp32 (exact MFMA chain, tight tolerance) and bf16, against torch's CPU conv2d.

bf16 also element by element against float64 (`bf16_bounds`): the kernel starts its fp32 accumulators at the fp32 bias
(igemm_conv.hip:146-157), adds the bf16 residual and applies ReLU / GELU in fp32, and rounds once when it stores (`pack_bf16x2` of the staged
epilogue, `f32_to_bf16` of the direct one, igemm_conv.hip:539-616); the reference rounds nowhere after the operands.

`test_conv_random_options` adds cases from a second generator (the 70 above stay as they were): every generic tile id, K-split ids included where
the geometry is on the LDS-DMA path; bf16 operands with fp32 output and a bf16 or fp32 residual; `act="relu_gate"`; the result written into a
column slice of a wider buffer, through a per-image row permutation, or scattered into a larger image the way a strided convolution's data
gradient is (`spatial_cnn_train._dgrad`).  Every output is checked with `check_bf16` / `check_f32`, everything the launch must not touch bit for
bit, and `mt4_conv_plan` is asked about every descriptor before `mt4_conv_nhwc` gets it."""
import ctypes

import conv_tiles as ct
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from bf16_bounds import GELU_APPROX_ERR, GELU_MAX_SLOPE, check_bf16, check_f32

pytestmark = pytest.mark.gpu


def _case(rng):
    k = int(rng.choice([1, 1, 3, 3, 5]))
    kw = int(rng.choice([k, 1, 3])) if k > 1 else 1
    cin = int(rng.choice([8, 16, 24, 64, 72, 128, 256]))
    cout = int(rng.choice([8, 32, 48, 64, 96, 131, 256, 320]))
    b = int(rng.integers(1, 4))
    h, w = int(rng.integers(max(k, 3), 20)), int(rng.integers(max(kw, 3), 24))
    sh, sw = int(rng.choice([1, 1, 2])), int(rng.choice([1, 1, 2]))
    dh, dw = int(rng.choice([1, 1, 2])), int(rng.choice([1, 1, 3]))
    ph, pw = int(rng.integers(0, k // 2 * dh + 2)), int(rng.integers(0, kw // 2 * dw + 2))
    if (h + 2 * ph - dh * (k - 1) - 1) < 0 or (w + 2 * pw - dw * (kw - 1) - 1) < 0:
        ph, pw = dh * (k - 1), dw * (kw - 1)
    return dict(b=b, h=h, w=w, cin=cin, cout=cout, kh=k, kw=kw, s=(sh, sw), p=(ph, pw), d=(dh, dw),
                tile=int(rng.integers(0, 21)), res=bool(rng.integers(0, 2)), act=str(rng.choice(["none", "relu", "gelu"])))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_random_shapes(cuda, dtype):
    from computervision_codes_amd import ops
    rng = np.random.default_rng(20260101 if dtype == torch.float32 else 20260102)
    worst = 0.0
    for it in range(70):
        c = _case(rng)
        x = torch.from_numpy(rng.standard_normal((c["b"], c["cin"], c["h"], c["w"])).astype(np.float32))
        wt = torch.from_numpy((rng.standard_normal((c["cout"], c["cin"], c["kh"], c["kw"])) / np.sqrt(c["cin"] * c["kh"] * c["kw"])).astype(np.float32))
        bias = torch.from_numpy(rng.standard_normal(c["cout"]).astype(np.float32))
        if dtype == torch.bfloat16:
            x, wt = x.to(dtype).float(), wt.to(dtype).float()
        ref = F.conv2d(x, wt, bias, c["s"], c["p"], c["d"])
        res = torch.from_numpy(rng.standard_normal(tuple(ref.shape)).astype(np.float32)) if c["res"] else None
        if res is not None:
            if dtype == torch.bfloat16:
                res = res.to(dtype).float()
            ref = ref + res
        ref = {"none": lambda t: t, "relu": F.relu, "gelu": F.gelu}[c["act"]](ref)
        xd = x.permute(0, 2, 3, 1).contiguous().to(dtype).to(cuda)
        wp = ops.pack_conv_weight(wt.to(cuda), None, dtype)
        rd = res.permute(0, 2, 3, 1).contiguous().to(dtype).to(cuda) if res is not None else None
        y = ops.conv_nhwc(xd, wp, bias.to(cuda), kh=c["kh"], kw=c["kw"], stride=c["s"], pad=c["p"], dil=c["d"], residual=rd, act=c["act"],
                          tile=c["tile"])
        got = y.float().cpu().permute(0, 3, 1, 2)
        scale = max(1.0, ref.abs().max().item())
        err = (got - ref).abs().max().item() / scale
        worst = max(worst, err)
        assert err < (2e-5 if dtype == torch.float32 else 1.2e-2), (it, c, err)
        if dtype == torch.bfloat16:
            act64 = {"none": lambda t: t, "relu": F.relu, "gelu": F.gelu}[c["act"]]
            pre64 = F.conv2d(x.double(), wt.double(), bias.double(), c["s"], c["p"], c["d"])
            acc64 = F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), c["s"], c["p"], c["d"])
            if res is not None:
                pre64, acc64 = pre64 + res.double(), acc64 + res.double().abs()
            gelu = c["act"] == "gelu"
            check_bf16(got, act64(pre64), acc64=acc64 * (GELU_MAX_SLOPE if gelu else 1.0), k=c["cin"] * c["kh"] * c["kw"] + 1,
                       extra=GELU_APPROX_ERR if gelu else 0.0, what=f"conv fuzz {it} {c}")


SEEDS2 = {"f32": 20260201, "bf16": 20260202}      # the second generator: options and tiles the cases above do not draw
N_EXTRA = 60
_ACT_CODE = {"none": 0, "relu": 1, "gelu": 2, "relu_gate": 3}


def case_descriptor(c, **ptr):
    """the descriptor `ops.conv_nhwc` builds for case `c` (pointers: small aligned stand-ins unless given)"""
    rows_per_image = c["rows"] if c["layout"] == "dgrad" else 0
    return ct.descriptor(c["b"], c["h"], c["w"], c["cin"], c["cout"], c["kh"], c["kw"], c["dt"], tile=c["tile"], stride=c["s"], pad=c["p"], dil=c["d"],
                         od=c["od"], out_hw=(c["ho"], c["wo"]), act=_ACT_CODE[c["act"]], residual=ptr.get("residual", ct.FAKE_PTR if c["res"] else None),
                         residual_float=int(c["res_dt"] == "f32" and c["dt"] == "bf16"), out_row_map=ptr.get("out_row_map", ct.FAKE_PTR if c["layout"] in ("perm", "dgrad") else None),
                         out_row_map_len=c["ho"] * c["wo"] if c["layout"] in ("perm", "dgrad") else 0, out_rows_per_image=rows_per_image,
                         y_ld=c["y_ld"], res_ld=c["res_ld"], **{k: v for k, v in ptr.items() if k in ("x", "w", "y", "bias")})


def predicted_refusal(c):
    """the documented rules under which `mt4_conv_nhwc` refuses a case of `_case2`: a K-split tile off the LDS-DMA path (never drawn: `_case2` asks
    the planner for `fast` first).  Everything else it draws is inside the contract of include/mt4hip.h."""
    return c["tile"] in ct.KSPLIT_TILES and not ct.fast_rule(c["cin"], 4 if c["dt"] == "f32" else 2, c["kh"], c["kw"])


def _case2(rng, dt):
    """`_case` plus the options it does not draw.  dt: "f32" / "bf16" operands"""
    c = _case(rng)
    c.update(dt=dt, ho=ct.out_size(c["h"], c["kh"], c["s"][0], c["p"][0], c["d"][0]), wo=ct.out_size(c["w"], c["kw"], c["s"][1], c["p"][1], c["d"][1]))
    c["od"] = "f32" if dt == "f32" or int(rng.integers(0, 5)) < 2 else "bf16"
    c["act"] = str(rng.choice(["none", "relu", "gelu", "relu_gate"]))
    c["res"] = c["res"] or c["act"] == "relu_gate"          # the gate IS the residual operand
    c["res_dt"] = None if not c["res"] else "f32" if (dt == "bf16" and c["od"] == "f32" and int(rng.integers(0, 2))) else dt
    c["layout"] = str(rng.choice(["dense", "slice", "perm", "dgrad"]))
    c["rows"] = c["ho"] * c["wo"] * (4 if c["layout"] == "dgrad" else 1)         # rows per image of the buffer the launch writes
    c["phase"] = (int(rng.integers(0, 2)), int(rng.integers(0, 2)))
    c["map_seed"] = int(rng.integers(0, 2 ** 31))
    c["y_off"] = c["y_ld"] = c["res_off"] = c["res_ld"] = 0
    if c["layout"] == "slice":      # offsets and pitches in multiples of 8 elements: 16-byte aligned rows for 2- and 4-byte elements
        c["y_off"] = 8 * int(rng.integers(0, 3))
        c["y_ld"] = c["cout"] + c["y_off"] + 8 * int(rng.integers(0 if c["y_off"] else 1, 3))
        if c["res"]:
            c["res_off"] = 8 * int(rng.integers(0, 3))
            c["res_ld"] = c["cout"] + c["res_off"] + 8 * int(rng.integers(0, 3))
    c["tile"] = 0
    fast = ct.plan(case_descriptor(c))[3] == 1
    c["tile"] = int(rng.choice([0] + ct.SEQ_TILES + (ct.KSPLIT_TILES if fast else [])))
    return c


def _row_map(c):
    """output row (within an image of c["rows"] rows) of each of the Ho x Wo results"""
    n = c["ho"] * c["wo"]
    if c["layout"] == "perm":
        return np.random.default_rng(c["map_seed"]).permutation(n).astype(np.int32)
    if c["layout"] == "dgrad":      # sub-pixel phase (ph, pw) of a 2 Ho x 2 Wo image
        a, b = np.meshgrid(np.arange(c["ho"]), np.arange(c["wo"]), indexing="ij")
        return ((2 * a + c["phase"][0]) * (2 * c["wo"]) + 2 * b + c["phase"][1]).reshape(-1).astype(np.int32)
    return np.arange(n, dtype=np.int32)


class _PlanFirst:
    """stands in for `ops.lib`: `mt4_conv_plan` sees every descriptor before `mt4_conv_nhwc` does; both answers are kept"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def mt4_conv_nhwc(self, dref, stream):
        d = dref._obj
        planned = ct.plan(d)
        ints = {f: getattr(d, f) for f, t in d._fields_ if t is ctypes.c_int32}
        rc = self._lib.mt4_conv_nhwc(dref, stream)
        self.calls.append((planned, rc, ints))
        return rc


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_conv_random_options(cuda, dt, monkeypatch):
    from computervision_codes_amd import ops
    proxy = _PlanFirst(ops.lib)
    monkeypatch.setattr(ops, "lib", proxy)
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}
    rng = np.random.default_rng(SEEDS2[dt])            # the cases: the stream test_conv_plan_cpu.py counts refusals on
    drng = np.random.default_rng(SEEDS2[dt] + 1000)    # their data
    seen_tiles, seen = set(), set()
    for it in range(N_EXTRA):
        c = _case2(rng, dt)
        od, B, C, L, R = tdt[c["od"]], c["b"], c["cout"], c["ho"] * c["wo"], c["rows"]
        x = torch.from_numpy(drng.standard_normal((B, c["cin"], c["h"], c["w"])).astype(np.float32)).to(dtype).float()
        wt = torch.from_numpy((drng.standard_normal((C, c["cin"], c["kh"], c["kw"])) / np.sqrt(c["cin"] * c["kh"] * c["kw"])).astype(np.float32)).to(dtype).float()
        bias = torch.from_numpy(drng.standard_normal(C).astype(np.float32))
        geo = (c["s"], c["p"], c["d"])
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, L, C)
        pre64 = rows(F.conv2d(x.double(), wt.double(), bias.double(), *geo))
        acc64 = rows(F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), *geo))
        assert pre64.shape == (B, L, C)
        rmap = torch.from_numpy(_row_map(c)).long()
        res = None
        if c["res"]:      # lives in the OUTPUT row space; rounded to its storage type, so the stored values are exact operands
            res = torch.from_numpy(drng.standard_normal((B, R, C)).astype(np.float32)).to(tdt[c["res_dt"]])
            rv = res.double()[:, rmap]
            if c["act"] == "relu_gate":
                pre64, acc64 = torch.where(rv > 0, pre64, torch.zeros_like(pre64)), torch.where(rv > 0, acc64, torch.zeros_like(acc64))
            else:
                pre64, acc64 = pre64 + rv, acc64 + rv.abs()
        ref64 = {"none": lambda t: t, "relu": F.relu, "gelu": F.gelu, "relu_gate": lambda t: t}[c["act"]](pre64)
        # device side: y (and the residual) possibly a column slice of a wider buffer, prefilled so that anything the launch must not touch shows
        y_ld, y_off = c["y_ld"] or C, c["y_off"]
        wide = torch.from_numpy(drng.standard_normal((B * R, y_ld)).astype(np.float32)).to(od).to(cuda)
        before = wide.clone()
        out = wide[:, y_off:y_off + C] if c["y_ld"] else wide.view(B, c["ho"], c["wo"], C) if R == L else wide
        rd = None
        if res is not None:
            r_ld, r_off = c["res_ld"] or C, c["res_off"]
            rwide = torch.zeros((B * R, r_ld), dtype=res.dtype)
            rwide[:, r_off:r_off + C] = res.reshape(B * R, C)
            rwide = rwide.to(cuda)
            rd = rwide[:, r_off:r_off + C] if c["res_ld"] else rwide
        xd = x.permute(0, 2, 3, 1).contiguous().to(dtype).to(cuda)
        wp = ops.pack_conv_weight(wt.to(cuda), None, dtype)
        mapped = c["layout"] in ("perm", "dgrad")
        ops.conv_nhwc(xd, wp, bias.to(cuda), kh=c["kh"], kw=c["kw"], stride=c["s"], pad=c["p"], dil=c["d"], residual=rd, act=c["act"], tile=c["tile"],
                      out_dtype=od, out=out, y_ld=c["y_ld"], res_ld=c["res_ld"], out_hw=(c["ho"], c["wo"]),
                      out_row_map=rmap.to(torch.int32).to(cuda) if mapped else None, out_rows_per_image=R if c["layout"] == "dgrad" else 0)
        torch.cuda.synchronize()
        (prc, pkind, ptile, pfast), rc, ints = proxy.calls[-1]
        want = case_descriptor(c)
        assert ints == {f: getattr(want, f) for f, t in want._fields_ if t is ctypes.c_int32}, (it, c)    # the descriptor the CPU test counted
        assert prc == rc == ct.MT4_OK and not predicted_refusal(c), (it, c, prc, rc)
        assert pkind == ct.GENERIC and (ptile == c["tile"] or c["tile"] == 0), (it, c, ptile)
        got_all = wide.cpu()
        got = got_all.view(B, R, y_ld)[:, :, y_off:y_off + C][:, rmap]
        gelu = c["act"] == "gelu"
        check = check_bf16 if c["od"] == "bf16" else check_f32
        check(got, ref64, acc64=acc64 * (GELU_MAX_SLOPE if gelu else 1.0), k=c["cin"] * c["kh"] * c["kw"] + 1,
              extra=GELU_APPROX_ERR if gelu else 0.0, what=f"conv fuzz options {it} {c} -> tile {ptile}")
        # columns beside the slice and rows the map does not name: bit for bit what they held
        expect = before.cpu().view(B, R, y_ld).clone()
        expect[:, rmap, y_off:y_off + C] = got
        ibits = torch.int16 if c["od"] == "bf16" else torch.int32
        assert torch.equal(got_all.view(ibits), expect.view(B * R, y_ld).view(ibits)), (it, c)
        seen_tiles.add(ptile)
        seen.add((c["layout"], c["act"] == "relu_gate", c["res_dt"] if dt == "bf16" and c["od"] == "f32" else None))
    assert len(proxy.calls) == N_EXTRA
    assert {l for l, _, _ in seen} == {"dense", "slice", "perm", "dgrad"} and any(g for _, g, _ in seen)
    assert seen_tiles & set(ct.KSPLIT_TILES) and len(seen_tiles) >= 20, sorted(seen_tiles)
    if dt == "bf16":
        assert {"bf16", "f32"} <= {r for _, _, r in seen}
