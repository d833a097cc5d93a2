"""GPU: the bf16-operand training mode of the spatial stage -- its kernels against torch fp32 on the CPU evaluated on the SAME bf16-valued
inputs (bf16 products are exact in fp32, so only the summation order and the final rounding differ), and the whole step against the fp32
fixtures of the reference step at the tolerance the operand rounding allows.

The bf16 outputs of the BatchNorm and pooling kernels are also checked element by element against float64 (`bf16_bounds`)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bf16_bounds import GELU_APPROX_ERR, GELU_MAX_SLOPE, check_bf16, check_f32
from computervision_codes_amd import shapes, synth
from conftest import load_golden

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _rand(shape, seed, scale=1.0):
    n = int(np.prod(shape))
    return torch.from_numpy(((synth.uniform01(seed, 1, n) * 2 - 1) * scale).astype(np.float32).reshape(shape))


@pytest.mark.parametrize("b,h,w,cin,cout,k,s", [(2, 16, 32, 64, 64, 3, 1), (3, 13, 21, 128, 64, 3, 1), (2, 9, 40, 64, 128, 1, 1), (2, 16, 32, 64, 64, 3, 2),
                                                (3, 14, 22, 128, 128, 3, 2), (2, 14, 30, 64, 128, 1, 2), (5, 8, 14, 256, 64, 1, 1), (1, 1, 1, 64, 64, 3, 1),
                                                (2, 9, 17, 128, 256, 1, 1), (2, 9, 17, 256, 128, 3, 1), (2, 10, 18, 128, 256, 3, 2), (2, 10, 18, 64, 256, 1, 2),
                                                (3, 9, 16, 72, 200, 1, 1), (2, 8, 16, 864, 40, 1, 1), (2, 7, 9, 24, 88, 3, 1)])
def test_wgrad_conv2d_bf16_vs_autograd(cuda, b, h, w, cin, cout, k, s):
    """`mt4_wgrad_conv2d_bf16` (bf16 MFMA, transposed LDS reads, kernel rows split over workgroups, fp32 atomics): full and ragged spatial tiles,
    both strides, 1x1 and 3x3, several channel tiles; accumulation into a non-zero buffer"""
    from computervision_codes_amd import ops
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    x = _rand((b, h, w, cin), 1).to(BF)
    dy = _rand((b, ho, wo, cout), 2).to(BF)
    wt = torch.zeros(cout, cin, k, k, requires_grad=True)
    with torch.enable_grad():
        y = F.conv2d(x.float().permute(0, 3, 1, 2), wt, None, stride=s, padding=pad)
        y.backward(dy.float().permute(0, 3, 1, 2))
    kp = ops.packed_k(cin, k, k, torch.float32)
    base = _rand((cout, kp), 3)
    dw = base.to(cuda).clone()
    ops.wgrad_conv2d_bf16(dy.to(cuda), x.to(cuda), dw, k, s)
    got = (dw.cpu() - base)[:, :k * k * cin].reshape(cout, k, k, cin).permute(0, 3, 1, 2)
    ref = wt.grad
    assert (got - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item()) + 1e-5, (got - ref).abs().max().item()
    assert float((dw.cpu() - base)[:, k * k * cin:].abs().max()) == 0.0 if kp > k * k * cin else True
    # per element against float64 of the same bf16 operands: fp32 MFMA accumulation over the b * ho * wo pixels, added to the buffer
    g64 = lambda xx, gg: torch.nn.grad.conv2d_weight(xx.permute(0, 3, 1, 2), (cout, cin, k, k), gg.permute(0, 3, 1, 2), s, pad).permute(0, 2, 3, 1).reshape(cout, -1)
    x64, dy64 = x.double(), dy.double()
    kk, b64 = k * k * cin, base[:, :k * k * cin].double()
    check_f32(dw.cpu()[:, :kk], b64 + g64(x64, dy64), acc64=b64.abs() + g64(x64.abs(), dy64.abs()), k=b * ho * wo + 1,
              what=f"wgrad_conv2d_bf16 {(b, h, w, cin, cout, k, s)}")


@pytest.mark.parametrize("m,c,relu,res,xf32", [(200, 64, True, False, False), (1031, 128, True, True, False), (77, 256, False, False, False), (300, 64, True, False, True)])
def test_batchnorm_bf16_fwd_bwd(cuda, m, c, relu, res, xf32):
    """train-mode BatchNorm with bf16 tensors (fp32 convolution output for the stem variant): statistics, output, and the three gradients against
    torch on the same bf16-valued inputs; outputs are bf16, so one rounding of tolerance.

    Per element against float64 (train2d_bf16.hip): the statistics are float64 sums, mean and invstd rounded to fp32 (:119-131);
    `bn_apply_t_kernel` stores (x - mean) * invstd * gamma + beta (+ bf16 residual, ReLU) from fp32 arithmetic with one rounding (:152-158);
    `bn_bwd_reduce_t_kernel` sums dy and dy * x_hat (x_hat in fp32) in float64, the ReLU gate read from the stored bf16 output (:176-222);
    `bn_bwd_apply_t_kernel` stores gamma invstd (dy - mean(dy) - x_hat mean(dy x_hat)) in fp32 with one rounding (:248-265), the gated dy as dres
    (exact), and dgamma / dbeta as the float64 sums rounded to fp32 (:241-242)."""
    from computervision_codes_amd import ops
    x = (_rand((m, c), 1, 2.0) + 0.3)
    x = x if xf32 else x.to(BF)
    g, bta = _rand((c,), 2) + 1.5, _rand((c,), 3)
    r = _rand((m, c), 4).to(BF) if res else None
    dy = _rand((m, c), 5).to(BF)
    rm, rv = _rand((c,), 6), _rand((c,), 7).abs() + 0.5
    xt, gt, bt = x.float().clone().requires_grad_(), g.clone().requires_grad_(), bta.clone().requires_grad_()
    rt = r.float().clone().requires_grad_() if res else None
    rm_t, rv_t = rm.clone(), rv.clone()
    with torch.enable_grad():
        y_ref = F.batch_norm(xt, rm_t, rv_t, gt, bt, training=True, momentum=0.1, eps=1e-5)
        if res:
            y_ref = y_ref + rt
        if relu:
            y_ref = torch.relu(y_ref)
    sums = torch.zeros(4 * c, dtype=torch.float64, device=cuda)
    rmd, rvd = rm.to(cuda), rv.to(cuda)
    mean, invstd = ops.bn_stats_t(x.to(cuda), rmd, rvd, sums=sums[:2 * c])
    y = ops.bn_apply_t(x.to(cuda), mean, invstd, g.to(cuda), bta.to(cuda), r.to(cuda) if res else None, relu)
    assert y.dtype == BF
    assert (rmd.cpu() - rm_t).abs().max() < 1e-5 and (rvd.cpu() - rv_t).abs().max() < 1e-5
    assert (y.float().cpu() - y_ref.detach()).abs().max().item() <= 2 ** -8 * max(1.0, y_ref.abs().max().item())
    x64, g64, b64 = x.double(), g.double(), bta.double()
    mu64 = x64.mean(0)
    is64 = 1.0 / torch.sqrt(((x64 - mu64) ** 2).mean(0) + 1e-5)
    xh64 = (x64 - mu64) * is64
    y64 = xh64 * g64 + b64
    acc_y = (x64.abs() + mu64.abs()) * is64 * g64.abs() + b64.abs()
    if res:
        y64, acc_y = y64 + r.double(), acc_y + r.double().abs()
    check_bf16(y.cpu(), torch.relu(y64) if relu else y64, acc64=acc_y, k=4, what=f"bn_apply_t {(m, c, relu, res, xf32)}")
    # backward on the bf16 output the kernel produced (the ReLU gate is read from it)
    with torch.enable_grad():
        y_ref.backward(dy.float())
    dg, db = torch.zeros(c, device=cuda), torch.zeros(c, device=cuda)
    dx, dres = ops.bn_backward_t(dy.to(cuda), y if relu else None, x.to(cuda), mean, invstd, g.to(cuda), dg, db, relu=relu, want_dres=res, sums=sums[2 * c:])
    assert dx.dtype == x.dtype
    dy64 = dy.double() * (y.cpu() > 0).double() if relu else dy.double()        # the kernel's gate: its own stored output
    m1, m2 = dy64.mean(0), (dy64 * xh64).mean(0)
    dx64 = g64 * is64 * (dy64 - m1 - xh64 * m2)
    acc_dx = g64.abs() * is64 * (dy64.abs() + m1.abs() + (xh64.abs() + (x64.abs() + mu64.abs()) * is64) * (m2.abs() + (dy64 * xh64).abs().mean(0)))
    if xf32:
        check_f32(dx.cpu(), dx64, acc64=acc_dx, k=8, what=f"bn_backward_t dx fp32 {(m, c, relu, res)}")
    else:
        check_bf16(dx.cpu(), dx64, acc64=acc_dx, k=8, what=f"bn_backward_t dx {(m, c, relu, res)}")
    check_f32(db.cpu(), dy64.sum(0), acc64=dy64.abs().sum(0), k=m, what=f"bn_backward_t dbeta {(m, c)}")
    check_f32(dg.cpu(), (dy64 * xh64).sum(0), acc64=(dy64 * xh64).abs().sum(0), k=m, what=f"bn_backward_t dgamma {(m, c)}")
    if res:
        check_bf16(dres.cpu(), dy64, what=f"bn_backward_t dres {(m, c, relu)}")
    tol = 2 ** -8 if not xf32 else 1e-4
    assert (dx.float().cpu() - xt.grad).abs().max().item() <= tol * max(1.0, xt.grad.abs().max().item())
    assert (dg.cpu() - gt.grad).abs().max().item() <= 2e-3 * max(1.0, gt.grad.abs().max().item())
    assert (db.cpu() - bt.grad).abs().max().item() <= 2e-3 * max(1.0, bt.grad.abs().max().item())
    if res:
        assert (dres.float().cpu() - rt.grad).abs().max().item() <= 2 ** -8 * max(1.0, rt.grad.abs().max().item())
    if relu and not res:   # the gate recomputed from x == the gate read from the stored output
        dg2, db2 = torch.zeros(c, device=cuda), torch.zeros(c, device=cuda)
        sums2 = torch.zeros(2 * c, dtype=torch.float64, device=cuda)
        dx2, _ = ops.bn_backward_t(dy.to(cuda), None, x.to(cuda), mean, invstd, g.to(cuda), dg2, db2, relu=True, sums=sums2, beta=bta.to(cuda))
        assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)


@pytest.mark.parametrize("b,h,w,cin,cout,k,s,dt,tile", [
    (2, 24, 40, 64, 64, 1, 1, "bf16", 0), (2, 24, 40, 64, 256, 1, 1, "bf16", 0), (3, 13, 21, 128, 128, 3, 1, "bf16", 0), (8, 64, 112, 64, 64, 3, 1, "bf16", 0),
    (2, 30, 52, 256, 512, 1, 2, "bf16", 0), (2, 24, 40, 64, 64, 1, 1, "bf16", 17), (2, 24, 40, 64, 128, 1, 1, "bf16", 5), (1, 40, 72, 4, 64, 7, 2, "f32", 0),
    (2, 24, 40, 64, 256, 1, 1, "f32", 0), (3, 13, 21, 128, 128, 3, 1, "f32", 0),
    (2, 16, 20, 64, 72, 1, 1, "bf16", 0)])
def test_conv_epilogue_statistics(cuda, b, h, w, cin, cout, k, s, dt, tile):
    """`mt4_conv_desc.stat_sums`: the replicas add up to the float64 column sums / sums of squares of the map the launch stored (generic tiles,
    the 3x3 patch kernel where it runs, the fp32 stem geometry, ragged last tiles and channel tiles), and `mt4_bn_apply_sums_t` equals
    `mt4_bn_stats_t` + `mt4_bn_apply_t` on the stored map bit for bit"""
    from computervision_codes_amd import ops
    tdt = BF if dt == "bf16" else torch.float32
    pad = k // 2
    x = _rand((b, h, w, cin), 1).to(tdt).to(cuda)
    wt = _rand((cout, cin, k, k), 2, 0.2).to(cuda)
    wp = ops.pack_conv_weight(wt, None, tdt)
    sums = torch.zeros((ops.STAT_REPLICAS, 2, cout), dtype=torch.float64, device=cuda)
    y = ops.conv_nhwc(x, wp, None, kh=k, kw=k, stride=(s, s), pad=(pad, pad), stat_sums=sums, tile=tile)
    y0 = ops.conv_nhwc(x, wp, None, kh=k, kw=k, stride=(s, s), pad=(pad, pad), tile=tile)
    assert torch.equal(y, y0)
    m = y.numel() // cout
    yd = y.view(m, cout).double()
    tot = sums.sum(0)
    assert (tot[0] - yd.sum(0)).abs().max().item() <= 1e-12 * m * yd.abs().max().item()
    assert (tot[1] - (yd * yd).sum(0)).abs().max().item() <= 1e-12 * m * yd.abs().max().item() ** 2
    g, bt = _rand((cout,), 3).to(cuda) + 1.5, _rand((cout,), 4).to(cuda)
    res = _rand((m, cout), 5).to(BF).to(cuda)
    rm, rv = torch.zeros(cout, device=cuda), torch.ones(cout, device=cuda)
    rm0, rv0 = rm.clone(), rv.clone()
    a, mean, invstd = ops.bn_apply_sums_t(y.view(m, cout), sums, g, bt, res, True, rm, rv)
    mean0, invstd0 = ops.bn_stats_t(y.view(m, cout), rm0, rv0, sums=torch.zeros(2 * cout, dtype=torch.float64, device=cuda))
    a0 = ops.bn_apply_t(y.view(m, cout), mean0, invstd0, g, bt, res, True)
    assert torch.equal(mean, mean0) and torch.equal(invstd, invstd0) and torch.equal(rm, rm0) and torch.equal(rv, rv0) and torch.equal(a, a0)
    if dt == "f32":   # the fp32 twin: fp32 residual and activation
        r32 = res.float()
        rm1, rv1, rm2, rv2 = torch.zeros(cout, device=cuda), torch.ones(cout, device=cuda), torch.zeros(cout, device=cuda), torch.ones(cout, device=cuda)
        a1, mean1, invstd1 = ops.bn_apply_sums(y.view(m, cout), sums, g, bt, r32, True, rm1, rv1)
        mean2, invstd2 = ops.bn_stats(y.view(m, cout), rm2, rv2)
        a2 = ops.bn_apply(y.view(m, cout), mean2, invstd2, g, bt, r32, True)
        assert torch.equal(mean1, mean2) and torch.equal(invstd1, invstd2) and torch.equal(rm1, rm2) and torch.equal(rv1, rv2) and torch.equal(a1, a2)


def test_conv_epilogue_statistics_refusals(cuda):
    from computervision_codes_amd import _lib, ops
    x = _rand((2, 16, 16, 64), 1).to(BF).to(cuda)
    wp = ops.pack_conv_weight(_rand((64, 64, 1, 1), 2).to(cuda), None, BF)
    sums = torch.zeros((ops.STAT_REPLICAS, 2, 64), dtype=torch.float64, device=cuda)
    for tile in (-1, 40):                                           # K-split tiles keep no channel sums
        with pytest.raises(_lib.Mt4Error):
            ops.conv_nhwc(x, wp, None, kh=1, kw=1, stat_sums=sums, tile=tile)
    assert float(sums.abs().max()) == 0.0


def _check_maxpool_bwd(x, dy, dx):
    """`maxpool3x3s2_bwd_bf16` (both kernels, train2d_bf16.hip:443-480 and the tiled one): the fp32 sum of the (up to 4) window gradients a
    pixel takes, one rounding.  Reference: the same routing by float64 autograd (ties: the first maximum in scan order, as in torch)"""
    xt = x.double().permute(0, 3, 1, 2).clone().requires_grad_()
    xa = x.double().permute(0, 3, 1, 2).clone().requires_grad_()
    with torch.enable_grad():
        F.max_pool2d(xt, 3, 2, 1).backward(dy.double().permute(0, 3, 1, 2))
        F.max_pool2d(xa, 3, 2, 1).backward(dy.double().abs().permute(0, 3, 1, 2))
    check_bf16(dx.cpu(), xt.grad.permute(0, 2, 3, 1), acc64=xa.grad.permute(0, 2, 3, 1), k=4, what=f"maxpool3x3s2_bwd_bf16 {tuple(x.shape)}")


@pytest.mark.parametrize("b,h,w,c", [(2, 13, 18, 64), (1, 40, 37, 128), (2, 13, 18, 8), (1, 32, 48, 64)])
def test_maxpool_backward_bf16(cuda, b, h, w, c):
    """C % 64 == 0 runs the LDS-tiled kernel (several 16 x 16 tiles, ragged edges), other channel counts the per-pixel one"""
    from computervision_codes_amd import ops
    x = _rand((b, h, w, c), 1).to(BF)
    x[0, 2:5, 2:5, :8] = 1.5                                        # ties: the first maximum in scan order takes the gradient
    x[0, 14:19, 14:19, :] = -0.25                                   # ties across a tile boundary
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = _rand((b, ho, wo, c), 2).to(BF)
    xt = x.float().permute(0, 3, 1, 2).clone().requires_grad_()
    with torch.enable_grad():
        F.max_pool2d(xt, 3, 2, 1).backward(dy.float().permute(0, 3, 1, 2))
    dx = ops.maxpool3x3s2_bwd_bf16(x.to(cuda), dy.to(cuda))
    ref = xt.grad.permute(0, 2, 3, 1)
    assert (dx.float().cpu() - ref).abs().max().item() <= 2 ** -7 * max(1.0, ref.abs().max().item())
    _check_maxpool_bwd(x, dy, dx)


def test_pool_backward_and_repack_bf16(cuda):
    from computervision_codes_amd import ops
    b, h, w, c = 2, 13, 18, 64
    x = _rand((b, h, w, c), 1).to(BF)
    x[0, 2:5, 2:5, :8] = 1.5                                        # ties: the first maximum in scan order takes the gradient
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = _rand((b, ho, wo, c), 2).to(BF)
    xt = x.float().permute(0, 3, 1, 2).clone().requires_grad_()
    with torch.enable_grad():
        F.max_pool2d(xt, 3, 2, 1).backward(dy.float().permute(0, 3, 1, 2))
    dx = ops.maxpool3x3s2_bwd_bf16(x.to(cuda), dy.to(cuda))
    ref = xt.grad.permute(0, 2, 3, 1)
    assert (dx.float().cpu() - ref).abs().max().item() <= 2 ** -7 * max(1.0, ref.abs().max().item())
    _check_maxpool_bwd(x, dy, dx)
    df = _rand((3, 128), 3)
    dxa = ops.avgpool_bwd_bf16(df.to(cuda), 3, 21, 128)
    assert (dxa.float().cpu() - (df / 21)[:, None, :].expand(3, 21, 128)).abs().max().item() <= 2 ** -8 * float(df.abs().max()) / 21
    # fp32 df * fp32(1 / 21), one rounding (train2d_bf16.hip:485-494)
    ref64 = (df.double() / 21)[:, None, :].expand(3, 21, 128)
    check_bf16(dxa.cpu(), ref64, acc64=ref64.abs(), k=2, what="avgpool_bwd_bf16")
    # packed fp32 -> packed bf16 == packing the bf16-rounded weights directly
    wt = _rand((128, 64, 3, 3), 4).to(cuda)
    w32 = ops.pack_conv_weight(wt, None, torch.float32)
    assert torch.equal(ops.repack_weight_bf16(w32, 128, 64, 3, 3), ops.pack_conv_weight(wt, None, BF))
    w1 = _rand((64, 256, 1, 1), 5).to(cuda)
    assert torch.equal(ops.repack_weight_bf16(ops.pack_conv_weight(w1, None, torch.float32), 64, 256, 1, 1), ops.pack_conv_weight(w1, None, BF))


def _inputs(cfg):
    img = synth.normalize_frames(synth.synthetic_frames(cfg["B"], cfg["H"], cfg["W"], seed=cfg["seed"]))
    labels = [torch.from_numpy((synth.uniform01(cfg["seed"], 700 + i, cfg["B"] * k) < 0.15).reshape(cfg["B"], k).astype(np.int64))
              for i, k in enumerate((6, 10, 15, 100))]
    tpred = [synth.synthetic_features(cfg["B"], k, seed=cfg["seed"] + 10 + i)[0] * 2.0 for i, k in enumerate((6, 10, 15))]
    tfeat = [synth.synthetic_features(cfg["B"], 1536, seed=cfg["seed"] + 20 + i)[0] for i in range(3)]
    return img, labels, tpred, tfeat


@pytest.mark.parametrize("name", ["cnn_train_resnet18", "cnn_train_resnet50"])
def test_bf16_operand_step_vs_reference_fixture(cuda, name):
    """the bf16-operand step against the fp32 fixtures captured from the reference module + torch autograd.  DECLARED tolerance of the mode (bf16
    operands carry 8 mantissa bits; sums are fp32 / fp64): every loss term within 3e-3 relative; per-parameter gradient norms within 2 % in the
    median, 8 % at the 90th percentile and 20 % at worst (norm floor 1e-6 of the largest); the SGD step moves the parameters in the fixture's
    direction (cosine > 0.9 on the sampled deltas of the large tensors; the stem, at the far end of the backward chain, is the noisiest at 0.92)"""
    from computervision_codes_amd.spatial_cnn_train import SpatialCnnTrainer
    from oracle.spatial_cnn_train import damp_residual_gamma
    z, cfg = load_golden(name)
    table = shapes.spatial_cnn_shapes(cfg["network"])
    sd = damp_residual_gamma(synth.fill_from_shapes(table, seed=cfg["seed"]), cfg["network"], cfg.get("damp", 1.0))
    img, labels, tpred, tfeat = _inputs(cfg)
    tr = SpatialCnnTrainer(cfg["network"], lr=cfg["lr"], weight_decay=1e-5, rates=cfg["rates"], temp=4.0, operand_dtype=BF).load_state_dict(sd)
    terms = tr.train_step(img.to(cuda), labels, tpred, tfeat, apply_update=False)
    for k in ("loss", "hard", "soft", "kd"):
        assert abs(terms[k] - float(z[k])) <= 3e-3 * max(1.0, abs(float(z[k]))), (k, terms[k], float(z[k]))
    g = tr.grads()
    ref = z["grad_norms"]
    rel = np.array([abs(float(g[k].norm()) - r) / max(r, 1e-6 * ref.max()) for (k, _), r in zip(table, ref) if r > 0 and k in g])
    assert np.median(rel) < 2e-2 and np.percentile(rel, 90) < 8e-2 and rel.max() < 0.2, (np.median(rel), np.percentile(rel, 90), rel.max())
    tr.apply_update()
    new = tr.state_dict()
    for key in z.files:
        if key.startswith("delta::") and "running" not in key:
            k = key[len("delta::"):]
            flat = (new[k].float() - sd[k].float()).flatten()
            got, want = flat[:: max(1, flat.numel() // 2048)], torch.from_numpy(z[key])
            if want.numel() >= 512:
                cos = float((got * want).sum() / (got.norm() * want.norm() + 1e-30))
                assert cos > 0.9, (k, cos)


def test_epilogue_statistics_step_equals_separate_pass(cuda, monkeypatch):
    """the forward of a bf16 step with BatchNorm statistics taken in the convolution epilogue (default) and with the separate statistics pass
    (`epilogue_stats=False`) agree bit for bit: every unit's activations, the advanced running statistics, the BCE term (the KL / MSE terms are
    summed with fp32 atomics and agree to their run-to-run noise)"""
    from computervision_codes_amd.spatial_cnn_train import SpatialCnnTrainer
    from oracle.spatial_cnn_train import damp_residual_gamma
    z, cfg = load_golden("cnn_train_resnet50")
    table = shapes.spatial_cnn_shapes(cfg["network"])
    sd = damp_residual_gamma(synth.fill_from_shapes(table, seed=cfg["seed"]), cfg["network"], cfg.get("damp", 1.0))
    img, labels, tpred, tfeat = _inputs(cfg)
    res = []
    for off in (False, True):
        tr = SpatialCnnTrainer(cfg["network"], lr=cfg["lr"], weight_decay=1e-5, rates=cfg["rates"], temp=4.0, operand_dtype=BF,
                               epilogue_stats=not off).load_state_dict(sd)
        assert tr.epilogue_stats == (not off)
        terms = tr.train_step(img.to(cuda), labels, tpred, tfeat, apply_update=False)
        res.append((terms, [rec[5].clone() for rec in tr.last_saved], {n: (u.rmean.clone(), u.rvar.clone()) for n, u in tr.units.items()}))
    (t0, a0, r0), (t1, a1, r1) = res
    assert all(torch.equal(x, y) for x, y in zip(a0, a1))
    assert t0["hard"] == t1["hard"]
    assert all(abs(t0[k] - t1[k]) <= 1e-6 * abs(t0[k]) for k in ("loss", "soft", "kd")), (t0, t1)   # (their reductions add with fp32 atomics)
    assert all(torch.equal(r0[n][0], r1[n][0]) and torch.equal(r0[n][1], r1[n][1]) for n in r0)


def test_bf16_operand_training_tracks_fp32(cuda):
    """six SGD steps on the same batches from the same start: the bf16-operand trainer's loss follows the fp32 trainer's within 1 %, and both fall"""
    from computervision_codes_amd.spatial_cnn_train import SpatialCnnTrainer
    cfg = dict(network="resnet18", B=8, H=64, W=96, seed=911)
    table = shapes.spatial_cnn_shapes("resnet18")
    sd = synth.fill_from_shapes(table, seed=cfg["seed"])
    img, labels, tpred, tfeat = _inputs(cfg)
    curves = []
    for dt in (torch.float32, BF):
        tr = SpatialCnnTrainer("resnet18", lr=0.01, weight_decay=1e-5, rates=(1.0, 1.0, 1.0), temp=4.0, operand_dtype=dt).load_state_dict(sd)
        curves.append([tr.train_step(img.to(cuda), labels, tpred, tfeat)["loss"] for _ in range(6)])
    f32, b16 = curves
    assert all(abs(a - b) <= 1e-2 * abs(a) for a, b in zip(f32, b16)), (f32, b16)
    assert f32[-1] < f32[0] and b16[-1] < b16[0]
    # hipGraph replay of the bf16 step == eager launches
    tr_e = SpatialCnnTrainer("resnet18", lr=0.01, operand_dtype=BF).load_state_dict(sd)
    tr_g = SpatialCnnTrainer("resnet18", lr=0.01, operand_dtype=BF).load_state_dict(sd)
    le = [tr_e.train_step(img.to(cuda), labels, tpred, tfeat)["loss"] for _ in range(2)]
    lg = [tr_g.train_step(img.to(cuda), labels, tpred, tfeat, use_graph=True)["loss"] for _ in range(2)]
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(le, lg)), (le, lg)


@pytest.mark.parametrize("m,k,n,act", [(300, 256, 128, None), (77, 64, 40, "relu"), (513, 384, 864, "gelu"), (200, 128, 64, "relu_gate")])
def test_mixed_precision_linear_fp32_residual(cuda, m, k, n, act):
    """the mixed-precision training GEMM: bf16 operands (activation copy by `mt4_cast_f32_bf16`, packed bf16 weights), fp32 output with an fp32
    residual / ReLU gate (`mt4_conv_desc.residual_float`) -- against fp32 torch on the bf16-valued operands"""
    from computervision_codes_amd import ops
    x, w, b, r = _rand((m, k), 1), _rand((n, k), 2, k ** -0.5), _rand((n,), 3), _rand((m, n), 4)
    xd = ops.cast_bf16(x.to(cuda))
    assert torch.equal(xd.cpu(), x.to(BF))
    wp = ops.pack_linear_weight(w.to(cuda), BF)
    y = ops.linear(xd, wp, b.to(cuda) if act != "relu_gate" else None, act=act, residual=r.to(cuda), out_dtype=torch.float32)
    assert y.dtype == torch.float32
    pre = x.to(BF).float() @ w.to(BF).float().t()
    if act == "relu_gate":
        ref = torch.where(r > 0, pre, torch.zeros_like(pre))
    else:
        ref = pre + b + r
        ref = torch.relu(ref) if act == "relu" else (F.gelu(ref) if act == "gelu" else ref)
    assert (y.cpu() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item()) + 1e-6 * (act == "gelu")
    # fp32 output: the accumulators start at the bias, the fp32 residual / gate and the activation are applied in fp32, nothing is rounded to bf16
    x64, w64, b64, r64 = x.to(BF).double(), w.to(BF).double(), b.double(), r.double()
    pre64, acc64 = x64 @ w64.t(), x64.abs() @ w64.abs().t()
    if act == "relu_gate":
        ref64 = torch.where(r64 > 0, pre64, torch.zeros_like(pre64))
    else:
        ref64, acc64 = pre64 + b64 + r64, acc64 + b64.abs() + r64.abs()
        ref64 = torch.relu(ref64) if act == "relu" else (F.gelu(ref64) if act == "gelu" else ref64)
    gelu = act == "gelu"
    check_f32(y.cpu(), ref64, acc64=acc64 * (GELU_MAX_SLOPE if gelu else 1.0), k=k + 2, extra=GELU_APPROX_ERR if gelu else 0.0,
              what=f"mixed-precision linear {(m, k, n, act)}")
