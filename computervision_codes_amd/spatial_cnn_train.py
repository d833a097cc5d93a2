"""One training step of the spatial student on MI355X (`Spatial_cnn/run.py:145-224`): train-mode ResNet-18/50 trunk
(BatchNorm on batch statistics), KD branch (`network.py:47-71`), hard BCE (pos_weight) + soft DistillKL + feature MSE
(`run.py:159-192,284-295,322-328`), backward and SGD (`:342-351`) as explicit HIP launches -- no autograd.  fp32, NHWC.

* conv forward / data gradient: `mt4_conv_nhwc` (data gradient = conv of dY with the transposed, tap-reversed weights;
  stride-2 3x3 convs as 4 sub-pixel phases and the stride-2 1x1 downsample as one phase, scattered through the output row
  map into dX);  weight gradient: `mt4_wgrad_conv2d_f32` / `mt4_wgrad_conv1d_f32`;
* BatchNorm: `mt4_bn_stats_f32` + `mt4_bn_apply_f32` forward, `mt4_bn_backward_f32` (ReLU gate and residual fan-out fused);
* losses: `mt4_bce_logits_pw_f32`, `mt4_distill_kl_f32`, `mt4_mse_f32`; KD mixing `mt4_kd_mix` / `mt4_kd_mix_bwd_f32`;
* one flat fp32 parameter buffer and one flat gradient buffer (packed layouts) -> ONE all-reduce per step for DDP, one
  `mt4_sgd_step_f32`.  BatchNorm statistics stay per GPU, like the reference's plain `BatchNorm2d`.
* `deterministic=True`: every sum above that crosses workgroups goes through the `_det` entry points (per-workgroup partials in one workspace, folded in
  index order; DESIGN.md, "Deterministic training") -- the same inputs give the same bits, eager or replayed.
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence

import torch

from . import ops
from .flatparams import FlatParams, FlatTrainer, _r4
from .shapes import resnet_feat_dim, spatial_cnn_shapes

_DEPTHS = {"resnet18": (2, 2, 2, 2), "resnet50": (3, 4, 6, 3)}
_ALL_HEADS = (("i", 6), ("v", 10), ("t", 15), ("ivt", 100))
# `Spatial_cnn/run.py:306-311`
TOOL_W = [0.93487068, 0.94234964, 0.93487068, 1.18448115, 1.02368339, 0.97974447]
VERB_W = [0.60002400, 0.60002400, 0.60002400, 0.61682467, 0.67082683, 0.80163207, 0.70562823, 2.11208448, 2.69230769, 0.60062402]
TARGET_W = [0.49752894, 0.52041527, 0.49752894, 0.51394739, 2.71899565, 1.75577963, 0.58509403, 1.25228034, 0.49752894, 2.42993134,
            0.49802647, 0.87266576, 1.36074165, 0.50150917, 0.49802647]
F32 = torch.float32
_POS_W = {"i": TOOL_W, "v": VERB_W, "t": TARGET_W, "ivt": [1.0] * 100}


class _Unit:
    """conv + BatchNorm (+ReLU) with its parameter / gradient views"""
    __slots__ = ("name", "bn", "cin", "cout", "k", "stride", "pad", "w", "gw", "gamma", "beta", "ggamma", "gbeta", "rmean", "rvar", "wt", "phase_w",
                 "sums_f", "sums_b", "w16", "wt16", "phase_w16")


class SpatialCnnTrainer(FlatTrainer):
    op16 = False                # (class defaults: GEMM operands fp32; no derived-weight table built yet)
    _refresh_table = None
    def __init__(self, network: str = "resnet50", lr: float = 0.01, weight_decay: float = 1e-5, rates: Sequence[float] = (1.0, 1.0, 1.0),
                 temp: float = 4.0, device: str = "cuda", process_group=None, overlap: bool = True, teacher_dim: int = 1536,
                 loss_type: str = "all", operand_dtype: torch.dtype = torch.float32, epilogue_stats: bool = True, deterministic: bool = False,
                 clip_grad_norm: float = 0.0, skip_nonfinite: bool = False, optim=None, ema=None):
        """loss_type 'all': the distillation recipe (four heads, KD branch, hard + soft + feature losses: `run.py:180-192`);
        'i' | 'v' | 't': a single-task student -- only that classifier exists (`network.py:34-41`) and the loss is its BCE alone
        (`run.py:165-179`)"""
        assert loss_type in ("all", "i", "v", "t")
        assert operand_dtype in (torch.float32, torch.bfloat16)
        # bfloat16: the convolutions' GEMM operands (activations, activation gradients, weight copies) are bf16, sums fp32 / fp64, master
        # weights + gradients + SGD fp32 (csrc/train2d_bf16.hip); the stem's 7x7x3 convolution and the heads / KD branch stay fp32
        self.op16 = operand_dtype == torch.bfloat16
        # BatchNorm statistics from the producing convolution's epilogue (False: the separate pass over the map -- same bits, tested)
        self.epilogue_stats = bool(epilogue_stats)
        # deterministic: every sum of the step that crosses workgroups -- BatchNorm statistics and backward sums, conv and linear weight / bias gradients,
        # the fp32 max-pool backward, the three losses -- comes from per-workgroup partials stored into ONE workspace and folded in index order (the
        # `_det` entry points; the max-pool backward in gather form), in both operand modes; a step is then a pure function of its inputs, eager or
        # replayed.  The statistics come from the separate pass (the convolution epilogue's sums are atomic: csrc/igemm_conv.hip is not covered).
        # Up to two ranks the all-reduce is one commutative add; beyond, the step is as reproducible as the collective.
        self.deterministic = bool(deterministic)
        if self.deterministic:
            self.epilogue_stats = False
        self._ws = self._ws64 = None
        self.loss_type = loss_type
        self.heads = _ALL_HEADS if loss_type == "all" else tuple(h for h in _ALL_HEADS if h[0] == loss_type)
        self.NH = sum(k for _, k in self.heads)
        self.NHP = (self.NH + 3) // 4 * 4
        # overlap: each gradient bucket is all-reduced as soon as the backward has written it (DDP, `FlatTrainer`)
        super().__init__(lr, weight_decay, device, process_group, overlap, clip_grad_norm, skip_nonfinite, optim, ema)
        self.network, self.rates, self.temp = network, tuple(rates), float(temp)
        self.C = resnet_feat_dim(network)
        self.TD = int(teacher_dim)          # `--teacher_dim` (`Spatial_cnn/run.py:82`): width of the teachers' frame features
        self._table = spatial_cnn_shapes(network, self.C, self.TD, loss_type)
        self.units: Dict[str, _Unit] = {}
        self.nbt: Dict[str, int] = {}
        self._extra: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ parameters
    def _unit_specs(self):
        pre = "basemodel.basemodel."
        specs = [(pre + "conv1", pre + "bn1", 4, 64, 7, 2, 0)]   # stem on the physically padded 4-channel image
        bott = self.network == "resnet50"
        cin = 64
        for li, (planes, n) in enumerate(zip((64, 128, 256, 512), _DEPTHS[self.network]), start=1):
            for b in range(n):
                s = 2 if (b == 0 and li > 1) else 1
                q = f"{pre}layer{li}.{b}."
                cout = planes * (4 if bott else 1)
                if bott:
                    specs += [(q + "conv1", q + "bn1", cin, planes, 1, 1, 0), (q + "conv2", q + "bn2", planes, planes, 3, s, 1),
                              (q + "conv3", q + "bn3", planes, cout, 1, 1, 0)]
                else:
                    specs += [(q + "conv1", q + "bn1", cin, planes, 3, s, 1), (q + "conv2", q + "bn2", planes, planes, 3, 1, 1)]
                if b == 0 and (s != 1 or cin != cout):
                    specs.append((q + "downsample.0", q + "downsample.1", cin, cout, 1, s, 0))
                cin = cout
        return specs

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        assert all(k in sd for k, _ in self._table), "state dict incomplete"
        dev, C, TD = self.dev, self.C, self.TD
        specs = self._unit_specs()
        # gradient buckets: "stem", "layer1".."layer4", "heads" (heads + KD branch); a unit is its conv weight, BN gamma, BN beta
        fp = FlatParams(dev)
        for conv, bn, ci, co, k, s, pad in specs:
            fp.bucket(conv.split(".")[2] if ".layer" in conv else "stem")
            stem = (torch.cat([sd[conv + ".weight"].float(), torch.zeros(co, 1, 7, 7)], 1), None) if ci == 4 else None
            fp.lin(conv, co, ci, taps=k, kh=k, bias=False, src=stem)
            fp.vec(bn + ".weight", (co,))
            fp.vec(bn + ".bias", (co,))
        fp.bucket("heads")
        fp.lin("heads", self.NH, C, src=(torch.cat([sd[f"classifier_{t}.fc.weight"] for t, _ in self.heads], 0),
                                         torch.cat([sd[f"classifier_{t}.fc.bias"] for t, _ in self.heads], 0)))
        if self.loss_type == "all":
            for name, co, ci in (("wi", TD, C), ("wv", TD, C), ("wt", TD, C), ("mi", C, TD), ("mv", C, TD), ("mt", C, TD)):
                fp.lin(name, co, ci)
        self.fp = fp.build(sd, derive=False)    # (the derived copies: `_refresh_transposed`)
        self._optim_buffers()
        trained = fp.keys() | {f"classifier_{t}.fc.{p}" for t, _ in self.heads for p in ("weight", "bias")}
        # the running statistics of every BatchNorm in ONE flat buffer (a unit's mean, then its variance, each padded to 4 floats; `u.rmean` / `u.rvar`
        # are views): --skip_nonfinite copies it aside before a step and `mt4_restore_if_skipped_f32` puts it back when the step is skipped
        self._rstats = torch.zeros(sum(2 * _r4(co) for _, _, _, co, _, _, _ in specs), dtype=F32, device=dev)
        self._rstats_keep = None
        ro = 0
        for conv, bn, ci, co, k, s, pad in specs:
            u = _Unit()
            u.name, u.bn, u.cin, u.cout, u.k, u.stride, u.pad = conv, bn, ci, co, k, s, pad
            u.w, u.gw = fp.L[conv].w, fp.L[conv].gw
            u.gamma, u.ggamma = fp.V[bn + ".weight"].p, fp.V[bn + ".weight"].g
            u.beta, u.gbeta = fp.V[bn + ".bias"].p, fp.V[bn + ".bias"].g
            u.rmean, u.rvar = self._rstats[ro:ro + co], self._rstats[ro + _r4(co):ro + _r4(co) + co]
            ro += 2 * _r4(co)
            u.rmean.copy_(sd[bn + ".running_mean"].float())
            u.rvar.copy_(sd[bn + ".running_var"].float())
            self.nbt[bn] = int(sd[bn + ".num_batches_tracked"])
            u.wt, u.phase_w = None, None
            u.w16, u.wt16, u.phase_w16 = None, None, None
            self.units[conv] = u
            trained |= {bn + ".running_mean", bn + ".running_var", bn + ".num_batches_tracked"}
        # the weight average (`FlatTrainer._ema_update`) also averages the running statistics: a copy of the loaded buffer, stepped with E's record
        self._rstats_ema = self._rstats.clone() if self.ema is not None else None
        # float64 scratch of every BatchNorm reduction of a step (forward 2C -- or its STAT_REPLICAS copies when the convolution's epilogue
        # fills them -- and backward 2C), zeroed once per step
        rep = ops.STAT_REPLICAS if self.epilogue_stats else 1
        self._arena = torch.zeros(sum((2 * rep + 2) * u.cout for u in self.units.values()), dtype=torch.float64, device=dev)
        o = 0
        for u in self.units.values():
            u.sums_f, u.sums_b = self._arena[o:o + 2 * rep * u.cout], self._arena[o + 2 * rep * u.cout:o + (2 * rep + 2) * u.cout]
            o += (2 * rep + 2) * u.cout
        self._row_maps: Dict[tuple, torch.Tensor] = {}
        self._col_scales: Dict[int, torch.Tensor] = {}
        self._graphs: Dict[tuple, object] = {}
        self._extra = {k: sd[k].detach().clone() for k, _ in self._table if k not in trained}   # the trunk's unused 1000-way fc
        self.pos_weight = torch.tensor(sum((_POS_W[t] for t, _ in self.heads), []), dtype=F32, device=dev)
        self._refresh_table = None
        self._refresh_transposed()
        return self

    def _refresh_transposed(self):
        """every weight matrix derived from the master weights -- data-gradient operators (transposed with flipped taps; the four sub-pixel phase
        kernels of a stride-2 3x3), in bf16 mode also the bf16 copies the forward convolutions read -- rebuilt by ONE launch over a table
        (`mt4_refresh_weights`; a launch per matrix was ~350 launches = 1.5 ms per step).  Destinations are allocated once: captured graphs keep
        their addresses."""
        if getattr(self, "_refresh_table", None) is None:
            dt = torch.bfloat16 if self.op16 else F32
            tab = ops.RefreshTable(self.dev)
            for u in self.units.values():
                if u.cin == 4:
                    continue   # stem: the image needs no gradient; it stays fp32
                taps = u.k * u.k
                if self.op16:
                    u.w16 = tab.add(u.w, u.cout, u.cin, dt, False, range(taps), (u.k, u.k))
                if u.stride == 1 or u.k == 1:
                    wt = tab.add(u.w, u.cout, u.cin, dt, True, [taps - 1 - t for t in range(taps)], (u.k, u.k))
                    if self.op16:
                        u.wt16 = wt
                    else:
                        u.wt = wt
                else:   # 3x3 stride 2 pad 1: sub-pixel phases, phase parity -> original taps in the order of the data-gradient offsets 0, +1
                    sel = {0: [1], 1: [2, 0]}
                    ph_w = {}
                    for ph in (0, 1):
                        for pw in (0, 1):
                            khs, kws = len(sel[ph]), len(sel[pw])
                            dst = tab.add(u.w, u.cout, u.cin, dt, True, [sel[ph][a_] * 3 + sel[pw][b_] for a_ in range(khs) for b_ in range(kws)], (khs, kws))
                            ph_w[(ph, pw)] = (dst, khs, kws)
                    if self.op16:
                        u.phase_w16 = ph_w
                    else:
                        u.phase_w = ph_w
            self._refresh_table = tab
        self._refresh_table.run()
        # (the linear layers' data gradients transpose their small weights on the fly in _linear_bwd)

    _refresh = _refresh_transposed      # (what `FlatTrainer.apply_update` runs after the update)

    def _restore_skipped(self, state: torch.Tensor):
        """a skipped step (--skip_nonfinite) leaves the BatchNorm running statistics as `train_step` found them; `num_batches_tracked`, a host
        integer, has advanced all the same (as torch's does for a step GradScaler skips)"""
        if self.skip_nonfinite and self._rstats_keep is not None:
            ops.restore_if_skipped(self._rstats, self._rstats_keep, state)

    def _ema_step_extra(self, state):
        """the averaged running statistics follow E: the same record, the same skip rule (the statistics of a skipped step were restored above)"""
        ops.ema_step(self._rstats_ema, self._rstats, self._estate, state)

    def _load_ema_extra(self, state: Dict[str, torch.Tensor]):
        ro = 0
        for u in self.units.values():
            co = u.cout
            self._rstats_ema[ro:ro + co].copy_(state[u.bn + ".running_mean"].float())
            self._rstats_ema[ro + _r4(co):ro + _r4(co) + co].copy_(state[u.bn + ".running_var"].float())
            ro += 2 * _r4(co)

    # ------------------------------------------------------------------ deterministic mode: the workspace
    def workspace_bytes(self, b: int, h: int, w: int) -> int:
        """the largest workspace over the launches of a step on b frames of h x w, from the plan queries (host only: needs no device, no weights)"""
        C, TD = self.C, self.TD
        need = [ops.bce_logits_pw_plan(b, self.NH).bytes, ops.wgrad_conv1d_plan(1, b, self.NHP, C, 1, True).bytes]
        if self.loss_type == "all":
            need += [ops.distill_kl_plan(b, k).bytes for _, k in self.heads[:3]] + [ops.mse_plan(b * TD).bytes]
            need += [ops.wgrad_conv1d_plan(1, b, TD, C, 1, True).bytes, ops.wgrad_conv1d_plan(1, b, C, TD, 1, True).bytes]     # wi / wv / wt, mi / mv / mt
        hp, wp = ops.stem_pad_dims(h, w)
        ho, wo = ops.conv_out_size(hp, 7, 2, 0, 1), ops.conv_out_size(wp, 7, 2, 0, 1)
        for conv, _, cin, cout, k, stride, _ in self._unit_specs():
            if cin == 4:                                     # the stem; the trunk behind it starts from the max-pooled map
                uh, uw = ho, wo
                ho, wo = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
            elif conv.endswith("downsample.0"):              # (declared behind its block's convolutions: the block's output size)
                uh, uw = ho, wo
            else:
                uh, uw = ho, wo = (ho - 1) // stride + 1, (wo - 1) // stride + 1
            need.append(ops.bn_plan(b * uh * uw, cout).bytes)
            if self.op16 and cin != 4:
                need.append(ops.wgrad_conv2d_bf16_plan(b, uh, uw, cout, cin, k, stride).bytes)
            else:
                need.append(ops.wgrad_conv2d_plan(b, uh, uw, cout, cin, k, k).bytes)
        return max(need)

    def _ensure_workspace(self, b: int, h: int, w: int):
        """allocated before any capture of the shape, so that graphs keep its address; a larger shape later drops the graphs captured on the smaller one.
        Reuse along the stream is ordered: a launch's fold has read the workspace before the next producer writes it, and every fold into a bucket's
        region of G is on the stream ahead of `_reduce_bucket`."""
        n = self.workspace_bytes(b, h, w)
        if self._ws is None or self._ws.numel() * 4 < n:
            self._graphs.clear()
            self._ws = torch.empty((n + 15) // 16 * 4, dtype=F32, device=self.dev)
            self._ws64 = self._ws.view(torch.float64)

    def running_stats(self, ema: bool = False) -> Dict[str, torch.Tensor]:
        """the BatchNorm buffers only (what a train-mode forward changes); ema: the averaged statistics in place of the running ones"""
        out, ro = {}, 0
        for u in self.units.values():
            co = u.cout
            if ema:
                mean, var = self._rstats_ema[ro:ro + co], self._rstats_ema[ro + _r4(co):ro + _r4(co) + co]
            else:
                mean, var = u.rmean, u.rvar
            ro += 2 * _r4(co)
            out[u.bn + ".running_mean"], out[u.bn + ".running_var"] = mean.clone().cpu(), var.clone().cpu()
            out[u.bn + ".num_batches_tracked"] = torch.tensor(self.nbt[u.bn], dtype=torch.int64)
        return out

    def _export(self, which: str) -> Dict[str, torch.Tensor]:
        out = self.fp.export(which)
        stem = "basemodel.basemodel.conv1.weight"
        out[stem] = out[stem][:, :3].contiguous()            # (the image's 4th channel is padding)
        w, b = out.pop("heads.weight"), out.pop("heads.bias")
        o = 0
        for t, k in self.heads:
            out[f"classifier_{t}.fc.weight"], out[f"classifier_{t}.fc.bias"] = w[o:o + k].clone(), b[o:o + k].clone()
            o += k
        return out

    def state_dict(self, which: str = "p") -> Dict[str, torch.Tensor]:
        """which "ema": the weight average in place of P and the averaged running statistics in place of the running ones"""
        out = dict(self._extra, **self._export(which), **self.running_stats(which == "ema"))
        return {k: out[k] for k, _ in self._table}

    def grads(self) -> Dict[str, torch.Tensor]:
        return self._export("g")

    # ------------------------------------------------------------------ building blocks
    def _fwd_unit(self, u: _Unit, x, residual=None, relu=True, saved=None):
        w = u.w16 if (self.op16 and u.cin != 4) else u.w            # (bf16 mode: the stem reads the fp32 image with its fp32 weights)
        if self.epilogue_stats:
            # the BatchNorm statistics ride in the convolution's epilogue, mean / invstd are evaluated inside the apply launch: no pass over z
            z = ops.conv_nhwc(x, w, None, kh=u.k, kw=u.k, stride=(u.stride, u.stride), pad=(u.pad, u.pad), stat_sums=u.sums_f)
            b, ho, wo, c = z.shape
            apply = ops.bn_apply_sums_t if self.op16 else ops.bn_apply_sums
            a, mean, invstd = apply(z.view(-1, c), u.sums_f, u.gamma, u.beta, residual.view(-1, c) if residual is not None else None, relu, u.rmean, u.rvar)
            a = a.view(b, ho, wo, c)
            if saved is not None:
                saved.append((u, x, z, mean, invstd, a, relu, residual is not None))
            return a
        z = ops.conv_nhwc(x, w, None, kh=u.k, kw=u.k, stride=(u.stride, u.stride), pad=(u.pad, u.pad))
        b, ho, wo, c = z.shape
        z2 = z.view(-1, c)
        if self.op16:
            mean, invstd = ops.bn_stats_t(z2, u.rmean, u.rvar, sums=u.sums_f, workspace=self._ws64)
            a = ops.bn_apply_t(z2, mean, invstd, u.gamma, u.beta, residual.view(-1, c) if residual is not None else None, relu).view(b, ho, wo, c)
        else:
            mean, invstd = ops.bn_stats(z2, u.rmean, u.rvar, sums=u.sums_f, workspace=self._ws64)
            a = ops.bn_apply(z2, mean, invstd, u.gamma, u.beta, residual.view(-1, c) if residual is not None else None, relu).view(b, ho, wo, c)
        if saved is not None:
            saved.append((u, x, z, mean, invstd, a, relu, residual is not None))
        return a

    def _dgrad(self, u: _Unit, dz, x_shape, residual=None):
        """gradient w.r.t. the unit's input [B,H,W,Cin] from dz [B,Ho,Wo,Cout]"""
        b, h, w, cin = x_shape
        wt, phase_w, dt = (u.wt16, u.phase_w16, dz.dtype) if self.op16 else (u.wt, u.phase_w, F32)
        if u.stride == 1:
            p = u.k - 1 - u.pad
            return ops.conv_nhwc(dz, wt, None, kh=u.k, kw=u.k, pad=(p, p), residual=residual)
        assert h % 2 == 0 and w % 2 == 0, "stride-2 data gradient is built for even input sizes"
        ho, wo = dz.shape[1], dz.shape[2]
        dx = torch.zeros((b, h, w, cin), dtype=dt, device=dz.device) if (u.k == 1 and residual is None) else \
            (residual.clone() if u.k == 1 else torch.empty((b, h, w, cin), dtype=dt, device=dz.device))
        if u.k == 1:   # dX[2a][2b] = W^T dY[a][b]; every other position keeps the residual (or zero)
            rm = self._row_map(ho, wo, w, 0, 0)
            ops.conv_nhwc(dz, wt, None, kh=1, kw=1, residual=dx if residual is not None else None, out=dx, out_row_map=rm, out_rows_per_image=h * w)
            return dx
        for (ph, pw), (wsub, khs, kws) in phase_w.items():
            rm = self._row_map(ho, wo, w, ph, pw)
            ops.conv_nhwc(dz, wsub, None, kh=khs, kw=kws, out_hw=(ho, wo), residual=residual, out=dx, out_row_map=rm, out_rows_per_image=h * w)
        return dx

    def _row_map(self, ho, wo, w, ph, pw) -> torch.Tensor:
        """output rows (2a+ph, 2b+pw) of a [*, 2*ho, w] image for the ho x wo results of one sub-pixel phase (cached on the device)"""
        key = (ho, wo, w, ph, pw)
        if key not in self._row_maps:
            aa, bb = torch.meshgrid(torch.arange(ho), torch.arange(wo), indexing="ij")
            self._row_maps[key] = ((2 * aa + ph) * w + 2 * bb + pw).reshape(-1).to(torch.int32).to(self.dev)
        return self._row_maps[key]

    def _bwd_unit(self, rec, dy, residual_for_dx=None, want_dres=False, need_dx=True):
        u, x, z, mean, invstd, a, relu, has_res = rec
        c = z.shape[-1]
        if self.op16:   # (units without a residual input recompute their ReLU gate from z: the stored activation is not read)
            dz, dres = ops.bn_backward_t(dy.reshape(-1, c), a.view(-1, c) if relu else None, z.view(-1, c), mean, invstd, u.gamma, u.ggamma, u.gbeta,
                                         relu=relu, want_dres=want_dres, sums=u.sums_b, beta=u.beta if (relu and not has_res) else None,
                                         workspace=self._ws64)
        else:
            dz, dres = ops.bn_backward(dy.reshape(-1, c), a.view(-1, c) if relu else None, z.view(-1, c), mean, invstd, u.gamma, u.ggamma, u.gbeta,
                                       relu=relu, want_dres=want_dres, sums=u.sums_b, beta=u.beta if (relu and not has_res) else None,
                                       workspace=self._ws64)
        dz = dz.view(z.shape)
        if self.op16 and u.cin != 4:
            ops.wgrad_conv2d_bf16(dz, x, u.gw, u.k, u.stride, workspace=self._ws)                     # (adds to G, zeroed once per step)
        else:
            ops.wgrad_conv2d(dz, x, u.gw, u.k, u.k, (u.stride, u.stride), (u.pad, u.pad), zero=False, workspace=self._ws)   # G is zeroed once per step
        dx = self._dgrad(u, dz, x.shape, residual_for_dx) if need_dx else None
        return dx, (dres.view(z.shape) if dres is not None else None)

    def _linear_fwd(self, name, x):
        l = self.fp.L[name]
        return ops.linear(x, l.w, l.b)

    def _linear_bwd(self, name, dy, x, need_dx=True):
        l = self.fp.L[name]
        ops.wgrad_conv1d(dy, x, l.gw, batch=1, t=x.shape[0], taps=1, dil=1, pad=0, accumulate=True, bias_grad=l.gb,   # (G is zeroed once per step)
                         workspace=self._ws)
        if not need_dx:
            return None
        wt = ops.transpose_pack_conv1d(l.w, l.cout, l.cin, 1)
        return ops.linear(dy, wt, None)

    # ------------------------------------------------------------------ one step
    def train_step(self, frames, labels, teacher_pred, teacher_feat, apply_update: bool = True, use_graph: bool = False):
        """frames: normalised float32 NCHW [B,3,H,W] or uint8 NHWC [B,H,W,3] on the GPU; labels (y_i, y_v, y_t, y_ivt) multi-hot [B,K]
        (or one prepared fp32 [B,131] device tensor); teacher_pred 3 x raw logits [B,K]; teacher_feat 3 x [B,1536].
        Returns the dict of loss terms.  use_graph: replay a hipGraph of the whole forward+backward captured for this input shape
        (~900 launches become one; running statistics and gradients are updated by the replay exactly as by the eager step)."""
        dev = self.dev
        if not torch.is_tensor(labels) and self.loss_type != "all":       # (y_i, y_v, y_t, y_ivt) as the loader yields them: keep the task's
            labels = [labels["ivt".index(self.loss_type)]] if len(labels) == 4 else labels
        z = labels if torch.is_tensor(labels) else torch.cat([l.to(dev, F32) for l in labels], 1).contiguous()
        tp = [t.to(dev, F32).contiguous() for t in teacher_pred]
        tf = [t.to(dev, F32).contiguous() for t in teacher_feat]
        B = frames.shape[0]
        assert frames.is_cuda and tuple(z.shape) == (B, self.NH)
        if self.deterministic:
            self._ensure_workspace(B, *(frames.shape[1:3] if frames.dtype == torch.uint8 else frames.shape[2:4]))
        self.bucket_order = []            # gradient buckets in the order their all-reduce was issued this step (DDP)
        if self.skip_nonfinite:           # the running statistics as they are before the step, in one launch (`_restore_skipped`)
            if self._rstats_keep is None or self._rstats_keep.shape != self._rstats.shape:
                self._rstats_keep = torch.empty_like(self._rstats)
            self._rstats_keep.copy_(self._rstats)
        if use_graph:
            col_loss, soft, kdl = self._graph_step((tuple(frames.shape), frames.dtype), lambda f, zz, *t: self._fwd_bwd(f, zz, t[:3], t[3:]),
                                                   [frames, z, *tp, *tf])
        else:
            col_loss, soft, kdl = self._fwd_bwd(frames, z, tp, tf)
        for bn in self.nbt:
            self.nbt[bn] += 1
        r0, r1, r2 = self.rates
        cl, sk = col_loss.cpu(), torch.cat([soft, kdl]).cpu()
        terms, o = {}, 0
        hard = 0.0
        for t, k in self.heads:
            terms["hard_" + t] = float(cl[o:o + k].sum() / (B * k))
            hard += terms["hard_" + t]
            o += k
        terms.update(hard=hard, soft=float(sk[0]) / 3.0, kd=float(sk[1]) / 3.0)
        terms["loss"] = (r0 * terms["hard"] + r1 * terms["soft"] + r2 * terms["kd"]) if self.loss_type == "all" else hard   # `run.py:165-192`
        if apply_update:
            self.apply_update()
        return terms

    def forward_train(self, frames, teacher_feats=None):
        """The reference module call under `model.train()` (`Spatial_cnn/network.py:43-92`): BatchNorm on batch statistics (running statistics and
        num_batches_tracked advance, as in torch), the KD branch when teacher features are given (`loss_type all` and `args.train`, `network.py:47`).  frames uint8 NHWC or normalised float32 NCHW on the
        GPU; teacher_feats = (feat_i, feat_v, feat_t) [B, teacher_dim].  Returns ((kd_i | 0, logit_i), (kd_v | 0, logit_v), (kd_t | 0, logit_t),
        (feat, logit_ivt)) with zeros for heads the model does not have (`network.py:79-82`).  Forward only: gradients come from `train_step`."""
        from .synth import IMAGENET_MEAN, IMAGENET_STD
        if frames.dtype == torch.uint8:
            xp = ops.preprocess_u8(frames, IMAGENET_MEAN, IMAGENET_STD, F32)
        else:
            xp = ops.pad_nchw(frames, F32)
        B = frames.shape[0]
        if self.deterministic:
            self._ensure_workspace(B, *(frames.shape[1:3] if frames.dtype == torch.uint8 else frames.shape[2:4]))
        self._arena.zero_()
        pre, U = "basemodel.basemodel.", self.units
        x = ops.maxpool3x3s2(self._fwd_unit(U[pre + "conv1"], xp))
        bott = self.network == "resnet50"
        for li, n in enumerate(_DEPTHS[self.network], start=1):
            for bi in range(n):
                q = f"{pre}layer{li}.{bi}."
                idt = self._fwd_unit(U[q + "downsample.0"], x, relu=False) if (q + "downsample.0") in U else x
                o = self._fwd_unit(U[q + "conv1"], x)
                if bott:
                    o = self._fwd_unit(U[q + "conv2"], o)
                    x = self._fwd_unit(U[q + "conv3"], o, residual=idt)
                else:
                    x = self._fwd_unit(U[q + "conv2"], o, residual=idt)
        for bn in self.nbt:
            self.nbt[bn] += 1
        feat = ops.global_avgpool(x)
        logits = self._linear_fwd("heads", feat)
        outs, o = {}, 0
        for t, k in self.heads:
            outs[t] = logits[:, o:o + k]
            o += k
        for t, k in _ALL_HEADS:
            outs.setdefault(t, torch.zeros((B, k), device=self.dev))
        cams = [0, 0, 0]
        if teacher_feats is not None:
            assert self.loss_type == "all" and len(teacher_feats) == 3
            teas = [self._linear_fwd(m, t.to(self.dev, F32).contiguous()) for m, t in zip(("mi", "mv", "mt"), teacher_feats)]
            cams = [self._linear_fwd(wn, mx) for wn, mx in zip(("wi", "wv", "wt"), ops.kd_mix(feat, *teas))]
        return (cams[0], outs["i"]), (cams[1], outs["v"]), (cams[2], outs["t"]), (feat, outs["ivt"])

    def _fwd_bwd(self, frames, z, tp, tf):
        """device part of a step (enqueue only): forward, losses, backward into self.G.  Returns (per-column BCE sums, soft, kd)."""
        from .synth import IMAGENET_MEAN, IMAGENET_STD
        dev, C = self.dev, self.C
        if frames.dtype == torch.uint8:
            B, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
            xp = ops.preprocess_u8(frames, IMAGENET_MEAN, IMAGENET_STD, F32)
        else:
            B, H, W = frames.shape[0], frames.shape[2], frames.shape[3]
            xp = ops.pad_nchw(frames, F32)
        self._arena.zero_()
        self.G.zero_()
        saved: List[tuple] = []
        self.last_saved = saved          # (unit, input, conv output, mean, invstd, post-activation, relu, has residual) per conv+BN, forward order
        pre = "basemodel.basemodel."
        U = self.units
        a0 = self._fwd_unit(U[pre + "conv1"], xp, saved=saved)
        x = ops.maxpool3x3s2(a0)
        blocks = []
        bott = self.network == "resnet50"
        for li, n in enumerate(_DEPTHS[self.network], start=1):
            for bi in range(n):
                q = f"{pre}layer{li}.{bi}."
                first = len(saved)
                has_ds = (q + "downsample.0") in U
                idt = self._fwd_unit(U[q + "downsample.0"], x, relu=False, saved=saved) if has_ds else x
                o = self._fwd_unit(U[q + "conv1"], x, saved=saved)
                if bott:
                    o = self._fwd_unit(U[q + "conv2"], o, saved=saved)
                    x = self._fwd_unit(U[q + "conv3"], o, residual=idt, saved=saved)
                else:
                    x = self._fwd_unit(U[q + "conv2"], o, residual=idt, saved=saved)
                blocks.append((first, has_ds, bott, li))
        Bh, Hh, Wh, _ = x.shape
        feat = ops.global_avgpool(x)                                               # [B, C]
        # ---- heads, KD branch
        NH, NHP, kd_on = self.NH, self.NHP, self.loss_type == "all"
        logits = self._linear_fwd("heads", feat)                                   # [B, 132] (single task: its K rounded up to 4)
        # ---- losses and their gradients
        r0, r1, r2 = self.rates
        col_scale = self._col_scale(B)
        col_loss = torch.zeros(NH, device=dev)
        dlog = torch.zeros((B, NHP), device=dev)
        ops.bce_logits_pw(logits[:, :NH], z, self.pos_weight, col_scale, dlog, col_loss, workspace=self._ws)
        soft = torch.zeros(1, device=dev)
        kdl = torch.zeros(1, device=dev)
        if kd_on:
            teas = [self._linear_fwd(m, t) for m, t in zip(("mi", "mv", "mt"), tf)]
            mixed = ops.kd_mix(feat, *teas)
            cams = [self._linear_fwd(wn, mx) for wn, mx in zip(("wi", "wv", "wt"), mixed)]
            o = 0
            for (t, k), tpn in zip(self.heads[:3], tp):
                ops.distill_kl(logits[:, o:o + k], tpn, dlog[:, o:o + k], soft, self.temp, r1 / 3.0, accumulate=True, workspace=self._ws)
                o += k
            dcams = [ops.mse(c, t, kdl, r2 / 3.0, workspace=self._ws) for c, t in zip(cams, tf)]
        # ---- backward: heads + KD branch -> dfeat
        dfeat = self._linear_bwd("heads", dlog, feat)
        if kd_on:
            gs = [self._linear_bwd(wn, dc, mx) for wn, dc, mx in zip(("wi", "wv", "wt"), dcams, mixed)]
            ds_kd, dtau = ops.kd_mix_bwd(feat, teas, gs)
            dfeat = ops.mul_add(dfeat, torch.ones_like(dfeat), ds_kd)
            for n, (m, t) in enumerate(zip(("mi", "mv", "mt"), tf)):
                dte = dtau[:, n:n + 1].expand(B, C).contiguous()                    # d(tea_n)[b][:] = dtau[b][n]
                self._linear_bwd(m, dte, t, need_dx=False)
        self._reduce_bucket("heads")
        # ---- backward through the trunk
        dx = (ops.avgpool_bwd_bf16 if self.op16 else ops.avgpool_bwd)(dfeat, Bh, Hh * Wh, C).view(Bh, Hh, Wh, C)
        for bi_, (first, has_ds, bott, li) in reversed(list(enumerate(blocks))):
            recs = saved[first:first + (1 if has_ds else 0) + (3 if bott else 2)]
            main = recs[1:] if has_ds else recs
            d, dres = self._bwd_unit(main[-1], dx, want_dres=True)                  # last conv: ReLU gate after the residual add
            for rec in reversed(main[1:-1]):
                d, _ = self._bwd_unit(rec, d)
            if has_ds:
                d_id, _ = self._bwd_unit(recs[0], dres)                             # identity path through downsample conv+bn
                dx, _ = self._bwd_unit(main[0], d, residual_for_dx=d_id)
            else:
                dx, _ = self._bwd_unit(main[0], d, residual_for_dx=dres)
            if bi_ == 0 or blocks[bi_ - 1][3] != li:      # first block of the layer done: the layer's gradients are complete
                self._reduce_bucket(f"layer{li}")
        da0 = ops.maxpool3x3s2_bwd_bf16(a0, dx) if self.op16 else ops.maxpool3x3s2_bwd(a0, dx, gather=self.deterministic)   # (the bf16 form is a gather)
        self._bwd_unit(saved[0], da0, need_dx=False)
        self._reduce_bucket("stem")
        return col_loss, soft, kdl

    def _capture(self, fn, inputs, seg):
        keep = {n: (u.rmean.clone(), u.rvar.clone()) for n, u in self.units.items()}   # warm-up + capture runs must not count
        g = super()._capture(fn, inputs, seg)
        for n, u in self.units.items():
            u.rmean.copy_(keep[n][0])
            u.rvar.copy_(keep[n][1])
        return g

    def _col_scale(self, B: int) -> torch.Tensor:
        if B not in self._col_scales:
            r0 = self.rates[0] if self.loss_type == "all" else 1.0       # a single-task loss carries no rate (`run.py:165-179`)
            self._col_scales[B] = torch.cat([torch.full((k,), r0 / (B * k)) for _, k in self.heads]).to(self.dev)
        return self._col_scales[B]

    def relu_outputs(self) -> Dict[str, torch.Tensor]:
        """post-ReLU activations of the last step by BatchNorm name, NCHW on the host (tests: ReLU-gate comparison)"""
        return {u.bn: a.permute(0, 3, 1, 2).cpu() for (u, _, _, _, _, a, relu, _) in self.last_saved if relu}
