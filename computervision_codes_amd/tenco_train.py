"""One training step of the temporal head on MI355X: forward (train mode), BCE-with-logits over the 4 FPN levels,
backward and SGD, as `Temporal_tenco/run.py:181-235` does with autograd -- here as explicit HIP launches.

* forward: the inference kernels (`mt4_conv_nhwc`), keeping each layer's input and ReLU output;
* data gradients: the SAME implicit-GEMM kernel with transposed / tap-reversed weights (`mt4_transpose_pack_conv1d_f32`),
  the ReLU gate and the residual fan-in fused into its epilogue (act "relu_gate", `residual`);
* weight gradients: `mt4_wgrad_conv1d_f32` (fp32 MFMA, contraction over time), the bias gradient (column sums of dY) in the same launch;
* loss: `mt4_bce_logits_f32` on the concatenated [T][131] heads; optimizer: `mt4_sgd_step_f32` on ONE flat parameter
  buffer (packed layouts), so DDP is ONE all-reduce of the flat gradient buffer over RCCL (videos shard over ranks).

Randomness (75 % input mask, Dropout2d, per-layer Dropout; `network.py:43-48,123-127,194-196`) is drawn on the host side
of this class (`draw_masks`) or passed in explicitly, so that parity tests feed the oracle the same draw -- or, with
`train_step(draws=(seed, step))`, drawn on the device from a counter generator (`tenco_draws`, csrc/tenco_draw_kernels.hip): nothing
is drawn, transposed or uploaded by the host, and the step replays as a hipGraph whose {seed, step} input changes the draw.
Parameters that the FPN configuration never reaches (PG.conv_out, Rs.*.conv_1x1, Rs.*.conv_out, fpn.latlayer2/3) get no
gradient and, like torch.optim.SGD with `grad is None`, are left untouched.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops, tenco_draws
from .flatparams import FlatParams, FlatTrainer, Lin
from .flatparams import allreduce_sum_flat  # noqa: F401  (its import path before it moved to flatparams)
from .shapes import tenco_shapes
from .trainloop import lr_at_epoch  # noqa: F401  (its import path before it moved to trainloop)

HEADS = (("", 100, 1.0), ("_i", 6, 0.1), ("_v", 10, 0.1), ("_t", 15, 0.1))   # loss = 0.1 (i + v + t) + ivt (`run.py:212`)
NH = 131
NHP = 132  # padded to a multiple of 4 (16-byte rows for the gradient GEMMs)


class TencoTrainer(FlatTrainer):
    def __init__(self, num_layers_PG=11, num_layers_R=10, num_R=3, num_f_maps=512, dim=512, num_classes=100, lr=0.1, weight_decay=1e-5,
                 device: str = "cuda", process_group=None, overlap: bool = True, hier: bool = False, max_graphs: int = 64,
                 deterministic: bool = False, clip_grad_norm: float = 0.0, skip_nonfinite: bool = False, optim=None, causal: bool = False, ema=None):
        # overlap: a stage's gradients are all-reduced as soon as its backward has written them (DDP, `FlatTrainer`)
        super().__init__(lr, weight_decay, device, process_group, overlap, clip_grad_norm, skip_nonfinite, optim, ema)
        # hier = `args.hier` (`network.py:147,154-155`): AvgPool1d(7, 3) behind every refinement stage, so level l has its own length T_l, the FPN
        # resamples (`:96`) and `fusion` scores every level against the labels resized to it (`run.py:159-179,196-212`)
        self.hier = bool(hier)
        # causal (`temporal_tenco.VideoNas(causal=True)`): the dilated convs pad 2 d in front (`network.py:165-183`) -- the same launches with other
        # padding arguments: forward pad 2 d, data gradient the flipped-tap operator with pad 0, weight gradient pad 2 d
        self.causal = bool(causal)
        if self.causal and self.hier:
            from .temporal_tenco import CAUSAL_HIER_REASON
            raise ValueError(CAUSAL_HIER_REASON)
        # deterministic: every sum of the step that crosses workgroups (the weight and bias gradients, the BCE column sums) goes through the `_det`
        # entry points -- partials stored into `_ws`, folded in index order -- so a step is a pure function of its inputs, eager or replayed, at any
        # length.  Up to two ranks the all-reduce is one commutative add; beyond, the step is as reproducible as the collective.
        self.deterministic = bool(deterministic)
        self._ws: Optional[torch.Tensor] = None
        # max_graphs: how many captured steps (one per length and mode) are kept; a step whose graph would be one more runs eagerly
        self.max_graphs = int(max_graphs)
        assert num_classes == 100 and num_R == 3, "the FPN training recipe (Scripts/train_fold1.sh:28) has PG + 3 refinement stages"
        self.LP, self.LR, self.R, self.C, self.D = num_layers_PG, num_layers_R, num_R, num_f_maps, dim
        self._table = tenco_shapes(num_layers_PG, num_layers_R, num_R, num_f_maps, dim, 100, fpn=True)
        self._extra: Dict[str, torch.Tensor] = {}   # parameters outside the trained graph, kept verbatim
        self._scales: Dict[int, torch.Tensor] = {}
        self._label_idx: Dict[tuple, torch.Tensor] = {}
        self._slots = tenco_draws.stage_slots(self._stages())
        self._state_host: Optional[torch.Tensor] = None     # pinned {seed, step}: every step ends in a device->host copy, so one buffer serves

    # ------------------------------------------------------------------ parameters
    def _stages(self):
        return [("PG", self.LP)] + [(f"Rs.{r}", self.LR) for r in range(self.R)]

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        names = [k for k, _ in self._table]
        assert all(k in sd for k in names), "state dict incomplete"
        C, D = self.C, self.D
        # gradient buckets: "PG", "Rs.0".."Rs.2", "heads" (FPN lateral + heads); the derived copies are the transposed, tap-reversed
        # data-gradient operators (a launch of `mt4_transpose_pack_conv1d_f32` per layer was 98 launches = 0.5 ms of an 8 ms whole-video step)
        fp = FlatParams(self.dev)
        fp.bucket("PG")
        fp.lin("PG.conv_1x1", C, D, dgrad=False)          # (the input projection needs no data gradient)
        for prefix, n in self._stages():
            fp.bucket(prefix)
            for i in range(n):
                fp.lin(f"{prefix}.layers.{i}.conv_dilated", C, C, taps=3)
                fp.lin(f"{prefix}.layers.{i}.conv_1x1", C, C)
        fp.bucket("heads")
        fp.lin("fpn.latlayer1", C, C)
        fp.lin("heads", NH, C, src=(torch.cat([sd[f"conv_out{s}.weight"] for s, _, _ in HEADS], 0),   # [131 (+1 zero row), C, 1]
                                    torch.cat([sd[f"conv_out{s}.bias"] for s, _, _ in HEADS], 0)))
        self.fp, self.convs = fp.build(sd), fp.L
        self._optim_buffers()
        trained = fp.keys() | {f"conv_out{s}.{p}" for s, _, _ in HEADS for p in ("weight", "bias")}
        self._extra = {k: sd[k].detach().clone() for k in names if k not in trained}
        if self.deterministic and self._ws is None:
            self._ws = torch.empty(self.workspace_bytes() // 4, dtype=torch.float32, device=self.dev)
        self._refresh()
        return self

    def workspace_bytes(self) -> int:
        """the ONE workspace of the deterministic mode: the largest over the step's launches, from the plan queries.  A conv1d weight gradient has
        at most ceil(1024 / tiles) parts however long the video (`mt4_wgrad_conv1d_det_plan`), which a plan at 2^24 frames reaches, and the BCE at
        most 64 slabs -- so the size holds for every length and is allocated once, before any capture: graphs keep its address.  Reuse along the
        stream is ordered: a launch's fold has read the workspace before the next producer writes it."""
        big = 1 << 24
        return max([ops.wgrad_conv1d_plan(1, big, l.cout, l.cin, l.taps, True).bytes for l in self.convs.values()] + [ops.bce_logits_plan(big, NH).bytes])

    def _export(self, which: str) -> Dict[str, torch.Tensor]:
        out = self.fp.export(which)
        w, b = out.pop("heads.weight"), out.pop("heads.bias")
        o = 0
        for s, k, _ in HEADS:
            out[f"conv_out{s}.weight"], out[f"conv_out{s}.bias"] = w[o:o + k].clone(), b[o:o + k].clone()
            o += k
        return out

    def state_dict(self, which: str = "p") -> Dict[str, torch.Tensor]:
        """reference layout and key names (`Temporal_tenco/network.py`), on the CPU; which "ema": the weight average in place of P"""
        out = dict(self._extra, **self._export(which))
        return {k: out[k] for k, _ in self._table}

    def grads(self) -> Dict[str, torch.Tensor]:
        """gradients of the last step in reference layout (trained parameters only), on the CPU"""
        return self._export("g")

    def level_lengths(self, t: int) -> List[int]:
        """frames of the four FPN levels for a video of t frames: all t, or t -> (t - 7) // 3 + 1 per refinement stage with --hier"""
        out = [t]
        for _ in range(self.R):
            if self.hier:
                if t < 7:
                    raise ValueError(f"--hier: a level of {t} < 7 frames cannot be pooled (AvgPool1d(7, 3))")
                t = (t - 7) // 3 + 1
            out.append(t)
        return out

    # ------------------------------------------------------------------ randomness
    def draw_masks(self, t: int, generator: Optional[torch.Generator] = None) -> dict:
        """the train-time random pieces as reference-shaped tensors ([1,D,T] / [1,D,1] / {prefix: [1,C,T_stage]}: a refinement stage runs at the
        length of the level it reads)"""
        g = generator
        n = self.D * t
        perm = torch.randperm(n, generator=g)
        flat = torch.cat((torch.zeros(n - int(n * 0.75)), torch.ones(int(n * 0.75))))[perm]   # `network.py:44-47`
        masks = {"input_mask": flat.view(1, self.D, t), "channel_mask": (torch.rand(1, self.D, 1, generator=g) >= 0.5).float() * 2.0,
                 "layer_masks": {}}
        lens = self.level_lengths(t)
        for si, (prefix, nl) in enumerate(self._stages()):
            ts = lens[max(si - 1, 0)]
            for i in range(nl):
                masks["layer_masks"][f"{prefix}.layers.{i}"] = (torch.rand(1, self.C, ts, generator=g) >= 0.5).float() * 2.0
        return masks

    # ------------------------------------------------------------------ one step
    def _conv(self, x, c: Lin, dil=1, residual=None, act=None, transposed=False, cout=None):
        w = c.wt if transposed else c.w
        b = None if transposed else (c.b if cout is None else c.b[:cout])
        pad = dil if c.taps == 3 else 0
        if self.causal and c.taps == 3:      # y[t] = sum_k W_k x[t - (2 - k) d]; dx[s] = sum_k' wt[k'] dy[s + k' d] (taps past the last frame read zeros)
            return ops.conv_nhwc(x, w, b, kh=1, kw=3, pad=(0, 0 if transposed else 2 * dil), dil=(1, dil), residual=residual, act=act,
                                 out_hw=(1, x.shape[2]))
        return ops.conv_nhwc(x, w, b, kh=1, kw=c.taps, pad=(0, pad), dil=(1, dil), residual=residual, act=act)

    @ops.with_latency_tiles
    def train_step(self, x: torch.Tensor, labels: Dict[str, torch.Tensor], masks: Optional[dict] = None, apply_update: bool = True,
                   use_graph: bool = False, draws: Optional[tuple] = None, input_mask: bool = True):
        """x [1,T,D] fp32 on the GPU; labels {'': [T,100], '_i': [T,6], '_v': [T,10], '_t': [T,15]} multi-hot.
        Returns (loss, {head: loss term}).  use_graph: replay a hipGraph of the whole forward+backward captured for this T
        (not with explicit masks: those change every step) -- ~900 launches become one.
        draws = (seed, step): the random pieces of `tenco_draws.host_masks(seed, step, ...)` drawn on the device instead of passed in `masks`
        (one or the other); input_mask False leaves the 75 % mask out, as the driver does without --mask.  With draws a step does replay:
        {seed, step} is an input of the graph next to x and the labels.  At most `max_graphs` graphs are kept; beyond, a step runs eagerly."""
        assert x.dim() == 3 and x.shape[0] == 1 and x.shape[2] == self.D
        assert draws is None or not masks, "draws and masks are two ways to say the same thing: pass one"
        T, dev = x.shape[1], self.dev
        z = labels if torch.is_tensor(labels) else self.prepare_labels(labels)
        assert z.is_cuda and tuple(z.shape) == (T, NH) and z.dtype == torch.float32
        self.bucket_order = []            # gradient buckets in the order their all-reduce was issued this step (DDP)
        state = self._draw_state(*draws) if draws is not None else None
        key = T if draws is None else ("draws", T, bool(input_mask))
        if use_graph and not masks and ((key, self._segmented()) in self._graphs or len(self._graphs) < self.max_graphs):
            if draws is None:
                col_loss = self._graph_step(key, lambda xx, zz: self._fwd_bwd(xx, zz, None), [x, z])
            else:
                col_loss = self._graph_step(key, lambda xx, zz, st: self._fwd_bwd(xx, zz, None, st, input_mask), [x, z, state])
        else:
            col_loss = self._fwd_bwd(x, z, masks, state, input_mask)
        cl = col_loss.cpu()                                  # [levels, 131]: BCE sums per level and column
        lens = self.level_lengths(T)
        terms, o = {}, 0
        for s, k, _ in HEADS:
            terms[s] = float(sum(cl[l, o:o + k].sum() / (lens[l] * k) for l in range(len(lens))))   # BCEWithLogitsLoss(mean) per level (`run.py:196-210`)
            o += k
        loss = sum(w * terms[s] for s, _, w in HEADS)
        if apply_update:
            self.apply_update()
        return loss, terms

    def prepare_labels(self, labels: Dict[str, torch.Tensor]) -> torch.Tensor:
        """{'': [T,100], '_i': [T,6], '_v': [T,10], '_t': [T,15]} -> one fp32 [T,131] device tensor.  Goes through pinned
        memory: a pageable copy of this size makes ROCm pin the user pages on the fly, which was measured to stall the
        step by 70-170 ms every other step (tools/probe_train2.py)."""
        z = torch.cat([labels[s].to(torch.float32) for s, _, _ in HEADS], 1).contiguous()
        return z.pin_memory().to(self.dev, non_blocking=True) if not z.is_cuda else z

    def _draw_state(self, seed: int, step: int) -> torch.Tensor:
        """{seed, step} on the device (int64 [2], taken modulo 2^64) through one pinned buffer"""
        if self._state_host is None:
            self._state_host = torch.empty(2, dtype=torch.int64).pin_memory()
        self._state_host[0], self._state_host[1] = ops.wrap_int64(seed), ops.wrap_int64(step)
        return self._state_host.to(self.dev, non_blocking=True)

    def _fwd_bwd(self, x: torch.Tensor, z: torch.Tensor, masks: Optional[dict], state: Optional[torch.Tensor] = None,
                 input_mask: bool = True) -> torch.Tensor:
        """device part of a step (enqueue only): forward, loss, backward into self.G.  Returns the per-column loss sums.
        state: {seed, step} on the device -- the draws are made by the kernels of csrc/tenco_draw_kernels.hip (the layer masks regenerated in
        the backward instead of stored) and `masks` is not looked at."""
        T, C, dev = x.shape[1], self.C, self.dev
        cv, ws = self.convs, self._ws                      # ws: None (atomic sums) or the deterministic mode's workspace
        to_rows = lambda m: m[0].transpose(0, 1).contiguous().to(dev)        # [1,C,T] -> [T,C]
        h0 = x.contiguous().view(1, 1, T, self.D)
        sl = self._slots
        if state is not None:
            masks = None
            n = T * self.D
            thr = ops.select_kth_key(n, (3 * n) // 4, state, sl["input_keys"]) if input_mask else None     # `int(n * 0.75)` ones (`network.py:45`)
            h0 = ops.tenco_input_draw(h0, state, sl["input_keys"], thr, sl["channel"])
        if masks and masks.get("input_mask") is not None:
            h0 = ops.mul_add(h0, to_rows(masks["input_mask"]).view_as(h0))
        if masks and masks.get("channel_mask") is not None:
            h0 = ops.mul_add(h0, masks["channel_mask"][0].transpose(0, 1).expand(T, self.D).contiguous().to(dev).view_as(h0))
        lm = {k: to_rows(v).view(1, 1, v.shape[-1], C) for k, v in ((masks or {}).get("layer_masks") or {}).items()}

        # ---- forward, saving layer inputs z and ReLU outputs u
        lens = self.level_lengths(T)                       # frames per FPN level (all T without --hier)
        saved: List[tuple] = []
        f = self._conv(h0, cv["PG.conv_1x1"])
        stage_out = []
        for si, (prefix, n) in enumerate(self._stages()):
            ts = lens[max(si - 1, 0)]                      # a refinement stage runs at the length of the level it reads
            for i in range(n):
                p = f"{prefix}.layers.{i}"
                d = 2 ** i
                u = self._conv(f, cv[p + ".conv_dilated"], dil=d, act="relu")
                if state is not None:
                    fn = ops.dropout_mul_add(self._conv(u, cv[p + ".conv_1x1"]), state, sl[p], 0.5, c=f)
                elif p in lm:
                    o = self._conv(u, cv[p + ".conv_1x1"])
                    fn = ops.mul_add(o, lm[p], f)
                else:
                    fn = self._conv(u, cv[p + ".conv_1x1"], residual=f)
                saved.append((p, d, f, u, ts))
                f = fn
            if self.hier and si > 0:                       # `Refinement.forward` (:154-155): the stage's feature is the pooled map
                f = ops.avgpool1d_rows(f.view(1, ts, C), 7, 3).view(1, 1, lens[si], C)
            stage_out.append(f)
        c1, c2, c3, p4 = stage_out
        lat = cv["fpn.latlayer1"]
        # `FPN._upsample_add` (:93-96): linear interpolation to the lateral's length (the identity at equal lengths) + lateral
        up = (lambda xx, li: ops.interp_linear_rows(xx.view(1, lens[li + 1], C), lens[li]).view(1, 1, lens[li], C)) if self.hier else (lambda xx, li: xx)
        p3 = self._conv(c3, lat, residual=up(p4, 2))
        p2 = self._conv(c2, lat, residual=up(p3, 1))
        p1 = self._conv(c1, lat, residual=up(p2, 0))
        levels = [p1, p2, p3, p4]
        hd = cv["heads"]
        logits = [self._conv(l, hd) for l in levels]                          # [1,1,T_l,132], column 131 is padding (= 0)

        # ---- loss + dL/dlogits
        # every weight / bias gradient below ADDS into the flat buffer, zeroed here once: zeroing per tensor in front of its (atomic) sums was
        # ~150 launches = 0.8 ms of an 8 ms whole-video step
        self.G.zero_()
        col_loss = torch.zeros((len(levels), NH), device=dev)
        dys = []
        for li, lg in enumerate(logits):
            tl = lens[li]
            dy = torch.zeros((1, 1, tl, NHP), device=dev)
            ops.bce_logits(lg.view(tl, NHP)[:, :NH], self._level_labels(z, T, tl), self._col_scale(tl), dy.view(tl, NHP), col_loss[li], workspace=ws)
            dys.append(dy)
        # ---- backward: heads and FPN (top-down adds fan the level gradients into each other)
        g = None
        dstage = [None, None, None, None]
        for li, (lv, dy) in enumerate(zip(levels, dys)):
            tl = lens[li]
            ops.wgrad_conv1d(dy.view(tl, NHP), lv.view(tl, C), hd.gw, batch=1, t=tl, taps=1, dil=1, pad=0, accumulate=True, bias_grad=hd.gb, workspace=ws)
            if g is not None and self.hier:                                    # p_{li} = interp(p_{li+1}) + lateral: the adjoint of the resampling
                g = ops.interp_linear_rows_bwd(g.view(1, lens[li - 1], C), tl).view(1, 1, tl, C)
            g = self._conv(dy, hd, transposed=True, residual=g)               # gradient w.r.t. p_{li+1}
            if li < 3:
                cl_ = stage_out[li]                                            # lateral input c_{li+1}
                ops.wgrad_conv1d(g.view(tl, C), cl_.view(tl, C), lat.gw, batch=1, t=tl, taps=1, dil=1, pad=0, accumulate=True, bias_grad=lat.gb, workspace=ws)
                dstage[li] = self._conv(g, lat, transposed=True)
            else:
                dstage[3] = g                                                  # p4 is the last stage's (pooled) output itself
        self._reduce_bucket("heads")
        # ---- backward through the stages, last to first
        df = dstage[3]
        idx = len(saved)
        for si in range(len(self._stages()) - 1, -1, -1):
            prefix, n = self._stages()[si]
            ts = lens[max(si - 1, 0)]
            if self.hier and si > 0:                                           # through the stage's AvgPool1d(7, 3)
                df = ops.avgpool1d_rows_bwd(df.view(1, lens[si], C), ts, 7, 3).view(1, 1, ts, C)
            for i in range(n - 1, -1, -1):
                idx -= 1
                p, d, zin, u, _ = saved[idx]
                w1, wd = cv[p + ".conv_1x1"], cv[p + ".conv_dilated"]
                do = ops.dropout_mul_add(df, state, sl[p], 0.5) if state is not None else ops.mul_add(df, lm[p]) if p in lm else df
                ops.wgrad_conv1d(do.view(ts, C), u.view(ts, C), w1.gw, batch=1, t=ts, taps=1, dil=1, pad=0, accumulate=True, bias_grad=w1.gb, workspace=ws)
                du = self._conv(do, w1, transposed=True, residual=u, act="relu_gate")
                ops.wgrad_conv1d(du.view(ts, C), zin.view(ts, C), wd.gw, batch=1, t=ts, taps=3, dil=d, pad=2 * d if self.causal else d, accumulate=True, bias_grad=wd.gb, workspace=ws)
                df = self._conv(du, wd, dil=d, transposed=True, residual=df)
            if si > 0:
                df = ops.mul_add(df, torch.ones_like(df), dstage[si - 1])      # + gradient of this stage's input as lateral c
                self._reduce_bucket(prefix)                                    # this stage's gradients are complete: exchange them behind
        pin = cv["PG.conv_1x1"]                                                #   the backward of the earlier stages
        ops.wgrad_conv1d(df.view(T, C), h0.view(T, self.D), pin.gw, batch=1, t=T, taps=1, dil=1, pad=0, accumulate=True, bias_grad=pin.gb, workspace=ws)
        self._reduce_bucket("PG")
        return col_loss

    def _level_labels(self, z: torch.Tensor, T: int, tl: int) -> torch.Tensor:
        """`fusion` (`run.py:169-175`): the labels of a level of tl != T frames are `F.interpolate(labels, size=tl, mode='nearest')` of the [T, K] rows:
        row j <- row min(floor(j * float32(T / tl)), T - 1) (torch's nearest index arithmetic, in float32)"""
        if tl == T:
            return z
        idx = self._label_idx.get((T, tl))
        if idx is None:
            import numpy as np
            scale = np.float32(T) / np.float32(tl)
            src = np.minimum(np.floor(np.arange(tl, dtype=np.float32) * scale).astype(np.int64), T - 1)
            idx = self._label_idx[(T, tl)] = torch.from_numpy(src).to(self.dev)
        return z.index_select(0, idx)

    def _col_scale(self, T: int) -> torch.Tensor:
        cs = self._scales.get(T)
        if cs is None:
            cs = self._scales[T] = torch.cat([torch.full((k,), w / (T * k)) for _, k, w in HEADS]).to(self.dev)
        return cs
