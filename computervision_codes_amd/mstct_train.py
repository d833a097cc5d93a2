"""One training step of the MS-TCT temporal teacher on MI355X: forward (train mode), BCE-with-logits, backward and SGD, as
`Temporal_mstct/run.py:147-235` does with torch autograd over `Temporal_mstct/network.py:75-101` -- here as explicit HIP launches.

* every nn.Linear / Conv1d: the implicit-GEMM kernel forward (`mt4_conv_nhwc`), the same kernel with transposed weights for the data
  gradient, `mt4_wgrad_conv1d_f32` + `mt4_colsum_f32` for the parameter gradients;
* Global_Relational_Block (`Temporal_Encoder.py:76-88`): q.k^T, softmax, P.v and their four backward products through the strided batched
  GEMM `mt4_bgemm_f32` on head slices of the packed q / kv buffers (no permutes), `mt4_softmax_rows_f32` / `mt4_softmax_bwd_rows_f32`;
  the probabilities P [B,8,T,T] are kept for the backward;
* nn.LayerNorm: `mt4_layernorm` / `mt4_layernorm_bwd_f32`; Local_Relational_Block (`:34-43`): `mt4_dwconv1d_k3` (+GELU) and
  `mt4_gelu_bwd_f32`, `mt4_dwconv1d_k3_bwd_f32`;
* Temporal_Mixer (`TS_Mixer.py:50-84`): at equal lengths `interpolate` is the identity and the three 1x1 convs that meet in each scale's
  output apply to the same input, so the forward uses their summed weight (rebuilt on the device every step) and each of the three
  receives the same gradient -- exactly what autograd gives;
* loss `mt4_bce_logits_pw_f32` (pos_weight for i / v / t, none for ivt: `run.py:331-334`), optimizer `mt4_sgd_step_f32` on ONE flat
  parameter buffer, so DDP is one all-reduce of the flat gradient buffer over RCCL (windows shard over ranks).

The two nn.Dropout(0.5) of `network.py:58,76,108,113` are drawn on the host (`draw_masks`) or passed in, so that parity tests feed the
oracle the same draw.  float32 throughout.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import ops
from .flatparams import FlatParams, GemmTrainer, Lin, _r4
from .shapes import mstct_shapes

F32 = torch.float32
NCLS = {"i": 6, "v": 10, "t": 15, "ivt": 100}
# `Temporal_mstct/run.py:322-328` (the class weights of the CholecT45 label statistics; same tables as Spatial_cnn/run.py:306-311)
POS_W = {"i": [0.93487068, 0.94234964, 0.93487068, 1.18448115, 1.02368339, 0.97974447],
         "v": [0.60002400, 0.60002400, 0.60002400, 0.61682467, 0.67082683, 0.80163207, 0.70562823, 2.11208448, 2.69230769, 0.60062402],
         "t": [0.49752894, 0.52041527, 0.49752894, 0.51394739, 2.71899565, 1.75577963, 0.58509403, 1.25228034, 0.49752894, 2.42993134,
               0.49802647, 0.87266576, 1.36074165, 0.50150917, 0.49802647],
         "ivt": None}


class MstctTrainer(GemmTrainer):
    def __init__(self, inter_channels: Sequence[int] = (256, 384, 576, 864), num_block: int = 2, head: int = 8, mlp_ratio: int = 8,
                 in_feat_dim: int = 1536, final_embedding_dim: int = 512, loss_type: str = "i", lr: float = 0.1, weight_decay: float = 1e-5,
                 device: str = "cuda", process_group=None, operand_dtype: torch.dtype = torch.float32, clip_grad_norm: float = 0.0,
                 skip_nonfinite: bool = False, optim=None, ema=None):
        assert loss_type in NCLS
        super().__init__(lr, weight_decay, device, process_group, clip_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite, optim=optim, ema=ema)
        assert operand_dtype in (torch.float32, torch.bfloat16)
        # bfloat16: the nn.Linear GEMMs (forward, data and weight gradients) read bf16 copies of their operands -- activations are cast on the
        # way in (`mt4_cast_f32_bf16`), weights re-derived from the fp32 masters after every step -- and accumulate / store in fp32; everything
        # between the GEMMs (LayerNorm, softmax, GELU, attention products, the k = 3 merge convolutions, the loss) stays fp32
        self.op16 = operand_dtype == torch.bfloat16
        self.inter, self.nb, self.H, self.ratio = tuple(inter_channels), num_block, head, mlp_ratio
        self.D, self.E, self.loss_type, self.K = in_feat_dim, final_embedding_dim, loss_type, NCLS[loss_type]
        self.KP = _r4(self.K)
        self._table = mstct_shapes(in_feat_dim, self.inter, num_block, mlp_ratio, final_embedding_dim, loss_type)

    # ------------------------------------------------------------------ parameters
    def _specs(self):
        """in flat-buffer order: lin (name, cout, cin, taps), then vec (name, shape)"""
        lin, vec = [], []
        cin = self.D
        for s, c in enumerate(self.inter, start=1):
            m = f"TemporalEncoder.Temporal_Merging_Block{s}"
            lin.append((m + ".proj", c, cin, 3))
            vec += [(m + ".norm.weight", (c,)), (m + ".norm.bias", (c,))]
            for b in range(self.nb):
                q = f"TemporalEncoder.block{s}.{b}"
                g, l = q + ".Global_Relational_Block", q + ".Local_Relational_Block"
                vec += [(q + ".norm1.weight", (c,)), (q + ".norm1.bias", (c,)), (q + ".norm2.weight", (c,)), (q + ".norm2.bias", (c,)),
                        (l + ".TC.weight", (self.ratio * c, 3)), (l + ".TC.bias", (self.ratio * c,))]
                lin += [(g + ".q", c, c, 1), (g + ".kv", 2 * c, c, 1), (g + ".proj", c, c, 1), (l + ".linear1", self.ratio * c, c, 1),
                        (l + ".linear2", c, self.ratio * c, 1)]
            vec += [(f"TemporalEncoder.norm{s}.weight", (c,)), (f"TemporalEncoder.norm{s}.bias", (c,))]
            cin = c
        for i, c in zip((4, 3, 2, 1), reversed(self.inter)):
            lin.append((f"Temporal_Mixer.linear_f{i}.proj", self.E, c, 1))
        for i in range(1, 10):
            lin.append((f"Temporal_Mixer.linear{i}", self.E, self.E, 1))
        q = f"classifier_{self.loss_type}"
        lin += [(q + ".linear_fuse", self.E, 4 * self.E, 1), (q + ".linear_pred", self.K, self.E, 1)]
        return lin, vec

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        names = [k for k, _ in self._table]
        assert all(k in sd for k in names), "state dict incomplete"
        lin, vec = self._specs()
        # every derived matrix -- the fp32 transposed (tap-flipped) weights of the data gradients and, in the bf16-operand mode, the bf16 forward /
        # transposed copies of the eligible nn.Linear layers -- comes from ONE launch over a table after each parameter change
        fp = FlatParams(self.dev, self.op16)
        for name, cout, cin, taps in lin:
            fp.lin(name, cout, cin, taps=taps, dgrad=not name.endswith("Block1.proj"))   # (the first merge conv needs no data gradient)
        for name, shp in vec:
            fp.vec(name, shp)
        self.fp = fp.build(sd)
        self._optim_buffers()
        self.lins = fp.L
        E = self.E
        kp = ops.packed_k(E, 1, 1, F32)
        self._wsum = torch.zeros((3, E, kp), dtype=F32, device=self.dev)       # summed 1x1 mixer weights of scales 3, 2, 1
        self._bsum = torch.zeros((3, E), dtype=F32, device=self.dev)
        self._wsum_t = torch.zeros((3, E, ops.packed_k(E, 1, 1, F32)), dtype=F32, device=self.dev)
        self._refresh()
        return self

    _MIX = ((3, (7, 1, 4)), (2, (8, 2, 5)), (1, (9, 3, 6)))     # scale -> the linear_k that meet in its output (`TS_Mixer.py:66-79`)

    def _refresh(self):
        """derived copies after a parameter change: transposed weights for the data gradients, summed mixer weights"""
        self.fp.tab.run()
        for j, (_, ids) in enumerate(self._MIX):
            for n, i in enumerate(ids):
                l = self.lins[f"Temporal_Mixer.linear{i}"]
                ops.axpby_(l.w, self._wsum[j], 1.0, 0.0 if n == 0 else 1.0)
                ops.axpby_(l.b, self._bsum[j], 1.0, 0.0 if n == 0 else 1.0)
            ops.transpose_pack_conv1d(self._wsum[j], self.E, self.E, 1, out=self._wsum_t[j])

    def state_dict(self, which: str = "p") -> Dict[str, torch.Tensor]:
        """reference layout and key names (`Temporal_mstct/network.py`), on the CPU; which "ema": the weight average in place of P"""
        out = self.fp.export(which)
        return {k: out[k] for k, _ in self._table}

    def grads(self) -> Dict[str, torch.Tensor]:
        return self.fp.export("g")

    # ------------------------------------------------------------------ randomness
    def draw_masks(self, b: int, t: int, generator: Optional[torch.Generator] = None) -> dict:
        """the two nn.Dropout(0.5) draws as reference-shaped tensors: input [B,D,T], feat [B,E,T]; values 0 or 2"""
        g = generator
        return {"input": (torch.rand(b, self.D, t, generator=g) >= 0.5).float() * 2.0,
                "feat": (torch.rand(b, self.E, t, generator=g) >= 0.5).float() * 2.0}

    def draw_masks_device(self, b: int, t: int, seed: int, step: int) -> dict:
        """the same two draws made on the device, already in row layout ([B*T,D] / [B*T,E]): what the training driver uses (a host draw of
        31 x 1536 x 256 values and its upload cost more than the step).  Element i of stream 2*step (+1) of `synth.uniform01(seed, .)`."""
        return {"input_rows": ops.dropout_mask((b * t, self.D), seed, 2 * step, 0.5, self.dev),
                "feat_rows": ops.dropout_mask((b * t, self.E), seed, 2 * step + 1, 0.5, self.dev)}

    # ------------------------------------------------------------------ building blocks
    def _dgrad(self, dy2d, c: Lin, residual=None):
        if c.wt16 is not None:
            dy2d = dy2d if dy2d.is_contiguous() else dy2d.contiguous()
            return ops.linear(self._cast(dy2d, grad=True), c.wt16, None, residual=residual, out_dtype=F32)
        return ops.linear(dy2d, c.wt, None, residual=residual)

    def _wgrad(self, dy2d, x2d, c: Lin):
        m = dy2d.shape[0]
        if c.w16 is not None and m % 16 == 0 and dy2d.is_contiguous() and x2d.is_contiguous():    # rows as a [M / 16, 16] pixel grid of one image
            ops.wgrad_conv2d_bf16(self._cast(dy2d, grad=True).view(1, m // 16, 16, c.cout), self._cast(x2d).view(1, m // 16, 16, c.cin), c.gw, 1, 1)
            ops.colsum(dy2d, c.gb, accumulate=True)
        else:   # (G is zeroed once per step; the bias gradient rides in the weight gradient's launch)
            ops.wgrad_conv1d(dy2d, x2d, c.gw, batch=1, t=m, taps=1, dil=1, pad=0, accumulate=True, bias_grad=c.gb)

    def _attention_fwd(self, q, kv, b, t, c):
        hd, H = c // self.H, self.H
        P = torch.empty((b, H, t, t), dtype=F32, device=self.dev)
        ops.bgemm(q, kv, P, m=t, n=t, k=hd, nb0=H, nb1=b, a_strides=(hd, t * c, c, 1), b_strides=(hd, t * 2 * c, 1, 2 * c),
                  c_strides=(t * t, H * t * t, t, 1))
        ops.softmax_rows_(P, hd ** -0.5)
        o = torch.empty((b * t, c), dtype=F32, device=self.dev)
        ops.bgemm(P, kv[:, c:], o, m=t, n=hd, k=t, nb0=H, nb1=b, a_strides=(t * t, H * t * t, t, 1), b_strides=(hd, t * 2 * c, 2 * c, 1),
                  c_strides=(hd, t * c, c, 1))
        return P, o

    def _attention_bwd(self, do, q, kv, P, b, t, c):
        hd, H = c // self.H, self.H
        dq = torch.empty((b * t, c), dtype=F32, device=self.dev)
        dkv = torch.empty((b * t, 2 * c), dtype=F32, device=self.dev)
        sp, sq, skv = (t * t, H * t * t), (hd, t * c), (hd, t * 2 * c)
        # dV = P^T dO
        ops.bgemm(P, do, dkv[:, c:], m=t, n=hd, k=t, nb0=H, nb1=b, a_strides=sp + (1, t), b_strides=sq + (c, 1), c_strides=skv + (2 * c, 1))
        # dP = dO V^T, then dS in place
        dP = torch.empty_like(P)
        ops.bgemm(do, kv[:, c:], dP, m=t, n=t, k=hd, nb0=H, nb1=b, a_strides=sq + (c, 1), b_strides=skv + (1, 2 * c), c_strides=sp + (t, 1))
        ops.softmax_bwd_rows_(P, dP, hd ** -0.5)
        # dQ = dS K, dK = dS^T Q
        ops.bgemm(dP, kv, dq, m=t, n=hd, k=t, nb0=H, nb1=b, a_strides=sp + (t, 1), b_strides=skv + (2 * c, 1), c_strides=sq + (c, 1))
        ops.bgemm(dP, q, dkv, m=t, n=hd, k=t, nb0=H, nb1=b, a_strides=sp + (1, t), b_strides=sq + (c, 1), c_strides=skv + (2 * c, 1))
        return dq, dkv

    # ------------------------------------------------------------------ forward + backward (enqueue only)
    def _fwd_bwd(self, x_btd: torch.Tensor, z: torch.Tensor, mask_in: Optional[torch.Tensor], mask_feat: Optional[torch.Tensor]):
        """x [B,T,D] frame-major, z [B*T,K] multi-hot fp32, masks as ROWS ([B*T,D] / [B*T,E]) or None.  Returns per-column loss sums [K]."""
        b, t, d = x_btd.shape
        M, E, L = b * t, self.E, self.lins
        self._begin_step()
        x = x_btd.contiguous().view(M, d)
        if mask_in is not None:
            x = ops.mul_add(x, mask_in)
        saved, feats = [], []
        cin = d
        for s, c in enumerate(self.inter, start=1):
            m = f"TemporalEncoder.Temporal_Merging_Block{s}"
            pm = ops.conv_nhwc(x.view(b, 1, t, cin), L[m + ".proj"].w, L[m + ".proj"].b, kh=1, kw=3, pad=(0, 1)).view(M, c)
            y = self._ln(pm, m + ".norm")
            st = dict(x_in=x, pm=pm, blocks=[])
            for bi in range(self.nb):
                q_ = f"TemporalEncoder.block{s}.{bi}"
                g_, l_ = q_ + ".Global_Relational_Block", q_ + ".Local_Relational_Block"
                n1 = self._ln(y, q_ + ".norm1")
                q = self._fwd(n1, L[g_ + ".q"])
                kv = self._fwd(n1, L[g_ + ".kv"])
                P, o = self._attention_fwd(q, kv, b, t, c)
                x_mid = self._fwd(o, L[g_ + ".proj"], residual=y)
                n2 = self._ln(x_mid, q_ + ".norm2")
                h1 = self._fwd(n2, L[l_ + ".linear1"])
                h2 = ops.dwconv1d_k3(h1.view(b, t, -1), self.fp.V[l_ + ".TC.weight"].p, self.fp.V[l_ + ".TC.bias"].p, act="none").view(M, -1)
                h3 = ops.gelu(h2)
                y_out = self._fwd(h3, L[l_ + ".linear2"], residual=x_mid)
                st["blocks"].append(dict(x_in=y, n1=n1, q=q, kv=kv, P=P, o=o, x_mid=x_mid, n2=n2, h1=h1, h2=h2, h3=h3))
                y = y_out
            st["pre_norm"] = y
            f = self._ln(y, f"TemporalEncoder.norm{s}")
            feats.append(f)
            saved.append(st)
            x, cin = f, c
        f1, f2, f3, f4 = feats
        concat = torch.empty((M, 4 * E), dtype=F32, device=self.dev)
        p4 = self._fwd(f4, L["Temporal_Mixer.linear_f4.proj"])
        concat[:, 0:E].copy_(p4)
        for slot, (j, (sc, _)) in enumerate(zip(range(3), self._MIX), start=1):
            r = self._fwd(feats[sc - 1], L[f"Temporal_Mixer.linear_f{sc}.proj"])
            ops.axpby_(r, r, 3.0, 0.0)                                                   # _f + (_f) + (_f): three residual copies
            ops.linear(p4, self._wsum[j], self._bsum[j], residual=r, out=concat[:, slot * E:(slot + 1) * E])
        cq = f"classifier_{self.loss_type}"
        zf = self._fwd(concat, L[cq + ".linear_fuse"])
        zd = ops.mul_add(zf, mask_feat) if mask_feat is not None else zf
        logits = self._fwd(zd, L[cq + ".linear_pred"])                                   # [M, KP]
        # ---- loss + its gradient
        dy = torch.zeros((M, self.KP), dtype=F32, device=self.dev)
        col_loss = torch.zeros(self.K, dtype=F32, device=self.dev)
        ops.bce_logits_pw(logits, z, self._pos_w, self._col_scale(M), dy, col_loss)
        # ---- backward: classifier
        self._wgrad(dy, zd, L[cq + ".linear_pred"])
        dzd = self._dgrad(dy, L[cq + ".linear_pred"])
        dzf = ops.mul_add(dzd, mask_feat) if mask_feat is not None else dzd
        self._wgrad(dzf, concat, L[cq + ".linear_fuse"])
        wt_fuse = L[cq + ".linear_fuse"].wt                                              # [4E rows (its cin)][Kpad(E)]
        dslots = [ops.linear(dzf, wt_fuse[sidx * E:(sidx + 1) * E], None) for sidx in range(4)]   # d concat, one contiguous block per slot
        # ---- backward: mixer
        dp4 = dslots[0]
        dfeat: List[Optional[torch.Tensor]] = [None, None, None, None]
        for slot, (j, (sc, ids)) in enumerate(zip(range(3), self._MIX), start=1):
            dout = dslots[slot]
            first = L[f"Temporal_Mixer.linear{ids[0]}"]
            self._wgrad(dout, p4, first)                                                 # the three 1x1 convs of this scale see the same
            for i in ids[1:]:                                                            # input and output gradient
                o_ = L[f"Temporal_Mixer.linear{i}"]
                ops.axpby_(first.gw, o_.gw, 1.0, 0.0)
                ops.axpby_(first.gb, o_.gb, 1.0, 0.0)
            dp4 = ops.linear(dout, self._wsum_t[j], None, residual=dp4)
            dr = ops.axpby_(dout, torch.empty_like(dout), 3.0, 0.0)
            lf = L[f"Temporal_Mixer.linear_f{sc}.proj"]
            self._wgrad(dr, feats[sc - 1], lf)
            dfeat[sc - 1] = self._dgrad(dr, lf)
        lf4 = L["Temporal_Mixer.linear_f4.proj"]
        self._wgrad(dp4, f4, lf4)
        dfeat[3] = self._dgrad(dp4, lf4)
        # ---- backward: encoder stages 4 .. 1
        gnext = None                                                                     # gradient arriving through the next stage's merge conv
        for s in range(4, 0, -1):
            c, st = self.inter[s - 1], saved[s - 1]
            gf = dfeat[s - 1]
            if gnext is not None:
                ops.axpby_(gnext, gf, 1.0, 1.0)
            g = self._ln_bwd(gf, st["pre_norm"], f"TemporalEncoder.norm{s}")
            for bi in range(self.nb - 1, -1, -1):
                blk = st["blocks"][bi]
                q_ = f"TemporalEncoder.block{s}.{bi}"
                g_, l_ = q_ + ".Global_Relational_Block", q_ + ".Local_Relational_Block"
                # local branch: y_out = x_mid + linear2(gelu(dwconv(linear1(LN2(x_mid)))))
                self._wgrad(g, blk["h3"], L[l_ + ".linear2"])
                dh3 = self._dgrad(g, L[l_ + ".linear2"])
                dh2 = ops.gelu_bwd(dh3, blk["h2"], out=dh3)
                dh1 = ops.dwconv1d_k3_bwd(dh2.view(b, t, -1), blk["h1"].view(b, t, -1), self.fp.V[l_ + ".TC.weight"].p,
                                          self.fp.V[l_ + ".TC.weight"].g, self.fp.V[l_ + ".TC.bias"].g).view(M, -1)
                self._wgrad(dh1, blk["n2"], L[l_ + ".linear1"])
                dn2 = self._dgrad(dh1, L[l_ + ".linear1"])
                self._ln_bwd(dn2, blk["x_mid"], q_ + ".norm2", dx=g, accumulate=True)
                # global branch: x_mid = x_in + proj(attention(LN1(x_in)))
                self._wgrad(g, blk["o"], L[g_ + ".proj"])
                do = self._dgrad(g, L[g_ + ".proj"])
                dq, dkv = self._attention_bwd(do, blk["q"], blk["kv"], blk["P"], b, t, c)
                self._wgrad(dq, blk["n1"], L[g_ + ".q"])
                self._wgrad(dkv, blk["n1"], L[g_ + ".kv"])
                dn1 = self._dgrad(dkv, L[g_ + ".kv"], residual=self._dgrad(dq, L[g_ + ".q"]))
                self._ln_bwd(dn1, blk["x_in"], q_ + ".norm1", dx=g, accumulate=True)
            m = f"TemporalEncoder.Temporal_Merging_Block{s}"
            dpm = self._ln_bwd(g, st["pm"], m + ".norm")
            pc = L[m + ".proj"]
            xin = st["x_in"]
            ops.wgrad_conv1d(dpm.view(b, t, c), xin.view(b, t, -1), pc.gw, batch=b, t=t, taps=3, dil=1, pad=1, accumulate=True, bias_grad=pc.gb)
            gnext = ops.conv_nhwc(dpm.view(b, 1, t, c), pc.wt, None, kh=1, kw=3, pad=(0, 1)).view(M, -1) if s > 1 else None
        return col_loss

    def _col_scale(self, M: int) -> torch.Tensor:
        key = ("cs", M)
        if key not in self._graphs:
            self._graphs[key] = torch.full((self.K,), 1.0 / (M * self.K), dtype=F32, device=self.dev)
        return self._graphs[key]

    @property
    def _pos_w(self):
        if not hasattr(self, "_pw"):
            self._pw = torch.tensor(POS_W[self.loss_type], dtype=F32, device=self.dev) if POS_W[self.loss_type] is not None else None
        return self._pw

    # ------------------------------------------------------------------ one step
    def prepare_labels(self, labels: torch.Tensor) -> torch.Tensor:
        """[B,T,K] multi-hot -> fp32 [B*T,K] on the device (through pinned memory, see tenco_train.prepare_labels)"""
        z = labels.reshape(-1, self.K).to(F32).contiguous()
        return z.pin_memory().to(self.dev, non_blocking=True) if not z.is_cuda else z

    @ops.with_latency_tiles
    def train_step(self, x: torch.Tensor, labels: torch.Tensor, masks: Optional[dict] = None, apply_update: bool = True, use_graph: bool = False):
        """x [B,D,T] as the reference's loader hands it over (`dataloader.py:236-245`) or frame-major [B,T,D] (pass `frame_major=True` via
        x.is_frame_major -- see `train_step_btd`); labels [B,T,K] (or prepared [B*T,K]); masks from `draw_masks` or None.  Returns the loss."""
        return self.train_step_btd(x.permute(0, 2, 1).contiguous(), labels, masks, apply_update, use_graph)

    @ops.with_latency_tiles
    def train_step_btd(self, x_btd: torch.Tensor, labels: torch.Tensor, masks: Optional[dict] = None, apply_update: bool = True,
                       use_graph: bool = False):
        b, t, d = x_btd.shape
        assert d == self.D and x_btd.is_cuda and x_btd.dtype == F32
        z = labels if (labels.dim() == 2 and labels.is_cuda) else self.prepare_labels(labels)
        assert tuple(z.shape) == (b * t, self.K)
        rows = lambda m: m.permute(0, 2, 1).reshape(b * t, -1).contiguous().to(self.dev)     # [B,C,T] -> rows
        masks = masks or {}
        mi = masks["input_rows"] if "input_rows" in masks else rows(masks["input"]) if masks.get("input") is not None else None
        mf = masks["feat_rows"] if "feat_rows" in masks else rows(masks["feat"]) if masks.get("feat") is not None else None
        if use_graph:
            ins = [x_btd, z] + ([mi] if mi is not None else []) + ([mf] if mf is not None else [])

            def fn(xx, zz, *ms):
                ms = list(ms)
                return self._fwd_bwd(xx, zz, ms.pop(0) if mi is not None else None, ms.pop(0) if mf is not None else None)
            col_loss = self._graph_step((b, t, mi is not None, mf is not None), fn, ins)
        else:
            col_loss = self._fwd_bwd(x_btd, z, mi, mf)
        loss = float(col_loss.sum().item()) / (b * t * self.K)
        if apply_update:
            self.apply_update()
        return loss


# ------------------------------------------------------------------------------------------------ Temporal_mstct/run.py -t
def draw_windows(lengths: Dict[str, int], rng, num_clips: int = 256) -> Dict[str, int]:
    """one random `num_clips`-frame window per training video and epoch (`Temporal_mstct/dataloader.py:225-245`: the dataset of a video has
    length 1 in train mode and its item starts at `random.choice(range(0, len - num_clips))`)"""
    return {v: rng.choice(range(0, n - num_clips)) for v, n in lengths.items()}
