"""The host-side core of the four trainers: every trained tensor in ONE flat fp32 parameter buffer P and ONE flat gradient buffer G (packed
GEMM layouts, every slot padded to 4 floats), the weight copies derived from the masters by one launch, and the data-parallel exchange of G
-- per-bucket all-reduces behind the backward or one flat all-reduce after it -- ahead of one `mt4_sgd_step_f32`, or, with a gradient-norm clip or
the non-finite guard on, of the guarded update (norm and decisions taken on the device: `mt4_grad_norm_parts_f32`, `mt4_grad_guard_finalize`,
`mt4_sgd_step_guarded_f32`), or, with momentum or AdamW (`Optim`), of the update that also carries flat state buffers of P's layout
(`mt4_sgd_momentum_step_f32`, `mt4_optim_advance` + `mt4_adamw_step_f32`).  With a weight average (`Ema`) the update is followed by
`mt4_ema_advance` + `mt4_ema_step_f32` on one more flat buffer of P's layout.

* `FlatParams` lays the slots out in the order they are declared, loads them from the reference state dict and exports P or G back in the
  reference's key names and shapes;
* `FlatTrainer` is the trainers' base: the buffers, SGD, the exchange and the hipGraph capture of a step's device part;
* `GemmTrainer` adds the bf16 operand copies and the LayerNorm helpers of the nn.Linear-built trainers (MS-TCT, Swin + Q2L).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import torch

from . import ops

F32 = torch.float32


def _r4(n: int) -> int:
    return (n + 3) // 4 * 4


class Optim(NamedTuple):
    """the update rule of a `FlatTrainer` (--optimizer, --momentum, --nesterov, --adam_betas, --adam_eps).  The default is plain SGD, the
    reference's effective rule: no state, the existing update launches"""
    kind: str = "sgd"
    momentum: float = 0.0
    nesterov: bool = False
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8

    @property
    def stateful(self) -> bool:
        return self.kind == "adamw" or self.momentum > 0

    @property
    def buffers(self) -> tuple:
        """the flat state buffers by the key torch.optim gives them"""
        return ("exp_avg", "exp_avg_sq") if self.kind == "adamw" else ("momentum_buffer",) if self.momentum > 0 else ()

    def config(self) -> dict:
        """what is written beside a checkpoint and compared on --resume: the fields the rule reads"""
        if self.kind == "adamw":
            return {"kind": "adamw", "beta1": float(self.beta1), "beta2": float(self.beta2), "eps": float(self.eps)}
        return {"kind": "sgd", "momentum": float(self.momentum), "nesterov": bool(self.nesterov)}

    def check(self) -> "Optim":
        if self.kind not in ("sgd", "adamw"):
            raise ValueError(f"optimizer {self.kind!r}: sgd | adamw")
        if self.kind == "adamw":
            if self.momentum != 0 or self.nesterov:
                raise ValueError("momentum / nesterov belong to sgd: adamw has its betas")
            if not (0 <= self.beta1 < 1 and 0 <= self.beta2 < 1):
                raise ValueError(f"adamw betas ({self.beta1}, {self.beta2}): each in [0, 1)")
            if not self.eps > 0:
                raise ValueError(f"adamw eps {self.eps}: positive")
        else:
            if not 0 <= self.momentum < 1:
                raise ValueError(f"momentum {self.momentum}: in [0, 1)")
            if self.nesterov and self.momentum == 0:
                raise ValueError("nesterov needs a momentum > 0")
        return self


class Ema(NamedTuple):
    """the weight average of a `FlatTrainer` (--ema_decay, --ema_warmup): E <- d E + (1 - d) P behind every applied update, d = `decay`, or with
    `warmup` min(decay, (1 + t) / (10 + t)) at the t-th averaged step.  The default is off: no buffer, no record, no launch"""
    decay: float = 0.0
    warmup: bool = False

    @property
    def active(self) -> bool:
        return self.decay > 0

    def config(self) -> dict:
        """what is written beside a checkpoint and compared on --resume"""
        return {"decay": float(self.decay), "warmup": bool(self.warmup)}

    def check(self) -> "Ema":
        if not 0 <= self.decay < 1:                          # (a NaN fails both comparisons)
            raise ValueError(f"ema decay {self.decay}: in [0, 1)")
        if self.warmup and not self.decay > 0:
            raise ValueError("ema warmup needs a decay > 0")
        return self


class Lin:
    """a packed GEMM / conv weight [cout][kpad] (kernel kh x taps; cout padded to 4, the padding rows zero) and its bias, with gradient views;
    `wt` = the transposed, tap-reversed copy of the data gradient, `w16` / `wt16` = bf16 copies of both (bf16-operand mode)"""
    __slots__ = ("name", "wkey", "bkey", "cout", "cout_real", "cin", "kh", "taps", "dgrad", "off", "src", "ref", "w", "b", "gw", "gb",
                 "wt", "w16", "wt16")


class Vec:
    """a plain vector (LayerNorm / BatchNorm affine, tables) viewed as `shape`; `ref` = its shape in the reference state dict"""
    __slots__ = ("key", "shape", "off", "ref", "p", "g")


class FlatParams:
    """the flat buffers P / G.  Declare the slots (`lin`, `vec`, `reserve`; `bucket` names the gradient bucket the following slots fall into),
    then `build` allocates, loads and registers the derived copies"""

    def __init__(self, device, op16: bool = False):
        self.dev, self.op16 = device, op16
        self.tab = ops.RefreshTable(device)          # every derived matrix (transposed fp32, bf16 copies) from one launch per refresh
        self.L: Dict[str, Lin] = {}
        self.V: Dict[str, Vec] = {}
        self.ranges: Dict[str, list] = {}            # flat range [a, b) of every gradient bucket
        self.S: Dict[str, torch.Tensor] = {}         # optimizer state buffers by name: flat fp32 of P's length and layout (`FlatTrainer`)
        self._slots: list = []
        self._n = 0
        self._bucket = None

    def _take(self, n: int) -> int:
        off = self._n
        self._n += _r4(n)
        if self._bucket is not None:
            self.ranges[self._bucket][1] = self._n
        return off

    def bucket(self, name: str):
        """the slots declared from here on belong to the gradient bucket `name` (continued if it is the current one)"""
        self._bucket = name
        self.ranges.setdefault(name, [self._n, self._n])

    def lin(self, name, cout, cin, taps=1, kh=1, wkey=None, bkey=None, bias=True, dgrad=True, src=None) -> Lin:
        """reference keys default to name + '.weight' / '.bias'; src = (weight, bias) loaded instead of the state dict's tensors (a slot that
        is not one reference tensor); dgrad False: no transposed copy (nothing needs the layer's data gradient)"""
        l = Lin()
        l.name, l.cout_real, l.cout, l.cin, l.kh, l.taps, l.dgrad, l.src = name, cout, _r4(cout), cin, kh, taps, dgrad, src
        l.wkey = wkey or name + ".weight"
        l.bkey = (bkey or name + ".bias") if bias else None
        l.off = self._take(l.cout * ops.packed_k(cin, kh, taps, F32))
        if bias:
            self._take(l.cout)
        self.L[name] = l
        self._slots.append(l)
        return l

    def vec(self, key, shape) -> Vec:
        v = Vec()
        v.key, v.shape = key, tuple(shape)
        v.off = self._take(int(torch.tensor(v.shape).prod()))
        self.V[key] = v
        self._slots.append(v)
        return v

    def reserve(self, n: int):
        """n unused floats (a slot the layout keeps)"""
        self._take(n)

    def build(self, sd: Dict[str, torch.Tensor], derive: bool = True):
        """allocate P / G, cut every slot's views, load it; derive: register the transposed / bf16 copies of every GEMM weight"""
        self.P = torch.zeros(self._n, dtype=F32, device=self.dev)
        self.G = torch.zeros(self._n, dtype=F32, device=self.dev)
        for s in self._slots:
            if isinstance(s, Vec):
                n = int(torch.tensor(s.shape).prod())
                s.p, s.g = self.P[s.off:s.off + n].view(*s.shape), self.G[s.off:s.off + n].view(*s.shape)
                src = sd[s.key]
                s.ref = tuple(src.shape)
                s.p.copy_(src.float().reshape(s.shape).to(self.dev))
                continue
            l, kp = s, ops.packed_k(s.cin, s.kh, s.taps, F32)
            a, n = l.off, l.cout * kp
            l.w, l.gw = self.P[a:a + n].view(l.cout, kp), self.G[a:a + n].view(l.cout, kp)
            l.b, l.gb = (self.P[a + n:a + n + l.cout], self.G[a + n:a + n + l.cout]) if l.bkey else (None, None)
            w, b = l.src if l.src is not None else (sd[l.wkey], sd[l.bkey] if l.bkey else None)
            l.src, l.ref = None, tuple(w.shape)
            w = w.float().reshape(l.cout_real, l.cin, l.kh, l.taps)
            if l.cout != l.cout_real:
                w = torch.cat([w, torch.zeros((l.cout - l.cout_real,) + tuple(w.shape[1:]))], 0)
            l.w.copy_(ops.pack_conv_weight(w.to(self.dev), None, F32))
            if b is not None:
                l.b[:l.cout_real].copy_(b.float().to(self.dev))
            if derive:
                self._derive(l, l.dgrad)
        return self

    def _derive(self, l: Lin, need_dgrad: bool):
        """the matrices the kernels read besides the master weight: the transposed (tap-reversed) copy of the data gradient (fp32) and, in the
        bf16-operand mode, bf16 copies of both for the single-tap GEMMs whose channel counts allow it"""
        l.wt = self.tab.add(l.w, l.cout, l.cin, F32, True, [l.taps - 1 - i for i in range(l.taps)]) if need_dgrad else None
        l.w16 = l.wt16 = None
        if self.op16 and l.taps == 1 and l.cin % 8 == 0 and l.cout % 8 == 0 and l.cout >= 64:
            l.w16 = self.tab.add(l.w, l.cout, l.cin, torch.bfloat16, False, [0])
            if need_dgrad:
                l.wt16 = self.tab.add(l.w, l.cout, l.cin, torch.bfloat16, True, [0])

    def rows(self, name: str, lo: int, hi: int) -> Lin:
        """a row slice of a packed weight (nn.MultiheadAttention's in_proj split into q / k / v) with its own derived copies"""
        src = self.L[name]
        l = Lin()
        l.name, l.cout, l.cin, l.taps = f"{name}[{lo}:{hi}]", hi - lo, src.cin, 1
        l.w, l.gw, l.b, l.gb = src.w[lo:hi], src.gw[lo:hi], src.b[lo:hi], src.gb[lo:hi]
        self._derive(l, True)
        return l

    def keys(self) -> set:
        """the reference keys the slots hold"""
        return {k for s in self._slots for k in ((s.key,) if isinstance(s, Vec) else (s.wkey, s.bkey)) if k}

    def export(self, which) -> Dict[str, torch.Tensor]:
        """P ('p'), G ('g'), a named state buffer of `S`, or any flat tensor of P's length (a buffer of flat indices gives the map back into the
        flat layout) in the reference's key names and shapes, on the CPU"""
        buf = which if isinstance(which, torch.Tensor) else self.P if which == "p" else self.G if which == "g" else self.S[which]
        assert buf.numel() == self._n and buf.is_contiguous()
        out = {}
        for s in self._slots:
            if isinstance(s, Vec):
                n = int(torch.tensor(s.shape).prod())
                out[s.key] = buf[s.off:s.off + n].reshape(s.ref).clone().cpu()
                continue
            kp = ops.packed_k(s.cin, s.kh, s.taps, F32)
            n = s.cout * kp
            w = buf[s.off:s.off + n].view(s.cout, kp)
            tapw = _r4(s.cin)
            w = w[:s.cout_real, :s.kh * s.taps * tapw].reshape(s.cout_real, s.kh, s.taps, tapw)[..., :s.cin].permute(0, 3, 1, 2)
            out[s.wkey] = w.reshape(s.ref).contiguous().cpu()
            if s.bkey:
                out[s.bkey] = buf[s.off + n:s.off + n + s.cout_real].clone().cpu()
        return out


def allreduce_sum_flat(flat_grad: torch.Tensor, group=None) -> float:
    """The ONE exchange of a data-parallel step: sum the flat gradient buffer over ranks in place (RCCL on the GPU,
    gloo in the CPU tests) and return the factor that turns the sum into the mean (1/world).  No-op for one rank."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return 1.0
    dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM, group=group)
    return 1.0 / dist.get_world_size(group)


class FlatTrainer:
    """the trainers' base: `fp` (a built `FlatParams`), SGD (`lr`, `wd`) and the data-parallel exchange of G over `pg`.
    exchange False: rank-local steps (bench: the step without its exchange).  overlap: the backward calls `_reduce_bucket` where a gradient
    bucket is complete and the bucket's all-reduce runs behind the backward of the earlier layers; otherwise `apply_update`
    all-reduces the whole of G once."""

    def __init__(self, lr: float, weight_decay: float, device, process_group, overlap: bool = False, clip_grad_norm: float = 0.0,
                 skip_nonfinite: bool = False, optim: Optional[Optim] = None, ema: Optional[Ema] = None):
        """clip_grad_norm > 0: the exchanged gradient is scaled to that global L2 norm when it is longer; skip_nonfinite: a step whose exchanged
        gradient holds a NaN or an Inf changes nothing (`apply_update`, the guarded update).  Both off: the plain `mt4_sgd_step_f32`.
        optim: the update rule (`Optim`); None or the default: plain SGD, today's launches, no state buffer.  With momentum or AdamW the state
        lives in flat buffers of P's layout (`fp.S`), allocated by `load_state_dict`; see `apply_update`.
        ema: the weight average (`Ema`); None or the default: none kept, every launch and byte as without it.  Active: `fp.S["ema"]` starts as a
        copy of the loaded P and follows every applied update (`_ema_update`); `ema_state_dict()` exports it.  A skipped step (--skip_nonfinite)
        does not enter the average: the count t, E and the averaged running statistics stay as they were.  Without --skip_nonfinite a non-finite
        parameter poisons the average for good, as it does the optimizer state."""
        if not clip_grad_norm >= 0:
            raise ValueError(f"clip_grad_norm {clip_grad_norm}: 0 (off) or a positive norm")
        optim = Optim(*optim).check() if optim is not None else None
        self.optim = optim if optim is not None and optim.stateful else None
        self._ostate = None                         # AdamW: the device step record (mt4_optim_state)
        ema = Ema(*ema).check() if ema is not None else None
        self.ema = ema if ema is not None and ema.active else None
        self._estate = None                         # the average's device record (mt4_ema_state)
        self._omap = None                           # reference key -> flat indices (`load_optimizer_state_dict`)
        self.lr, self.wd = lr, weight_decay
        self.clip_grad_norm, self.skip_nonfinite = float(clip_grad_norm), bool(skip_nonfinite)
        self._guard = None                          # (workspace, state, stats) of the guarded update, allocated at its first use
        self.dev, self.pg = torch.device(device), process_group
        self.exchange = True
        self.overlap = overlap
        self.bucket_order: List[str] = []           # gradient buckets in the order their all-reduce was issued this step
        self._pending: list = []
        self._capturing = False
        self._cut = None
        self._graphs: Dict[tuple, object] = {}
        self.graph_reserved_bytes = 0               # what the captures added to the allocator's reserved memory (their private pools)

    @property
    def P(self) -> torch.Tensor:
        return self.fp.P

    @property
    def G(self) -> torch.Tensor:
        return self.fp.G

    def _refresh(self):
        """derived copies after a parameter change"""
        self.fp.tab.run()

    def _ddp_world(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size(self.pg) if (dist.is_available() and dist.is_initialized()) else 1

    def _reduce_bucket(self, name: str):
        """the bucket's gradients are complete: enqueue its all-reduce behind the kernels that wrote it (`apply_update` waits for all of them).
        Under a segmented capture the graph is cut here instead and the all-reduce is issued at replay."""
        if self._capturing:
            if self._cut is not None:
                self._cut(name)
            return
        if self.overlap and self.exchange and self._ddp_world() > 1:
            self._issue_bucket(name)

    def _issue_bucket(self, name: str):
        import torch.distributed as dist
        a, b = self.fp.ranges[name]
        self.bucket_order.append(name)
        if b > a:
            self._pending.append(dist.all_reduce(self.G[a:b], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))

    def _graph_step(self, key, fn, inputs: List[torch.Tensor]):
        """`fn(*inputs)` (a step's device part) replayed from the hipGraph captured for `key` on first use.  Data-parallel steps with bucket
        overlap are captured in segments cut at `_reduce_bucket`, a bucket's all-reduce issued between two replays (`graph.SegmentedGraph`);
        otherwise one graph, one flat all-reduce behind it."""
        seg = self._segmented()
        g = self._graphs.get((key, seg))
        if g is None:
            before = torch.cuda.memory_reserved(self.dev)
            g = self._graphs[(key, seg)] = self._capture(fn, inputs, seg)
            self.graph_reserved_bytes += max(0, torch.cuda.memory_reserved(self.dev) - before)
        return g(*inputs, on_cut=self._issue_bucket) if seg else g(*inputs)

    def _segmented(self) -> bool:
        return bool(self.overlap and self.exchange and self._ddp_world() > 1)

    def _capture(self, fn, inputs: List[torch.Tensor], seg: bool):
        from .graph import GraphedForward, SegmentedGraph
        self._capturing = True
        try:
            if not seg:
                return GraphedForward(fn, inputs)

            def fn_cut(cut, *a):
                self._cut = cut
                try:
                    return fn(*a)
                finally:
                    self._cut = None
            return SegmentedGraph(fn_cut, inputs)
        finally:
            self._capturing = False

    def apply_update(self):
        """DDP exchange (mean over ranks) + SGD + refresh of the derived copies"""
        if self._pending:                                   # buckets were reduced during the backward
            for h in self._pending:
                h.wait()
            self._pending = []
            scale = 1.0 / self._ddp_world()
        else:
            scale = allreduce_sum_flat(self.G, self.pg) if self.exchange else 1.0
        if self.optim is not None:
            self._stateful_update(scale)
            return
        if not self.guarded:
            ops.sgd_step(self.P, self.G, self.lr, self.wd, scale)
            self._ema_update(None)
            self._refresh()
            return
        # the guarded update: norm and decisions from the fully exchanged G -- the same on every rank (NaN and Inf survive a sum), so all ranks clip
        # and skip alike without another collective -- taken on the device and read there by the update; no copy to the host
        ws, state, stats = self._guard_buffers()
        ops.grad_guard(self.G, scale, self.clip_grad_norm, self.skip_nonfinite, ws, state, stats)
        ops.sgd_step_guarded(self.P, self.G, self.lr, self.wd, scale, state)
        self._restore_skipped(state)
        self._ema_update(state)
        self._refresh()

    @property
    def guarded(self) -> bool:
        return self.clip_grad_norm > 0 or self.skip_nonfinite

    def _guard_buffers(self):
        if self._guard is None or self._guard[0].shape[0] != ops.grad_norm_plan(self.G.numel()).nparts or self._guard[0].device != self.G.device:
            self._guard = ops.guard_buffers(self.G.numel(), self.G.device)
        return self._guard

    def _restore_skipped(self, state: torch.Tensor):
        """buffers besides P that a skipped step must leave as they were (the student's BatchNorm running statistics)"""

    # ------------------------------------------------------------------ optimizer state
    def _stateful_update(self, scale: float):
        """the update with momentum or AdamW: the guard pass as in the plain path when guarded, `mt4_optim_advance` for AdamW, ONE update launch
        that reads the guard record on the device.  The clip coefficient scales the gradient before it enters the state (torch clips ahead of
        `step()`); a skipped step leaves P, the state buffers and the step count as they were.  Every rank updates from the same exchanged G,
        so the state is the same on every rank and is never exchanged."""
        o, S = self.optim, self.fp.S
        state = None
        if self.guarded:
            ws, state, stats = self._guard_buffers()
            ops.grad_guard(self.G, scale, self.clip_grad_norm, self.skip_nonfinite, ws, state, stats)
        if o.kind == "adamw":
            ops.optim_advance(self._ostate, o.beta1, o.beta2, state)
            ops.adamw_step(self.P, self.G, S["exp_avg"], S["exp_avg_sq"], self.lr, self.wd, scale, o.beta1, o.beta2, o.eps, self._ostate, state)
        else:
            ops.sgd_momentum_step(self.P, self.G, S["momentum_buffer"], self.lr, self.wd, scale, o.momentum, o.nesterov, state)
        if state is not None:
            self._restore_skipped(state)
        self._ema_update(state)
        self._refresh()

    def _optim_buffers(self):
        """`load_state_dict`, once `fp` is built and before any graph capture: the zero-filled state buffers of the update rule (padding columns
        and reserved slots stay exact zeros, as in G: their gradient and parameter are zero) and a fresh step record.  Nothing for plain SGD.  The
        weight average's buffer and record are allocated at the same point (`_ema_buffers`)."""
        self._omap = None
        self._ema_buffers()
        if self.optim is None:
            return
        for name in self.optim.buffers:
            self.fp.S[name] = torch.zeros_like(self.fp.P)
        if self.optim.kind == "adamw":
            self._ostate = ops.optim_state_buffer(self.dev)

    # ------------------------------------------------------------------ weight average
    def _ema_update(self, state: Optional[torch.Tensor]):
        """behind the parameter update and `_restore_skipped` of every `apply_update` branch: `mt4_ema_advance`, then `mt4_ema_step_f32` on P and on
        the trainer's other averaged buffers (`_ema_step_extra`), all reading the step's guard record `state` on the device where there is one --
        a skipped step leaves t, E and those buffers as they were.  Outside the replayed hipGraphs, so eager and replayed steps give the same
        bits; every rank averages the same P, so E is the same on every rank and is never exchanged.  Nothing without an average."""
        if self.ema is None:
            return
        ops.ema_advance(self._estate, self.ema.decay, self.ema.warmup, state)
        ops.ema_step(self.fp.S["ema"], self.P, self._estate, state)
        self._ema_step_extra(state)

    def _ema_step_extra(self, state: Optional[torch.Tensor]):
        """buffers besides P that are averaged with the same record (the student's BatchNorm running statistics)"""

    def _ema_buffers(self):
        """`load_state_dict`, once the weights are loaded (`_optim_buffers` calls it): E starts as a COPY of P -- padding columns and reserved slots
        stay exact zeros under d 0 + c 0 -- beside a fresh record.  Nothing without an average."""
        self._estate = None
        self.fp.S.pop("ema", None)
        if self.ema is None:
            return
        self.fp.S["ema"] = self.fp.P.clone()
        self._estate = ops.ema_state_buffer(self.dev)

    def ema_config(self) -> Optional[dict]:
        """the average's config as --resume records it; None without one"""
        return self.ema.config() if self.ema is not None else None

    def ema_record(self) -> dict:
        """the average's record on the host: t, decay, comp (one device-to-host copy); {} without an average"""
        return ops.read_ema_state(self._estate) if self._estate is not None else {}

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """the trainer's own `state_dict()` with E in place of P (the student: the averaged running statistics in place of the running ones,
        `num_batches_tracked` the trainer's own integer); parameters the trainer keeps verbatim are unchanged.  Same keys, shapes, dtypes and
        order: what `validate` scores and the best `.pth` holds when the average is on"""
        if self.ema is None:
            raise ValueError("this trainer keeps no weight average (ema=None)")
        return self.state_dict("ema")

    def ema_export(self) -> dict:
        """{"ema": the config, "t": the averaged steps, "state": `ema_state_dict()`} on the CPU: what --resume keeps beside a checkpoint"""
        return {"ema": self.ema_config(), "t": int(self.ema_record()["t"]), "state": self.ema_state_dict()}

    def load_ema_export(self, exp: dict):
        """the inverse of `ema_export`: the tensors go back to their flat places through the map `load_optimizer_state_dict` uses, the record is
        rebuilt by `t` host advances"""
        if self.ema is None:
            raise ValueError("this trainer keeps no weight average (ema=None)")
        if exp.get("ema") != self.ema.config():
            raise ValueError(f"weight average of {exp.get('ema')} does not belong to this trainer's {self.ema.config()}")
        state, omap = exp["state"], self._flat_map()
        if set(state) != set(self.state_dict()):
            raise ValueError("weight average holds other tensors than this trainer's state dict")
        flat = torch.zeros(self.fp.P.numel(), dtype=F32)
        for k, idx in omap.items():
            if tuple(state[k].shape) != tuple(idx.shape):
                raise ValueError(f"weight average {k}: shape {tuple(state[k].shape)}, expected {tuple(idx.shape)}")
            flat[idx.reshape(-1).long()] = state[k].reshape(-1).to(F32)
        self.fp.S["ema"].copy_(flat.to(self.dev))
        self._load_ema_extra(state)
        rec = {"t": 0, "decay": 0.0, "comp": 1.0}
        for _ in range(int(exp["t"])):
            rec = ops.ema_advance_host(rec, self.ema.decay, self.ema.warmup)
        ops.write_ema_state(self._estate, rec["t"], rec["decay"], rec["comp"])

    def _load_ema_extra(self, state: Dict[str, torch.Tensor]):
        """the averaged buffers besides E out of a loaded `ema_state_dict()`"""

    def _flat_map(self) -> Dict[str, torch.Tensor]:
        """reference key -> the flat indices of its elements (found by exporting a buffer of flat indices, so every packing and head fusion of the
        export is inverted by construction)"""
        if self._omap is None:
            n = self.fp.P.numel()
            self._omap = self._export_any(torch.arange(n, dtype=torch.int32 if n < 2 ** 31 else torch.int64, device=self.dev))
        return self._omap

    def _export_any(self, which) -> Dict[str, torch.Tensor]:
        """`fp.export` through the trainer's own `_export` where it has one (fused heads cut back into the reference's tensors)"""
        return (getattr(self, "_export", None) or self.fp.export)(which)

    def optim_config(self) -> Optional[dict]:
        """the rule's config as --resume records it; None for plain SGD"""
        return self.optim.config() if self.optim is not None else None

    def optim_record(self) -> dict:
        """the step record on the host: t, beta1_pow, beta2_pow (AdamW; one device-to-host copy) or {} where the rule keeps none"""
        return ops.read_optim_state(self._ostate) if self._ostate is not None else {}

    def optimizer_state_dict(self) -> Optional[dict]:
        """{"optim": the rule's config, "step": AdamW's step count (0 for SGD), "state": {reference parameter name: {"momentum_buffer"} |
        {"exp_avg", "exp_avg_sq"}}} on the CPU, in the names and shapes of `grads()` -- what the matching torch.optim object holds per
        parameter.  None for plain SGD."""
        if self.optim is None:
            return None
        bufs = {name: self._export_any(name) for name in self.optim.buffers}
        keys = next(iter(bufs.values())).keys()
        return {"optim": self.optim.config(), "step": int(self.optim_record().get("t", 0)),
                "state": {k: {name: bufs[name][k] for name in self.optim.buffers} for k in keys}}

    def load_optimizer_state_dict(self, osd: dict):
        """the inverse of `optimizer_state_dict`: the tensors go back to their flat places (found by exporting a buffer of flat indices, so every
        packing and head fusion of the export is inverted by construction), the step record is rebuilt by `step` double multiplies"""
        if self.optim is None:
            raise ValueError("this trainer keeps no optimizer state (plain SGD)")
        if osd.get("optim") != self.optim.config():
            raise ValueError(f"optimizer state of {osd.get('optim')} does not belong to this trainer's {self.optim.config()}")
        omap = self._flat_map()
        if set(osd["state"]) != set(omap):
            raise ValueError("optimizer state holds other parameters than this trainer's")
        for name in self.optim.buffers:
            flat = torch.zeros(self.fp.P.numel(), dtype=F32)
            for k, idx in omap.items():
                t = osd["state"][k][name]
                if tuple(t.shape) != tuple(idx.shape):
                    raise ValueError(f"optimizer state {k}.{name}: shape {tuple(t.shape)}, expected {tuple(idx.shape)}")
                flat[idx.reshape(-1).long()] = t.reshape(-1).to(F32)
            self.fp.S[name].copy_(flat.to(self.dev))
        if self._ostate is not None:
            rec = {"t": 0, "beta1_pow": 1.0, "beta2_pow": 1.0}
            for _ in range(int(osd["step"])):
                rec = ops.optim_advance_host(rec, self.optim.beta1, self.optim.beta2)
            ops.write_optim_state(self._ostate, rec["t"], rec["beta1_pow"], rec["beta2_pow"])

    def guard_state(self) -> dict:
        """what the last guarded update decided: sumsq, norm, coef, skip, nonfinite (one device-to-host copy)"""
        return ops.read_guard_state(self._guard_buffers()[1])

    def guard_stats(self, reset: bool = False) -> dict:
        """the guarded updates since the last reset: steps, skipped, clipped, norm_sum / norm_max / norm_mean over the steps not skipped (one
        device-to-host copy)"""
        stats = self._guard_buffers()[2]
        out = ops.read_guard_stats(stats)
        applied = out["steps"] - out["skipped"]
        out["norm_mean"] = out["norm_sum"] / applied if applied else 0.0
        if reset:
            stats.zero_()
        return out


class GemmTrainer(FlatTrainer):
    """trainers built from nn.Linear GEMMs on rows whose bf16-operand mode reads bf16 copies of the operands (`Lin.w16`), and LayerNorms"""

    def _begin_step(self):
        """every parameter gradient of a step ADDS into G; the operand copies of the previous step are dropped"""
        self.G.zero_()
        self._c16: Dict[tuple, tuple] = {}
        self._dy16 = None

    def _cast(self, x2d, grad=False):
        """bf16 copy of a GEMM operand.  Forward activations: made once per step and kept with their source (the copy also serves the weight
        gradient; holding the source keeps the allocator from handing its address to another tensor).  Gradients are short-lived: only the
        latest one is remembered (a layer's data and weight gradient ask for the same tensor back to back)."""
        key = (x2d.data_ptr(), tuple(x2d.shape))
        if grad:
            if self._dy16 is not None and self._dy16[0] == key:
                return self._dy16[2]
            y = ops.cast_bf16(x2d)
            self._dy16 = (key, x2d, y)
            return y
        hit = self._c16.get(key)
        if hit is None:
            hit = self._c16[key] = (x2d, ops.cast_bf16(x2d))
        return hit[1]

    def _fwd(self, x, l: Lin, residual=None, act=None, out_row_map=None):
        if l.w16 is not None:
            x = x if x.is_contiguous() else x.contiguous()
            return ops.linear(self._cast(x), l.w16, l.b, residual=residual, act=act, out_row_map=out_row_map, out_dtype=F32)
        return ops.linear(x, l.w, l.b, residual=residual, act=act, out_row_map=out_row_map)

    def _ln(self, x, key):
        V = self.fp.V
        return ops.layernorm(x, V[key + ".weight"].p, V[key + ".bias"].p)

    def _ln_bwd(self, dy, x, key, dx=None, accumulate=False):
        V = self.fp.V
        return ops.layernorm_bwd(dy, x, V[key + ".weight"].p, V[key + ".weight"].g, V[key + ".bias"].g, dx=dx, accumulate_dx=accumulate)
