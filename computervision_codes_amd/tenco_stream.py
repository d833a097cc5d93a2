"""The causal temporal head frame by frame: `TencoStream(model).push(features[n, D])` answers for the n newest frames from the frames seen so
far, without re-reading the video (no reference counterpart: its `DilatedResidualCausalLayer`, `Temporal_tenco/network.py:165-183`, is used by
nothing, and its only forward is the whole-video one).

State: every DilatedResidualLayer keeps its INPUT in a ring of L rows x C floats, L the power of two >= 2 d + 32 (frame f in row f mod L); a
layer's 1x1 + residual launch writes the next layer's ring, a stage's last layer the next stage's first ring, which is also that level's c_l.
The front padding is the frame counter (`ops.tcn_stream_conv`: a tap at a negative frame reads zeros), so `reset()` is one store.  At the
shipped 11 / 10 / 3 x 512 configuration the rings hold 8384 + 3 x 4288 rows of 2 KB = 41.5 MiB; a frame's answer looks back over
4094 + 3 x 2046 frames (the receptive field of the offline causal forward: both compute the same function).

A push is 1 + 2 x layers + 3 + 1 launches of `mt4_tcn_stream_conv_f32` and one that advances the counter, on one stream, replayed as one
hipGraph per chunk size (captured as `graph.GraphedForward` does; the staging buffer is the graph's input, the counter and the rings its state).
A frame's logits do not depend on how the video was cut into chunks, nor on eager or replayed execution: bit-identical."""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from . import ops

HEADS = ("ivt", "i", "v", "t")
MAX_CHUNK = ops.STREAM_MAX_CHUNK


def ring_rows(d: int, taps: int = 3) -> int:
    """rows of the input ring of a conv with dilation d: the power of two >= (taps - 1) d + MAX_CHUNK (the chunk and the history of its oldest tap)"""
    need, rows = (taps - 1) * d + MAX_CHUNK, 1
    while rows < need:
        rows *= 2
    return rows


def tap_rows(t0: int, n: int, d: int, L: int, taps: int = 3) -> Tuple[List[List[int]], List[int]]:
    """host restatement of the kernel's ring indexing: for a chunk of n frames behind t0 pushed ones -> (reads, writes); reads[i][k] is the ring row
    tap k of chunk row i reads (frame t0 + i - (taps - 1 - k) d), -1 where that frame is negative (padding: zeros); writes[i] the row frame t0 + i
    is stored in.  L: a power of two >= (taps - 1) d + n"""
    assert L > 0 and L & (L - 1) == 0 and L >= (taps - 1) * d + n and 1 <= n <= MAX_CHUNK and t0 >= 0
    reads = [[(f & (L - 1)) if f >= 0 else -1 for f in (t0 + i - (taps - 1 - k) * d for k in range(taps))] for i in range(n)]
    return reads, [(t0 + i) & (L - 1) for i in range(n)]


class TencoStream:
    """model: a loaded `temporal_tenco.VideoNas(causal=True)` with --fpn, fp32, not --hier.  use_graph: replay one hipGraph per chunk size."""

    def __init__(self, model, use_graph: bool = True):
        if not getattr(model, "causal", False):
            raise ValueError("TencoStream needs a causal head (VideoNas(causal=True), --causal): a head that pads symmetrically needs frames that have not arrived")
        if model.hier:
            raise ValueError("TencoStream: --hier pools and resamples over future frames (AvgPool1d(7, 3), linear FPN resampling)")
        if model.dtype != torch.float32:
            raise ValueError("TencoStream: the streaming step (mt4_tcn_stream_conv_f32) is fp32 only; load the head with dtype float32")
        if not model.use_fpn:
            raise ValueError("TencoStream needs --fpn: without it the head has no component logits (network.py:56-66)")
        if not (ops.tcn_supported(model.C, torch.float32) and ops.tcn_supported(model.D, torch.float32)):
            raise ValueError(f"TencoStream: channel counts {model.D} / {model.C} are not whole 128-byte K-steps (multiples of 32 floats)")
        if not model._p:
            raise RuntimeError("load_state_dict first")
        self.model, self.use_graph = model, bool(use_graph)
        dev, C = model.device, model.C
        self.stages = [("PG", model.num_layers_PG)] + [(f"Rs.{r}", model.num_layers_R) for r in range(model.num_R)]
        # one input ring per layer; rings[si][0] is stage si's input = level c_si of the FPN for si >= 1
        self.rings = [[torch.zeros((ring_rows(2 ** i), C), device=dev) for i in range(n)] for _, n in self.stages]
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.staging = torch.zeros((MAX_CHUNK, model.D), device=dev)
        self.h = torch.zeros((MAX_CHUNK, C), device=dev)                 # a layer's hidden map (dilated conv + ReLU)
        self.top = torch.zeros((MAX_CHUNK, C), device=dev)               # the last stage's output: p4
        self.pl = [torch.zeros((MAX_CHUNK, C), device=dev) for _ in range(max(1, model.num_R))]   # p3, p2, p1
        # the four heads as one [132][C] GEMM (Cout % 4 == 0: one zero row behind the 131)
        sd, k = model._sd, sum(model.head_sizes)
        w = torch.cat([sd[f"conv_out{s}.weight"] for s in ("", "_i", "_v", "_t")], 0).to(dev).float()
        b = torch.cat([sd[f"conv_out{s}.bias"] for s in ("", "_i", "_v", "_t")], 0).to(dev).float()
        kp = (k + 3) // 4 * 4
        self.heads_w = ops.pack_conv_weight(torch.cat([w, w.new_zeros((kp - k,) + tuple(w.shape[1:]))], 0).unsqueeze(2), None, torch.float32)
        self.heads_b = torch.cat([b, b.new_zeros(kp - k)]).contiguous()
        self.logits = torch.zeros((MAX_CHUNK, kp), device=dev)
        self._graphs: Dict[int, "torch.cuda.CUDAGraph"] = {}
        self._seen = 0

    # ------------------------------------------------------------------ state
    @property
    def frames_seen(self) -> int:
        return self._seen

    def ring_bytes(self) -> int:
        return sum(r.numel() * 4 for st in self.rings for r in st)

    def reset(self) -> None:
        """a new video: the counter back to 0 -- whatever the rings hold lies behind frame 0 and is never read"""
        self.counter.zero_()
        self._seen = 0

    # ------------------------------------------------------------------ one chunk
    def _chain(self, n: int, x: torch.Tensor) -> torch.Tensor:
        """enqueue the launches of one chunk of n frames (x: the staging buffer); -> the [32, 132] logits buffer"""
        p, t0, conv = self.model._p, self.counter, ops.tcn_stream_conv
        conv(x, p["PG.conv_1x1.w"], p["PG.conv_1x1.b"], self.rings[0][0], t0, n=n, x_ring=False)
        for si, (prefix, nl) in enumerate(self.stages):
            for i in range(nl):
                name, ring = f"{prefix}.layers.{i}", self.rings[si][i]
                conv(ring, p[name + ".conv_dilated.w"], p[name + ".conv_dilated.b"], self.h, t0, n=n, taps=3, dilation=2 ** i, relu=True, out_ring=False)
                last = i == nl - 1 and si == len(self.stages) - 1
                nxt = self.top if last else self.rings[si][i + 1] if i < nl - 1 else self.rings[si + 1][0]
                conv(self.h, p[name + ".conv_1x1.w"], p[name + ".conv_1x1.b"], nxt, t0, n=n, residual=ring, x_ring=False, out_ring=not last)
        # FPN top-down at equal lengths, in the offline association order (`mt4_fpn_topdown`): p_l = lat(c_l) + p_{l+1}, top first
        cur = self.top
        for j, si in enumerate(range(len(self.stages) - 1, 0, -1)):
            conv(self.rings[si][0], p["fpn.latlayer1.w"], p["fpn.latlayer1.b"], self.pl[j], t0, n=n, residual=cur, residual_ring=False, out_ring=False)
            cur = self.pl[j]
        conv(cur, self.heads_w, self.heads_b, self.logits, t0, n=n, x_ring=False, out_ring=False)       # the finest level: what predict.py decodes
        ops.tcn_stream_advance(t0, n)
        return self.logits

    def _capture(self, n: int) -> "torch.cuda.CUDAGraph":
        """the chain of a chunk of n frames as one hipGraph (the pattern of `graph.GraphedForward`; here the static input is the staging buffer
        itself and the frame counter is graph state on the device, as {seed, step} is an input of `tenco_train`'s graphs).  The warm-up run
        advances the counter, which is put back behind it; the rows it wrote belong to frames >= the counter, and the replay rewrites them
        before anything reads them."""
        keep = self.counter.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):               # warm-up on a side stream (lazy module loading must not happen inside a capture)
            self._chain(n, self.staging)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._chain(n, self.staging)
        self.counter.copy_(keep)
        return g

    def push(self, features: torch.Tensor) -> Dict[str, torch.Tensor]:
        """features fp32 [n, D] on the device, 1 <= n <= 32: the next n frames -> {head: fp32 [n, K]} logits of those frames (new tensors)"""
        assert features.dim() == 2 and features.shape[1] == self.model.D and features.dtype == torch.float32 and features.is_cuda
        n = features.shape[0]
        if not 1 <= n <= MAX_CHUNK:
            raise ValueError(f"push: {n} frames; 1..{MAX_CHUNK} per chunk")
        self.staging[:n].copy_(features, non_blocking=True)
        if not self.use_graph:
            out = self._chain(n, self.staging)
        else:
            g = self._graphs.get(n)
            if g is None:
                g = self._graphs[n] = self._capture(n)
            g.replay()
            out = self.logits
        self._seen += n
        y = out[:n].clone()
        k0, k1, k2, k3 = self.model.head_sizes
        return {"ivt": y[:, :k0], "i": y[:, k0:k0 + k1], "v": y[:, k0 + k1:k0 + k1 + k2], "t": y[:, k0 + k1 + k2:k0 + k1 + k2 + k3]}
