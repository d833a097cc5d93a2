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
A frame's logits do not depend on how the video was cut into chunks, nor on eager or replayed execution: bit-identical.

Several videos at once: `StreamBank(model, capacity)` keeps `capacity` such states side by side (rings [capacity, L, C], one counter per slot) and
answers one chunk of EACH open video with the same number of launches, `mt4_tcn_stream_conv_rows_f32`: a launch's rows are described by a table
(`row_table`: which slot, which of its new frames), 32 rows per workgroup row.  A row is computed as its video's solo launch computes it, so a
video's logits are the solo stream's to the bit, whatever shares its launches."""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from . import ops

HEADS = ("ivt", "i", "v", "t")
MAX_CHUNK = ops.STREAM_MAX_CHUNK
MAX_STREAMS = ops.STREAM_MAX_SLOTS


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


def row_table(counts: Dict[int, int], capacity: int) -> Tuple[List[int], List[int], List[int], List[int]]:
    """the tables of one `StreamBank.push`: {slot: new frames} -> (row_slot, row_idx, push_slot, push_count).  Streams in ascending slot order,
    each stream's rows contiguous with idx 0 .. n_s - 1; push_slot / push_count name every stream once (what `ops.tcn_stream_advance_rows` adds).
    Refuses an empty dict, a slot outside 0 .. capacity - 1 and a count outside 1 .. MAX_CHUNK."""
    if not counts:
        raise ValueError("row_table: no stream brings a frame")
    row_slot, row_idx, push_slot, push_count = [], [], [], []
    for slot in sorted(counts):
        n = counts[slot]
        if not (isinstance(slot, int) and 0 <= slot < capacity):
            raise ValueError(f"row_table: slot {slot!r} is not in 0..{capacity - 1}")
        if not (isinstance(n, int) and 1 <= n <= MAX_CHUNK):
            raise ValueError(f"row_table: slot {slot}: {n!r} frames; 1..{MAX_CHUNK} per stream and push")
        row_slot += [slot] * n
        row_idx += list(range(n))
        push_slot.append(slot)
        push_count.append(n)
    return row_slot, row_idx, push_slot, push_count


def _require_streamable(model, who: str) -> None:
    """what the streaming step asks of a head, each refusal with its reason"""
    if not getattr(model, "causal", False):
        raise ValueError(f"{who} needs a causal head (VideoNas(causal=True), --causal): a head that pads symmetrically needs frames that have not arrived")
    if model.hier:
        raise ValueError(f"{who}: --hier pools and resamples over future frames (AvgPool1d(7, 3), linear FPN resampling)")
    if model.dtype != torch.float32:
        raise ValueError(f"{who}: the streaming step (mt4_tcn_stream_conv_f32) is fp32 only; load the head with dtype float32")
    if not model.use_fpn:
        raise ValueError(f"{who} needs --fpn: without it the head has no component logits (network.py:56-66)")
    if not (ops.tcn_supported(model.C, torch.float32) and ops.tcn_supported(model.D, torch.float32)):
        raise ValueError(f"{who}: channel counts {model.D} / {model.C} are not whole 128-byte K-steps (multiples of 32 floats)")
    if not model._p:
        raise RuntimeError("load_state_dict first")


def _heads_gemm(model) -> Tuple[torch.Tensor, torch.Tensor]:
    """the four heads as one [132][C] GEMM (Cout % 4 == 0: one zero row behind the 131) -> (packed weight, bias)"""
    sd, k, dev = model._sd, sum(model.head_sizes), model.device
    w = torch.cat([sd[f"conv_out{s}.weight"] for s in ("", "_i", "_v", "_t")], 0).to(dev).float()
    b = torch.cat([sd[f"conv_out{s}.bias"] for s in ("", "_i", "_v", "_t")], 0).to(dev).float()
    kp = (k + 3) // 4 * 4
    wp = ops.pack_conv_weight(torch.cat([w, w.new_zeros((kp - k,) + tuple(w.shape[1:]))], 0).unsqueeze(2), None, torch.float32)
    return wp, torch.cat([b, b.new_zeros(kp - k)]).contiguous()


def _enqueue_layers(st, x: torch.Tensor, conv) -> None:
    """the conv launches of one push of `st` (a TencoStream or a StreamBank: model, stages, rings, h, top, pl, heads_w, heads_b, logits), x its
    staging buffer; `conv(x, w, b, out, **kw)` is the launch with the chunk's own arguments (the counter and n, or the row table) bound"""
    p = st.model._p
    conv(x, p["PG.conv_1x1.w"], p["PG.conv_1x1.b"], st.rings[0][0], x_ring=False)
    for si, (prefix, nl) in enumerate(st.stages):
        for i in range(nl):
            name, ring = f"{prefix}.layers.{i}", st.rings[si][i]
            conv(ring, p[name + ".conv_dilated.w"], p[name + ".conv_dilated.b"], st.h, taps=3, dilation=2 ** i, relu=True, out_ring=False)
            last = i == nl - 1 and si == len(st.stages) - 1
            nxt = st.top if last else st.rings[si][i + 1] if i < nl - 1 else st.rings[si + 1][0]
            conv(st.h, p[name + ".conv_1x1.w"], p[name + ".conv_1x1.b"], nxt, residual=ring, x_ring=False, out_ring=not last)
    # FPN top-down at equal lengths, in the offline association order (`mt4_fpn_topdown`): p_l = lat(c_l) + p_{l+1}, top first
    cur = st.top
    for j, si in enumerate(range(len(st.stages) - 1, 0, -1)):
        conv(st.rings[si][0], p["fpn.latlayer1.w"], p["fpn.latlayer1.b"], st.pl[j], residual=cur, residual_ring=False, out_ring=False)
        cur = st.pl[j]
    conv(cur, st.heads_w, st.heads_b, st.logits, x_ring=False, out_ring=False)       # the finest level: what predict.py decodes


def _split_heads(model, y: torch.Tensor) -> Dict[str, torch.Tensor]:
    k0, k1, k2, k3 = model.head_sizes
    return {"ivt": y[:, :k0], "i": y[:, k0:k0 + k1], "v": y[:, k0 + k1:k0 + k1 + k2], "t": y[:, k0 + k1 + k2:k0 + k1 + k2 + k3]}


class _StreamState:
    """what a `TencoStream` and a `StreamBank` share: the buffers of a push -- `lead` is the shape ahead of a ring's [L, C], () or (capacity,), and
    `rows` the rows of a plain buffer, MAX_CHUNK or MAX_CHUNK x capacity -- and the capture of its chain as a hipGraph.  A subclass supplies
    `_chain(key, x)`, the launches of one push, and `_capture(key)` around `_capture_chain`."""

    def __init__(self, model, who: str, use_graph: bool, lead: Tuple[int, ...], rows: int):
        _require_streamable(model, who)
        self.model, self.use_graph = model, bool(use_graph)
        dev, C = model.device, model.C
        self.stages = [("PG", model.num_layers_PG)] + [(f"Rs.{r}", model.num_layers_R) for r in range(model.num_R)]
        # one input ring per layer; rings[si][0] is stage si's input = level c_si of the FPN for si >= 1
        self.rings = [[torch.zeros(lead + (ring_rows(2 ** i), C), device=dev) for i in range(n)] for _, n in self.stages]
        self.staging = torch.zeros((rows, model.D), device=dev)
        self.h = torch.zeros((rows, C), device=dev)                      # a layer's hidden map (dilated conv + ReLU)
        self.top = torch.zeros((rows, C), device=dev)                    # the last stage's output: p4
        self.pl = [torch.zeros((rows, C), device=dev) for _ in range(max(1, model.num_R))]   # p3, p2, p1
        self.heads_w, self.heads_b = _heads_gemm(model)
        self.logits = torch.zeros((rows, self.heads_b.numel()), device=dev)
        self._graphs: Dict[int, "torch.cuda.CUDAGraph"] = {}

    def ring_bytes(self) -> int:
        """the rings' reservation (a bank's: capacity x a solo stream's)"""
        return sum(r.numel() * 4 for st in self.rings for r in st)

    def _graph(self, key: int) -> "torch.cuda.CUDAGraph":
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = self._capture(key)
        return g

    def _capture_chain(self, key: int) -> "torch.cuda.CUDAGraph":
        """`_chain(key, staging)` as one hipGraph (the pattern of `graph.GraphedForward`; here the static input is the staging buffer itself and
        the frame counters are graph state on the device, as {seed, step} is an input of `tenco_train`'s graphs).  The chain runs twice: the
        warm-up and the capture"""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):               # warm-up on a side stream (lazy module loading must not happen inside a capture)
            self._chain(key, self.staging)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._chain(key, self.staging)
        return g


class TencoStream(_StreamState):
    """model: a loaded `temporal_tenco.VideoNas(causal=True)` with --fpn, fp32, not --hier.  use_graph: replay one hipGraph per chunk size."""

    def __init__(self, model, use_graph: bool = True):
        super().__init__(model, "TencoStream", use_graph, (), MAX_CHUNK)
        self.counter = torch.zeros(1, dtype=torch.int64, device=model.device)
        self._seen = 0

    # ------------------------------------------------------------------ state
    @property
    def frames_seen(self) -> int:
        return self._seen

    def reset(self) -> None:
        """a new video: the counter back to 0 -- whatever the rings hold lies behind frame 0 and is never read"""
        self.counter.zero_()
        self._seen = 0

    # ------------------------------------------------------------------ one chunk
    def _chain(self, n: int, x: torch.Tensor) -> torch.Tensor:
        """enqueue the launches of one chunk of n frames (x: the staging buffer); -> the [32, 132] logits buffer"""
        t0 = self.counter
        _enqueue_layers(self, x, lambda a, w, b, out, **kw: ops.tcn_stream_conv(a, w, b, out, t0, n=n, **kw))
        ops.tcn_stream_advance(t0, n)
        return self.logits

    def _capture(self, n: int) -> "torch.cuda.CUDAGraph":
        """the chain of a chunk of n frames as one hipGraph.  The warm-up run advances the counter, which is put back behind it; the rows it
        wrote belong to frames >= the counter, and the replay rewrites them before anything reads them."""
        keep = self.counter.clone()
        g = self._capture_chain(n)
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
            self._graph(n).replay()
            out = self.logits
        self._seen += n
        return _split_heads(self.model, out[:n].clone())


class StreamBank(_StreamState):
    """`capacity` (1..64) causal streams side by side, pushed together: model as for `TencoStream`.  `open()` hands out a slot, `push({slot:
    features[n_s, D]})` answers the n_s newest frames of every slot given, `close(slot)` frees it.  use_graph: replay one hipGraph per number of
    32-row blocks (the row count inside the last block is a device word, so differing per-stream counts share a graph)."""

    def __init__(self, model, capacity: int, use_graph: bool = True):
        if not 1 <= int(capacity) <= MAX_STREAMS:
            raise ValueError(f"StreamBank: capacity {capacity}; 1..{MAX_STREAMS} streams")
        self.capacity = cap = int(capacity)
        rows = MAX_CHUNK * cap
        super().__init__(model, "StreamBank", use_graph, (cap,), rows)       # TencoStream's buffers, one ring slice per slot
        dev = model.device
        self.counters = torch.zeros(cap, dtype=torch.int64, device=dev)
        # the tables of a push, one buffer on either side: [n_rows, n_push, 0, 0 | push_slot | push_count | row_slot | row_idx]
        self._host = torch.zeros(4 + 2 * cap + 2 * rows, dtype=torch.int32).pin_memory()
        self._host_np = self._host.numpy()                               # (the same pinned bytes)
        self._dev = torch.zeros(self._host.numel(), dtype=torch.int32, device=dev)
        at = [4, 4 + cap, 4 + 2 * cap, 4 + 2 * cap + rows, 4 + 2 * cap + 2 * rows]
        self._n_rows, self._n_push = self._dev[0:1], self._dev[1:2]
        self._push_slot, self._push_count, self._row_slot, self._row_idx = (self._dev[a:b] for a, b in zip(at[:-1], at[1:]))
        self._at = at
        self._uploaded = torch.cuda.Event()
        self._seen: List[int] = [-1] * cap                               # frames pushed per slot; -1: the slot is free

    # ------------------------------------------------------------------ state
    def open(self) -> int:
        """the lowest free slot, its counter at 0 -- whatever its rings hold lies behind frame 0 and is never read"""
        free = [s for s, n in enumerate(self._seen) if n < 0]
        if not free:
            raise RuntimeError(f"StreamBank: all {self.capacity} slots are open")
        self.counters[free[0]:free[0] + 1].zero_()
        self._seen[free[0]] = 0
        return free[0]

    def _need_open(self, slot) -> None:
        if not (isinstance(slot, int) and 0 <= slot < self.capacity and self._seen[slot] >= 0):
            raise ValueError(f"StreamBank: slot {slot!r} is not open")

    def close(self, slot: int) -> None:
        self._need_open(slot)
        self._seen[slot] = -1

    def frames_seen(self, slot: int) -> int:
        self._need_open(slot)
        return self._seen[slot]

    # ------------------------------------------------------------------ one push
    def _chain(self, max_rows: int, x: torch.Tensor) -> torch.Tensor:
        """enqueue the launches of one push of up to max_rows rows (x: the staging buffer); -> the logits buffer"""
        tab = (self._row_slot, self._row_idx, self._n_rows, self.counters)
        _enqueue_layers(self, x, lambda a, w, b, out, **kw: ops.tcn_stream_conv_rows(a, w, b, out, *tab, max_rows=max_rows, **kw))
        ops.tcn_stream_advance_rows(self.counters, self._push_slot, self._push_count, self._n_push)
        return self.logits

    def _capture(self, max_rows: int) -> "torch.cuda.CUDAGraph":
        """as `TencoStream._capture`, with the device row count and push count at 0 for the warm-up: every workgroup returns and no counter
        moves, so nothing has to be put back"""
        self._dev[0:2].zero_()
        return self._capture_chain(max_rows)

    def push_rows(self, counts: Dict[int, int], features: torch.Tensor) -> Dict[str, torch.Tensor]:
        """`push` for features that already lie in one tensor: features fp32 [sum of counts, D], the streams in ascending slot order, each
        stream's n_s frames contiguous (the order of `row_table`) -> {head: fp32 [sum of counts, K]} in the same row order"""
        for slot in counts:
            self._need_open(slot)
        row_slot, row_idx, push_slot, push_count = row_table(counts, self.capacity)
        n = len(row_slot)
        assert features.shape == (n, self.model.D) and features.dtype == torch.float32 and features.is_cuda
        max_rows = (n + MAX_CHUNK - 1) // MAX_CHUNK * MAX_CHUNK
        g = self._graph(max_rows) if self.use_graph else None
        self._uploaded.synchronize()                                     # the last push's upload has left the pinned buffer
        h, at = self._host_np, self._at
        h[0], h[1] = n, len(push_slot)
        h[at[0]:at[0] + len(push_slot)], h[at[1]:at[1] + len(push_slot)] = push_slot, push_count
        h[at[2]:at[2] + n], h[at[3]:at[3] + n] = row_slot, row_idx
        self._dev.copy_(self._host, non_blocking=True)
        self._uploaded.record()
        self.staging[:n].copy_(features, non_blocking=True)
        if g is None:
            self._chain(max_rows, self.staging)
        else:
            g.replay()
        for slot, c in zip(push_slot, push_count):
            self._seen[slot] += c
        return _split_heads(self.model, self.logits[:n].clone())

    def push(self, features: Dict[int, torch.Tensor]) -> Dict[int, Dict[str, torch.Tensor]]:
        """{slot: fp32 [n_s, D] on the device, 1 <= n_s <= 32}: the next n_s frames of every slot given (each open; open slots that are absent
        keep their rings and counters) -> {slot: {head: fp32 [n_s, K]}} logits of those frames"""
        slots = sorted(features)
        for s in slots:
            self._need_open(s)
            f = features[s]
            assert f.dim() == 2 and f.shape[1] == self.model.D and f.dtype == torch.float32 and f.is_cuda
            if not 1 <= f.shape[0] <= MAX_CHUNK:
                raise ValueError(f"push: slot {s}: {f.shape[0]} frames; 1..{MAX_CHUNK} per stream and push")
        if not slots:
            raise ValueError("push: no stream brings a frame")
        counts = {s: int(features[s].shape[0]) for s in slots}
        out = self.push_rows(counts, features[slots[0]] if len(slots) == 1 else torch.cat([features[s] for s in slots]))
        res, at = {}, 0
        for s in slots:
            res[s] = {hd: y[at:at + counts[s]] for hd, y in out.items()}
            at += counts[s]
        return res
