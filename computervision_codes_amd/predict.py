"""From a directory of frames to per-frame triplet predictions in one pass (no reference counterpart: its only way there is the
`Spatial_cnn/test.py` -> feature pickle -> `Temporal_tenco/run.py -e` chain, which takes its frame list from the LABEL files and leaves
per-frame predictions as a side effect of the report).  `Predictor` runs PNG decode + Resize (`cholect.load_files_device`), the student in
chunks and the whole-video TCN with the [T, 512] features left in HBM between the two stages, decodes the logits with `ops.topk_rows`
(`mt4_topk_rows_f32`: per-frame top-K triplets, how many are above the threshold, the component heads' picks) and copies the small result
down once per video.  No label file is opened anywhere on this path.  `drivers.predict` is the command line (`MT4MTLKD/predict.py`)."""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence

import numpy as np

from .metrics import _TRIPLETS

HEADS = ("ivt", "i", "v", "t")


def parse_names(path: str) -> List[str]:
    """--names FILE: one line per triplet id, `name` (ids count up from 0) or `id:name`; empty lines are skipped.  -> 100 strings"""
    names: List[Optional[str]] = [None] * len(_TRIPLETS)
    nxt = 0
    with open(path) as f:
        for ln in f:
            ln = ln.strip()
            if not ln:
                continue
            head, sep, rest = ln.partition(":")
            if sep and head.strip().isdigit():
                tid, name = int(head), rest.strip()
            else:
                tid, name = nxt, ln
            if not 0 <= tid < len(names):
                raise ValueError(f"--names {path}: triplet id {tid} is not in 0..{len(names) - 1}")
            names[tid] = name
            nxt = tid + 1
    missing = [i for i, n in enumerate(names) if n is None]
    if missing:
        raise ValueError(f"--names {path}: no name for triplet ids {missing[:5]}{'...' if len(missing) > 5 else ''} (one line per id, {len(names)} ids)")
    return names      # type: ignore


class Prediction:
    """What a video's frames show, on the host (numpy):
      frames        file names, one per frame, in the order they ran
      topk_ids      int32 [T, k]    the k highest triplets of every frame, best first (equal logits: lower id first)
      topk_scores   float32 [T, k]  sigmoid of their logits
      n_active      int32 [T]       triplets whose logit is above logit(threshold)
      topk_ivt      int32 [T, k, 3] (instrument, verb, target) of every top-K triplet (`metrics._TRIPLETS`)
      top_i / top_v / top_t         (ids int32 [T], scores float32 [T]): the component heads' own first pick
      scores        None, or {head -> float32 [T, K]} sigmoid scores of the four heads (keep_scores)"""

    def __init__(self, frames: Sequence[str], topk_ids, topk_scores, n_active, top_i, top_v, top_t, threshold: float = 0.5, scores=None):
        self.frames = [str(f) for f in frames]
        self.topk_ids = np.asarray(topk_ids, dtype=np.int32)
        self.topk_scores = np.asarray(topk_scores, dtype=np.float32)
        self.n_active = np.asarray(n_active, dtype=np.int32)
        self.top_i, self.top_v, self.top_t = ((np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.float32)) for a, b in (top_i, top_v, top_t))
        self.threshold = float(threshold)
        self.scores = None if scores is None else {h: np.asarray(scores[h], dtype=np.float32) for h in HEADS}
        if self.topk_ids.shape != self.topk_scores.shape or self.topk_ids.ndim != 2 or self.topk_ids.shape[0] != len(self.frames):
            raise ValueError(f"Prediction: {len(self.frames)} frames, top-K arrays {self.topk_ids.shape} / {self.topk_scores.shape}")
        self.topk_ivt = np.array(_TRIPLETS, dtype=np.int32)[self.topk_ids]

    def _arrays(self):
        out = {"frames": np.array(self.frames, dtype=str), "threshold": np.float64(self.threshold), "topk_ids": self.topk_ids,
               "topk_scores": self.topk_scores, "n_active": self.n_active, "topk_ivt": self.topk_ivt}
        for h, (ids, sc) in (("i", self.top_i), ("v", self.top_v), ("t", self.top_t)):
            out[f"top_{h}_ids"], out[f"top_{h}_scores"] = ids, sc
        if self.scores is not None:
            out.update({f"scores_{h}": self.scores[h] for h in HEADS})
        return out

    def save(self, stem: str, names: Optional[Sequence[str]] = None):
        """`<stem>.npz` with the arrays above (`scores_<head>` when kept) and `<stem>.csv`: a header and one line per (frame, rank),
        `frame,rank,triplet,i,v,t,score[,name]`; names: 100 strings (`parse_names`)"""
        if names is not None and len(names) != len(_TRIPLETS):
            raise ValueError(f"names: {len(_TRIPLETS)} strings, one per triplet id; got {len(names)}")
        os.makedirs(os.path.dirname(os.path.abspath(stem)), exist_ok=True)
        np.savez(stem + ".npz", **self._arrays())
        with open(stem + ".csv", "w") as f:
            f.write("frame,rank,triplet,i,v,t,score" + (",name" if names is not None else "") + "\n")
            for fi, frame in enumerate(self.frames):
                for r in range(self.topk_ids.shape[1]):
                    tid = int(self.topk_ids[fi, r])
                    i, v, t = (int(c) for c in self.topk_ivt[fi, r])
                    name = "" if names is None else ',"' + str(names[tid]).replace('"', '""') + '"'
                    f.write(f"{frame},{r},{tid},{i},{v},{t},{float(self.topk_scores[fi, r]):.6f}{name}\n")

    @classmethod
    def load(cls, stem: str) -> "Prediction":
        with np.load(stem + ".npz") as z:
            scores = {h: z[f"scores_{h}"] for h in HEADS} if "scores_ivt" in z.files else None
            return cls([str(f) for f in z["frames"]], z["topk_ids"], z["topk_scores"], z["n_active"], (z["top_i_ids"], z["top_i_scores"]),
                       (z["top_v_ids"], z["top_v_scores"]), (z["top_t_ids"], z["top_t_scores"]), float(z["threshold"]), scores)


def segments(pred: Prediction, min_len: int = 1):
    """runs of consecutive frames in which a triplet's score is above `pred.threshold`: [(triplet, first_frame_index, last_frame_index,
    mean_score)], ordered by first frame, then triplet; runs shorter than `min_len` frames are left out.  From the full score matrix when the
    prediction kept it, otherwise from the top-K (a triplet above the threshold but below a frame's K-th place then breaks its run there)."""
    n = len(pred.frames)
    if pred.scores is not None:
        s = np.asarray(pred.scores["ivt"], dtype=np.float32)
    else:
        s = np.full((n, len(_TRIPLETS)), -np.inf, dtype=np.float32)
        if n:
            s[np.arange(n)[:, None], pred.topk_ids] = pred.topk_scores
    on = s > np.float32(pred.threshold)
    out = []
    for tid in np.flatnonzero(on.any(axis=0)):
        col = on[:, tid].astype(np.int8)
        edges = np.diff(np.concatenate([[0], col, [0]]))
        for a, b in zip(np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)):        # [a, b)
            if b - a >= min_len:
                out.append((int(tid), int(a), int(b - 1), float(s[a:b, tid].astype(np.float64).mean())))
    return sorted(out, key=lambda r: (r[1], r[0], r[2]))


def save_segments(path: str, segs, frames: Sequence[str], names: Optional[Sequence[str]] = None):
    """`<video>.segments.csv`: `triplet,first_index,last_index,first_frame,last_frame,frames,mean_score[,name]`"""
    with open(path, "w") as f:
        f.write("triplet,first_index,last_index,first_frame,last_frame,frames,mean_score" + (",name" if names is not None else "") + "\n")
        for tid, a, b, m in segs:
            name = "" if names is None else ',"' + str(names[tid]).replace('"', '""') + '"'
            f.write(f"{tid},{a},{b},{frames[a]},{frames[b]},{b - a + 1},{m:.6f}{name}\n")


class Predictor:
    """student: a loaded `spatial_cnn.VideoNas`; temporal: a loaded `temporal_tenco.VideoNas` or None (the student's own four heads are decoded).
    height, width: the Resize target; device_batch: frames per student pass (a frame's result does not depend on it); png_decode / decode_workers:
    as the extraction drivers' flags; topk <= 32; threshold in (0, 1): a triplet counts as on when its logit is above logit(threshold).
    online_chunk N > 0: the latency mode -- the frames go N at a time through the student, `tenco_stream.TencoStream.push` (temporal must be a
    causal head) and the top-K decode, every answer computed from the frames seen so far; `chunk_latencies_ms` holds the last video's per-chunk
    times (frames on the device -> decoded rows on the device, one synchronise per chunk).  0: the whole-video pass.
    online_streams S > 1 (with online_chunk): S videos at once through `tenco_stream.StreamBank`, see `predict_streams`."""

    def __init__(self, student, temporal=None, *, height: int = 256, width: int = 448, device_batch: int = 512, png_decode: str = "host",
                 decode_workers: int = 8, topk: int = 5, threshold: float = 0.5, online_chunk: int = 0, online_streams: int = 1):
        from . import ops
        if not 1 <= int(topk) <= ops.TOPK_MAX_K:
            raise ValueError(f"topk {topk}: 1..{ops.TOPK_MAX_K} (`mt4_topk_rows_f32` keeps a row's winners in one wave's lanes)")
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"threshold {threshold}: a sigmoid score strictly between 0 and 1")
        if png_decode not in ("host", "device"):
            raise ValueError(f"png_decode {png_decode!r}: host | device")
        self.student, self.temporal = student.eval(), temporal.eval() if temporal is not None else None
        self.height, self.width, self.device_batch = int(height), int(width), max(1, int(device_batch))
        self.png_decode, self.decode_workers = png_decode, int(decode_workers)
        self.topk, self.threshold = int(topk), float(threshold)
        self.online_chunk, self.chunk_latencies_ms, self._stream = int(online_chunk), [], None
        self.online_streams, self.tick_latencies_ms, self.tick_frames, self._bank = int(online_streams), [], [], None
        if not 1 <= self.online_streams <= ops.STREAM_MAX_SLOTS:
            raise ValueError(f"online_streams {online_streams}: 1..{ops.STREAM_MAX_SLOTS} videos open at once")
        if self.online_streams > 1 and not self.online_chunk:
            raise ValueError("online_streams > 1 needs the streaming mode (online_chunk > 0)")
        if self.online_chunk:
            from .tenco_stream import StreamBank, TencoStream
            if not 1 <= self.online_chunk <= ops.STREAM_MAX_CHUNK:
                raise ValueError(f"online_chunk {online_chunk}: 1..{ops.STREAM_MAX_CHUNK} frames per `TencoStream.push`")
            if self.temporal is None:
                raise ValueError("online_chunk: the streaming mode needs a temporal head")
            if self.online_streams > 1:
                self._bank = StreamBank(self.temporal, self.online_streams)
            else:
                self._stream = TencoStream(self.temporal)                     # (refuses a non-causal, --hier or bf16 head with the reason)

    def features(self, paths: Sequence[str]):
        """the student over the frames -> (features fp32 [T, D], logits fp32 (i, v, t, ivt)), all on the device.  Loads run ahead of the model
        on side streams (`extract.iter_chunks`); the device PNG decoder gets loads of >= 1024 frames, two in flight, as in `Spatial_cnn/test.py`"""
        import torch

        from . import cholect, extract
        paths = list(paths)
        step, dev_dec = self.device_batch, self.png_decode == "device"
        lb = (1023 // step + 1) * step if dev_dec else step
        spans = [(s, min(len(paths), s + lb)) for s in range(0, len(paths), lb)]
        load = lambda s, e: cholect.load_files_device(paths[s:e], self.height, self.width, workers=self.decode_workers, decode=self.png_decode)
        feats, logits = [], [[], [], [], []]
        for span in extract.iter_chunks(spans, load, 2 if dev_dec else 1):
            for p0 in range(0, span.shape[0], step):
                (_, li), (_, lv), (_, lt), (feat, livt) = self.student.extract_u8(span[p0:p0 + step])
                feats.append(feat)
                for acc, lg in zip(logits, (li, lv, lt, livt)):
                    acc.append(lg)
        return torch.cat(feats).float(), tuple(torch.cat(l).float() for l in logits)       # concatenated ON the device: [2000, 512] fp32 is 4 MB

    def logits(self, paths: Sequence[str]):
        """{head -> fp32 [T, K] logits on the device, as VIEWS in the layout the model left them in}: the whole-video TCN on the student's
        features (`model(x, False)`, the finest FPN level, as `drivers._tenco_scores`), or the student's own heads without a temporal model"""
        feat, (li, lv, lt, livt) = self.features(paths)
        if self.temporal is None:
            return {"ivt": livt, "i": li, "v": lv, "t": lt}
        out, out_i, out_v, out_t, _, _ = self.temporal(feat.unsqueeze(0), False)
        return {h: lg[0][0].transpose(0, 1) for h, lg in (("ivt", out), ("i", out_i), ("v", out_v), ("t", out_t))}

    def _decode(self, lg, keep_scores: bool):
        """{head -> logits [n, K]} -> the device pieces of a `Prediction`: top-K ids, scores, counts, the component heads' picks[, score matrices]"""
        import torch

        from . import ops
        k = min(self.topk, lg["ivt"].shape[1])
        ids, vals, n_act = ops.topk_rows(lg["ivt"], k, count_above=math.log(self.threshold / (1.0 - self.threshold)))
        parts = [ids, torch.sigmoid(vals), n_act]
        for h in ("i", "v", "t"):
            hid, hval, _ = ops.topk_rows(lg[h], 1)
            parts += [hid, torch.sigmoid(hval)]
        if keep_scores:
            parts += [torch.sigmoid(lg[h]) for h in HEADS]
        return parts

    def _online_parts(self, paths: Sequence[str], keep_scores: bool):
        """the frames in order, `online_chunk` at a time: student pass -> `TencoStream.push` -> decode of the chunk's rows; the pieces of the
        chunks are joined on the device.  A frame's rows do not depend on the chunk size (the student's and the stream's results do not)."""
        import time

        import torch

        from . import cholect
        self._stream.reset()
        self.chunk_latencies_ms = []
        chunks = []
        for s in range(0, len(paths), self.online_chunk):
            fr = cholect.load_files_device(paths[s:s + self.online_chunk], self.height, self.width, workers=self.decode_workers, decode=self.png_decode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            feat = self.student.extract_u8(fr)[3][0]
            chunks.append(self._decode(self._stream.push(feat.float().contiguous()), keep_scores))
            torch.cuda.synchronize()
            self.chunk_latencies_ms.append((time.perf_counter() - t0) * 1e3)
        return [torch.cat([c[j] for c in chunks]) for j in range(len(chunks[0]))]

    def predict_streams(self, videos: Sequence, keep_scores: bool = False):
        """online_streams > 1: [(name, frame paths)] -> yields (name, Prediction, that video's tick latencies in ms, the `time.time()` it was
        opened at) as each video ends.  Up to `online_streams` videos are open at once; a tick takes the next `online_chunk` frames of every open video through
        ONE load, ONE student pass, ONE `StreamBank.push_rows` and ONE decode, whose rows are then dealt to the videos (slot order).  A frame's rows
        are those of `predict_paths`: neither the student's, the bank's nor the decode's results depend on what shares a pass.  `tick_latencies_ms`
        / `tick_frames` hold every tick of the call."""
        import time

        import torch

        from . import cholect
        if self._bank is None:
            raise ValueError("predict_streams: a Predictor built with online_streams > 1")
        waiting = [(name, list(paths)) for name, paths in videos]
        if any(not paths for _, paths in waiting):
            raise ValueError("predict_streams: a video without frames")
        waiting.reverse()
        bank, live = self._bank, {}                       # slot -> [name, paths, frames taken, chunks, latencies, opened at]
        self.tick_latencies_ms, self.tick_frames = [], []
        while waiting or live:
            while waiting and len(live) < self.online_streams:
                name, paths = waiting.pop()
                live[bank.open()] = [name, paths, 0, [], [], time.time()]
            slots = sorted(live)
            take = {s: live[s][1][live[s][2]:live[s][2] + self.online_chunk] for s in slots}
            fr = cholect.load_files_device([p for s in slots for p in take[s]], self.height, self.width, workers=self.decode_workers,
                                           decode=self.png_decode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            feat = self.student.extract_u8(fr)[3][0]
            parts = self._decode(bank.push_rows({s: len(take[s]) for s in slots}, feat.float().contiguous()), keep_scores)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            self.tick_latencies_ms.append(ms)
            self.tick_frames.append(fr.shape[0])
            at = 0
            for s in slots:
                v, n = live[s], len(take[s])
                v[3].append([p[at:at + n] for p in parts])
                v[4].append(ms)
                v[2] += n
                at += n
                if v[2] == len(v[1]):
                    bank.close(s)
                    del live[s]
                    joined = [torch.cat([c[j] for c in v[3]]) for j in range(len(parts))]
                    yield v[0], self._to_prediction(v[1], joined, keep_scores), v[4], v[5]

    def predict_paths(self, paths: Sequence[str], keep_scores: bool = False) -> Prediction:
        paths = list(paths)
        if not paths:
            raise ValueError("predict_paths: no frames")
        if self._bank is not None:
            raise ValueError("predict_paths: a Predictor with online_streams > 1 answers through predict_streams")
        if self.online_chunk:
            parts = self._online_parts(paths, keep_scores)
        else:
            parts = self._decode(self.logits(paths), keep_scores)
        return self._to_prediction(paths, parts, keep_scores)

    def _to_prediction(self, paths: Sequence[str], parts, keep_scores: bool) -> Prediction:
        import torch
        n = parts[0].shape[0]
        # every piece is 4 bytes wide: one buffer, ONE device-to-host copy per video
        flat = torch.cat([p.reshape(-1).view(torch.int32) for p in parts]).cpu().numpy()
        pieces, at = [], 0
        for p in parts:
            a = flat[at:at + p.numel()]
            pieces.append((a if p.dtype == torch.int32 else a.view(np.float32)).reshape(tuple(p.shape)).copy())
            at += p.numel()
        scores = dict(zip(HEADS, pieces[9:13])) if keep_scores else None
        flat1 = lambda a: a.reshape(n)
        return Prediction([os.path.basename(p) for p in paths], pieces[0], pieces[1], pieces[2], (flat1(pieces[3]), flat1(pieces[4])),
                          (flat1(pieces[5]), flat1(pieces[6])), (flat1(pieces[7]), flat1(pieces[8])), self.threshold, scores)
