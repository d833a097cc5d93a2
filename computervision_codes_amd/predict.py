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
LOCALIZE_HEADS = ("i", "ivt")
LOC_ARRAYS = ("loc_peak", "loc_box", "loc_area", "loc_range")


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
      scores        None, or {head -> float32 [T, K]} sigmoid scores of the four heads (keep_scores)
    and, when localisation ran (`loc`: a dict of the arrays below without the prefix; None otherwise, and then every attribute is None):
      loc_peak      int32 [T, k, 2]   (y, x) cell of the maximum of each top-K triplet's class-activation map
      loc_box       int32 [T, k, 4]   (y0, x0, y1, x1), inclusive, in cells: the region around the peak (`ops.class_maps`)
      loc_area      int32 [T, k]      its cell count
      loc_range     float32 [T, k, 2] minimum and maximum of the map
      loc_cells / loc_frame           (h, w) of the layer4 grid / (H, W) of the resized frame
      loc_head / loc_frac             "i" | "ivt": the head whose columns were mapped / the region's threshold fraction
      loc_maps      None, or float32 [T, k, h, w] the maps themselves (--save_maps)"""

    def __init__(self, frames: Sequence[str], topk_ids, topk_scores, n_active, top_i, top_v, top_t, threshold: float = 0.5, scores=None, loc=None):
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
        self.loc_peak = self.loc_box = self.loc_area = self.loc_range = self.loc_cells = self.loc_frame = self.loc_head = self.loc_frac = self.loc_maps = None
        if loc is not None:
            t, k = self.topk_ids.shape
            self.loc_peak, self.loc_box, self.loc_area = (np.asarray(loc[n], dtype=np.int32) for n in ("peak", "box", "area"))
            self.loc_range = np.asarray(loc["range"], dtype=np.float32)
            self.loc_cells, self.loc_frame = tuple(int(v) for v in loc["cells"]), tuple(int(v) for v in loc["frame"])
            self.loc_head, self.loc_frac = str(loc["head"]), float(loc["frac"])
            if self.loc_head not in LOCALIZE_HEADS:
                raise ValueError(f"Prediction: loc head {self.loc_head!r}: one of {LOCALIZE_HEADS}")
            if (self.loc_peak.shape, self.loc_box.shape, self.loc_area.shape, self.loc_range.shape) != ((t, k, 2), (t, k, 4), (t, k), (t, k, 2)):
                raise ValueError(f"Prediction: localisation arrays {self.loc_peak.shape} / {self.loc_box.shape} / {self.loc_area.shape} / "
                                 f"{self.loc_range.shape} for top-K arrays {self.topk_ids.shape}")
            if loc.get("maps") is not None:
                self.loc_maps = np.asarray(loc["maps"], dtype=np.float32)
                if self.loc_maps.shape != (t, k) + self.loc_cells:
                    raise ValueError(f"Prediction: loc maps {self.loc_maps.shape}, expected {(t, k) + self.loc_cells}")

    def loc_columns(self):
        """int32 [T, k]: the column of `loc_head` that localised each top-K triplet (its own id, or its instrument)"""
        return self.topk_ids if self.loc_head == "ivt" else np.ascontiguousarray(self.topk_ivt[..., 0])

    def loc_pixels(self):
        """(peak float64 [T, k, 2] as (x, y), box float64 [T, k, 4] as (x0, y0, x1, y1)) in resized-frame pixels: cell x covers
        [x W / w, (x + 1) W / w), a box is written by its outer edges, the peak as its cell's centre"""
        (h, w), (fh, fw) = self.loc_cells, self.loc_frame
        sy, sx = fh / h, fw / w
        peak = np.stack([(self.loc_peak[..., 1] + 0.5) * sx, (self.loc_peak[..., 0] + 0.5) * sy], axis=-1)
        b = self.loc_box.astype(np.float64)
        return peak, np.stack([b[..., 1] * sx, b[..., 0] * sy, (b[..., 3] + 1) * sx, (b[..., 2] + 1) * sy], axis=-1)

    def _arrays(self):
        out = {"frames": np.array(self.frames, dtype=str), "threshold": np.float64(self.threshold), "topk_ids": self.topk_ids,
               "topk_scores": self.topk_scores, "n_active": self.n_active, "topk_ivt": self.topk_ivt}
        for h, (ids, sc) in (("i", self.top_i), ("v", self.top_v), ("t", self.top_t)):
            out[f"top_{h}_ids"], out[f"top_{h}_scores"] = ids, sc
        if self.scores is not None:
            out.update({f"scores_{h}": self.scores[h] for h in HEADS})
        if self.loc_head is not None:
            out.update({n: getattr(self, n) for n in LOC_ARRAYS})
            out.update(loc_cells=np.array(self.loc_cells, dtype=np.int32), loc_frame=np.array(self.loc_frame, dtype=np.int32),
                       loc_head=np.array(self.loc_head), loc_frac=np.float64(self.loc_frac))
            if self.loc_maps is not None:
                out["loc_maps"] = self.loc_maps
        return out

    def save(self, stem: str, names: Optional[Sequence[str]] = None):
        """`<stem>.npz` with the arrays above (`scores_<head>` when kept) and `<stem>.csv`: a header and one line per (frame, rank),
        `frame,rank,triplet,i,v,t,score[,name]`; names: 100 strings (`parse_names`).  With localisation also `<stem>.loc.csv`:
        `frame,rank,triplet,column,peak_x,peak_y,x0,y0,x1,y1,area` in resized-frame pixels (`loc_pixels`), area in cells"""
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
        if self.loc_head is not None:
            peak, box = self.loc_pixels()
            cols = self.loc_columns()
            with open(stem + ".loc.csv", "w") as f:
                f.write("frame,rank,triplet,column,peak_x,peak_y,x0,y0,x1,y1,area\n")
                for fi, frame in enumerate(self.frames):
                    for r in range(self.topk_ids.shape[1]):
                        nums = ",".join(f"{float(v):.3f}" for v in (*peak[fi, r], *box[fi, r]))
                        f.write(f"{frame},{r},{int(self.topk_ids[fi, r])},{int(cols[fi, r])},{nums},{int(self.loc_area[fi, r])}\n")

    @classmethod
    def load(cls, stem: str) -> "Prediction":
        with np.load(stem + ".npz") as z:
            scores = {h: z[f"scores_{h}"] for h in HEADS} if "scores_ivt" in z.files else None
            loc = None
            if "loc_head" in z.files:
                loc = dict(peak=z["loc_peak"], box=z["loc_box"], area=z["loc_area"], range=z["loc_range"], cells=z["loc_cells"], frame=z["loc_frame"],
                           head=str(z["loc_head"]), frac=float(z["loc_frac"]), maps=z["loc_maps"] if "loc_maps" in z.files else None)
            return cls([str(f) for f in z["frames"]], z["topk_ids"], z["topk_scores"], z["n_active"], (z["top_i_ids"], z["top_i_scores"]),
                       (z["top_v_ids"], z["top_v_scores"]), (z["top_t_ids"], z["top_t_scores"]), float(z["threshold"]), scores, loc)


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
    online_streams S > 1 (with online_chunk): S videos at once through `tenco_stream.StreamBank`, see `predict_streams`.
    localize "i" | "ivt" (None: off, and then no launch, line or output byte differs): where in the frame each top-K triplet is.  The student's
    heads are linear layers on the average of the layer4 map, so a column's class-activation map M_c = sum_k W[c, k] F[y, x, k] is exact
    (mean(M_c) + b_c is the column's logit).  "ivt" maps each top-K triplet by its own column of the triplet head, "i" by the instrument-head
    column of its instrument (`topk_ivt[..., 0]`).  In every mode each student pass calls `ops.class_maps` ONCE on that pass's layer4 map, for
    all columns of the chosen head (6 or 100) -- the winners are only known after the decode, with a whole-video temporal head only after the
    TCN -- and the map is released; peak, region (`localize_frac`: the region is the connected component of {M >= min + frac (max - min)} around
    the peak) and range of ALL columns stay on the device, 10 words per frame and column, and the winners' rows are gathered with torch indexing
    after `_decode` and join the one device-to-host copy.  localize_maps (--save_maps) keeps the dense maps too until the gather: T x ncol x h x w
    x 4 bytes per video, 90 MB for 2000 frames of "ivt" at 8 x 14; without it the dense buffer is 8 MB for the same video."""

    def __init__(self, student, temporal=None, *, height: int = 256, width: int = 448, device_batch: int = 512, png_decode: str = "host",
                 decode_workers: int = 8, topk: int = 5, threshold: float = 0.5, online_chunk: int = 0, online_streams: int = 1,
                 localize: Optional[str] = None, localize_frac: float = 0.5, localize_maps: bool = False):
        from . import ops
        if not 1 <= int(topk) <= ops.TOPK_MAX_K:
            raise ValueError(f"topk {topk}: 1..{ops.TOPK_MAX_K} (`mt4_topk_rows_f32` keeps a row's winners in one wave's lanes)")
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"threshold {threshold}: a sigmoid score strictly between 0 and 1")
        if png_decode not in ("host", "device"):
            raise ValueError(f"png_decode {png_decode!r}: host | device")
        if localize is not None and localize not in LOCALIZE_HEADS:
            raise ValueError(f"localize {localize!r}: None | 'i' | 'ivt'")
        if not 0.0 <= float(localize_frac) <= 1.0:
            raise ValueError(f"localize_frac {localize_frac}: a fraction of the map's range, 0..1")
        if localize_maps and localize is None:
            raise ValueError("localize_maps needs localize 'i' or 'ivt'")
        if localize is not None and localize not in getattr(student, "_head_slices", {}):
            raise ValueError(f"localize {localize!r}: the student (loss_type {getattr(student, 'loss_type', None)!r}) has no {localize!r} head to map")
        self.localize, self.localize_frac, self.localize_maps, self._loc_dense = localize, float(localize_frac), bool(localize_maps), None
        self._loc_cells = None                                       # (h, w) of the layer4 grid, known after the first student pass
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
        feats, logits, locs = [], [[], [], [], []], []
        for span in extract.iter_chunks(spans, load, 2 if dev_dec else 1):
            for p0 in range(0, span.shape[0], step):
                ((_, li), (_, lv), (_, lt), (feat, livt)), loc = self._student_pass(span[p0:p0 + step])
                feats.append(feat)
                locs.append(loc)
                for acc, lg in zip(logits, (li, lv, lt, livt)):
                    acc.append(lg)
        # the dense localisation rows of the video, for the gather behind `_decode` (None without localize)
        self._loc_dense = [torch.cat(c) for c in zip(*locs)] if self.localize else None
        return torch.cat(feats).float(), tuple(torch.cat(l).float() for l in logits)       # concatenated ON the device: [2000, 512] fp32 is 4 MB

    def _student_pass(self, frames_u8):
        """one student pass -> (the forward's tuple, None | [regions int32 [n, ncol, 8], range fp32 [n, ncol, 2][, maps fp32 [n, ncol, h, w]]] of
        ALL columns of the localising head: ONE `ops.class_maps` launch on the pass's layer4 map, which is then released)"""
        from . import ops
        if self.localize is None:
            return self.student.extract_u8(frames_u8), None
        out, fmap = self.student.extract_u8(frames_u8, return_map=True)
        lo, hi = self.student._head_slices[self.localize]
        maps, regions, rng = ops.class_maps(fmap, self.student._p["heads.rows"], lo, hi - lo, self.localize_frac)
        self._loc_cells = (int(fmap.shape[1]), int(fmap.shape[2]))
        del fmap
        return out, [regions, rng] + ([maps] if self.localize_maps else [])

    def _gather_loc(self, ids, dense):
        """top-K triplet ids int32 [n, k] + the dense rows of `_student_pass` -> the winners' rows [n, k, ...], on the device"""
        import torch
        cols = ids.long()
        if self.localize == "i":
            cols = torch.tensor([t[0] for t in _TRIPLETS], dtype=torch.long, device=ids.device)[cols]
        rows = torch.arange(ids.shape[0], device=ids.device)[:, None]
        return [d[rows, cols] for d in dense]

    def logits(self, paths: Sequence[str]):
        """{head -> fp32 [T, K] logits on the device, as VIEWS in the layout the model left them in}: the whole-video TCN on the student's
        features (`model(x, False)`, the finest FPN level, as `drivers._tenco_scores`), or the student's own heads without a temporal model"""
        feat, (li, lv, lt, livt) = self.features(paths)
        if self.temporal is None:
            return {"ivt": livt, "i": li, "v": lv, "t": lt}
        out, out_i, out_v, out_t, _, _ = self.temporal(feat.unsqueeze(0), False)
        return {h: lg[0][0].transpose(0, 1) for h, lg in (("ivt", out), ("i", out_i), ("v", out_v), ("t", out_t))}

    def _decode(self, lg, keep_scores: bool, loc=None):
        """{head -> logits [n, K]} -> the device pieces of a `Prediction`: top-K ids, scores, counts, the component heads' picks[, score matrices]
        [, the winners' localisation rows out of `loc`, the dense rows of the same n frames]"""
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
        if loc is not None:
            parts += self._gather_loc(ids, loc)
        return parts

    def _timed_tick(self, paths: Sequence[str], push, keep_scores: bool):
        """one online tick: the frames of `paths` through ONE load, ONE student pass, `push(features fp32 [n, D])` (a `TencoStream.push` or a
        `StreamBank.push_rows`) and ONE decode -> (the decoded pieces, the milliseconds from the loaded frames to the decoded rows, both ends
        synchronised, and the number of frames)"""
        import time

        import torch

        from . import cholect
        fr = cholect.load_files_device(paths, self.height, self.width, workers=self.decode_workers, decode=self.png_decode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, loc = self._student_pass(fr)
        feat = out[3][0]
        parts = self._decode(push(feat.float().contiguous()), keep_scores, loc)
        torch.cuda.synchronize()
        return parts, (time.perf_counter() - t0) * 1e3, fr.shape[0]

    def _online_parts(self, paths: Sequence[str], keep_scores: bool):
        """the frames in order, `online_chunk` at a time: student pass -> `TencoStream.push` -> decode of the chunk's rows; the pieces of the
        chunks are joined on the device.  A frame's rows do not depend on the chunk size (the student's and the stream's results do not)."""
        import torch
        self._stream.reset()
        self.chunk_latencies_ms = []
        chunks = []
        for s in range(0, len(paths), self.online_chunk):
            parts, ms, _ = self._timed_tick(paths[s:s + self.online_chunk], self._stream.push, keep_scores)
            chunks.append(parts)
            self.chunk_latencies_ms.append(ms)
        return [torch.cat([c[j] for c in chunks]) for j in range(len(chunks[0]))]

    def predict_streams(self, videos: Sequence, keep_scores: bool = False):
        """online_streams > 1: [(name, frame paths)] -> yields (name, Prediction, that video's tick latencies in ms, the `time.time()` it was
        opened at) as each video ends.  Up to `online_streams` videos are open at once; a tick takes the next `online_chunk` frames of every open video through
        ONE load, ONE student pass, ONE `StreamBank.push_rows` and ONE decode, whose rows are then dealt to the videos (slot order).  A frame's rows
        are those of `predict_paths`: neither the student's, the bank's nor the decode's results depend on what shares a pass.  `tick_latencies_ms`
        / `tick_frames` hold every tick of the call."""
        import time

        import torch
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
            parts, ms, frames = self._timed_tick([p for s in slots for p in take[s]],
                                                 lambda feat: bank.push_rows({s: len(take[s]) for s in slots}, feat), keep_scores)
            self.tick_latencies_ms.append(ms)
            self.tick_frames.append(frames)
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
            lg = self.logits(paths)
            parts, self._loc_dense = self._decode(lg, keep_scores, self._loc_dense), None
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
        loc = None
        if self.localize:
            at = 13 if keep_scores else 9
            reg, rng = pieces[at], pieces[at + 1]
            maps = pieces[at + 2] if self.localize_maps else None
            cells = self._loc_cells
            loc = dict(peak=reg[..., 0:2], box=reg[..., 2:6], area=reg[..., 6], range=rng, cells=cells, frame=(self.height, self.width),
                       head=self.localize, frac=self.localize_frac, maps=maps)
        return Prediction([os.path.basename(p) for p in paths], pieces[0], pieces[1], pieces[2], (flat1(pieces[3]), flat1(pieces[4])),
                          (flat1(pieces[5]), flat1(pieces[6])), (flat1(pieces[7]), flat1(pieces[8])), self.threshold, scores, loc)
