"""The prefetching loader of the two frame trainers (`--prefetch K`, `drivers.spatial_cnn_train` / `drivers.spatial_transformer_train`).

`drivers._frame_batch` loads one batch synchronously: while the files are read, inflated and transformed the GPU runs one wave per frame of a
latency-bound kernel and nothing else, and while the step runs nothing is loaded.  The device PNG decoder takes ~74 ms per call for anything
up to 1024 frames (profiles/r02_png_decode.txt), so a batch of 64 pays for 1024.  Two pieces change that without changing a byte of what the
trainers see:

`SampleTables` keeps the label rows and the teacher prediction / feature rows of every training sample on the device (the reference's dataset
assembles them per sample on the host, `Spatial_cnn/dataloader.py:216-261`); the rows of a batch -- or of a chunk of batches -- come from ONE
launch of `mt4_take_rows_f32` instead of ten host-side `np.stack` calls and ten pageable uploads per step.

`FrameLoader` groups consecutive batches into chunks of up to K batches (at most 1024 frames: one round of inflate waves), loads a chunk with one
decode call, one transform and one gather on a side stream of a helper thread (`extract.iter_chunks`) and hands out its batches as views.  The
augmentation draws are made by the consumer, chunk by chunk in order, so the generator ends an epoch in the state `_frame_batch` leaves."""
from __future__ import annotations

import os
import threading
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import featfile

HEADS = (("i", 6), ("v", 10), ("t", 15), ("ivt", 100))
MAX_CHUNK_FRAMES = 1024         # one round of inflate waves: the decode call takes ~74 ms up to here and twice that at 1280 (profiles/r02_png_decode.txt)


def plan_chunks(n_batches: int, batch: int, k: int) -> List[Tuple[int, int]]:
    """[b0, b1) batch ranges of the chunks: consecutive batches in groups of min(k, max(1, 1024 // batch)); the last chunk may be short"""
    per = min(int(k), max(1, MAX_CHUNK_FRAMES // max(1, int(batch))))
    if per < 1:
        raise ValueError("prefetch must be >= 1 to plan chunks")
    return [(b0, min(n_batches, b0 + per)) for b0 in range(0, n_batches, per)]


class SampleTables:
    """The per-sample rows of a run, resident on the device: the four label tables as fp32 multi-hot [N, 6 | 10 | 15 | 100] (without the frame-id
    column) and, when the teacher files are given, the three prediction tables [N, 6 | 10 | 15] and the three feature tables [N, teacher_dim]
    (`astype(float32)`, as `drivers._frame_batch` converts them).  N = the frames of `videos` (default: every video of `labels`); sample
    (video, i) is row base[video] + i.  Device memory: N x (131 + 31 + 3 x teacher_dim) x 4 bytes per rank with teacher files, N x 131 x 4 without.

    `rows(batch)` maps samples to rows ON THE HOST and raises ValueError for a sample outside its video's rows before anything is uploaded;
    `take(batch)` -> (lab[4], tpred[3] | [], tfeat[3] | []) contiguous fp32 device tensors from one `mt4_take_rows_f32` launch.
    device=None keeps the tables as numpy arrays in `.host` and uploads nothing (`take` is then unavailable): the host part alone, for CPU tests."""

    def __init__(self, labels, tpred=None, tfeat=None, videos: Sequence[str] = None, device="cuda"):
        self.videos = list(labels.keys()) if videos is None else list(videos)
        self.base: Dict[str, int] = {}
        self.valid: Dict[str, int] = {}          # rows of the video that EVERY table holds (a teacher file may be shorter than the label file)
        n = 0
        for v in self.videos:
            self.base[v] = n
            n += len(labels[v]["ivt"])
        self.n = n
        self.has_teacher = bool(tpred) and bool(tfeat)
        self.device = device
        self.host: List[np.ndarray] = []
        self.tables = []
        for k, width in HEADS:
            self._add([labels[v][k][:, 1:] for v in self.videos], labels, width)
        if self.has_teacher:
            for files in (tpred, tfeat):
                for t in "ivt":
                    self._add([files[t][featfile.video_key(v)] for v in self.videos], labels, None)

    def _add(self, parts, labels, width):
        """one table [N, C] from the per-video arrays: a video's array is cut or zero-padded to its label rows, `valid` keeps the shorter count"""
        width = int(parts[0].shape[1]) if width is None and parts else width
        tab = np.zeros((self.n, width), np.float32)
        for v, a in zip(self.videos, parts):
            a = np.asarray(a)
            if a.ndim != 2 or a.shape[1] != width:
                raise ValueError(f"{v}: rows of width {a.shape[1:]} in a table of width {width}")
            rows = min(len(a), len(labels[v]["ivt"]))
            tab[self.base[v]:self.base[v] + rows] = a[:rows].astype(np.float32)
            self.valid[v] = min(self.valid.get(v, rows), rows)
        if self.device is None:
            self.host.append(tab)
        else:
            import torch
            self.tables.append(torch.from_numpy(tab).to(self.device))

    def rows(self, batch) -> np.ndarray:
        """int64 [B]: the table row of every (video, i) sample; ValueError for an unknown video or an i outside [0, rows of that video)"""
        out = np.empty(len(batch), np.int64)
        for j, (v, i) in enumerate(batch):
            if v not in self.base or not 0 <= int(i) < self.valid[v]:
                raise ValueError(f"sample ({v}, {i}) lies outside the sample tables ({self.valid.get(v, 0)} rows of that video, {self.n} in all)")
            out[j] = self.base[v] + int(i)
        if len(out) and not (0 <= int(out.min()) and int(out.max()) < self.n):
            raise ValueError(f"row {int(out.max())} outside the {self.n} rows of the sample tables")
        return out

    def take(self, batch):
        import torch
        from . import ops
        if self.device is None:
            raise ValueError("SampleTables(device=None) holds host tables only")
        idx = torch.from_numpy(self.rows(batch)).to(self.tables[0].device)       # (checked on the host above, before the upload)
        out = ops.take_rows(self.tables, idx)
        return out[:4], out[4:7], out[7:10]

    def nbytes(self) -> int:
        return sum(t.numel() * 4 for t in self.tables) + sum(t.nbytes for t in self.host)


class FrameLoader:
    """Iterate over `batches` (the list `trainloop.deal` returned for this rank and epoch) -> (frames, lab, tpred, tfeat) per batch: the bytes
    and values `drivers._frame_batch(F, batch, labels, tpred, tfeat, size, aug_rng)` returns batch after batch, labels and teacher rows as fp32
    device tensors from `tables` (a `SampleTables`); after the last batch `aug_rng` is in the state those calls leave.

    Consecutive batches form chunks of min(prefetch, max(1, 1024 // batch)) batches (`plan_chunks`).
    Device transform (`drivers._device_transform(F)`): a chunk is one `cholect.load_files_device` call (with --png_decode device one inflate
    call), one `augment.train_transform_device` and one `tables.take`, on a helper thread and a side stream of `extract.iter_chunks`; up to two
    chunks are in flight beside the one being consumed, and the decoder's blocking status read waits for its side stream on the helper.  The
    augmentation draws of a chunk are made by the CONSUMER when the chunk is submitted, in chunk order (`augment.draw_params` draws frame by
    frame, so one call over a chunk equals the per-batch calls in sequence); helper threads never touch `aug_rng`.
    Host transform: the draws are interleaved with Pillow work (`drivers._augment`), so ONE helper thread owns the generator for the epoch,
    produces the chunks strictly in order and runs one chunk ahead.
    Prefetch stays inside an epoch: the first chunk of every epoch is loaded while the consumer waits for it and is not hidden.
    An exception of a load is raised in the consumer when it asks for the first batch of the failing chunk, after every batch of the chunks
    before it.  `close()` (or leaving the `with` block, or exhausting the iterator) lets the loads in flight finish; no helper is launching on
    the GPU afterwards.  A loop left early finds `aug_rng` advanced by the chunks already submitted.
    `cache` (a `cholect.FrameCache`, --frame_cache; device transform only): the consumer also makes the chunk's plan when it submits the chunk
    (`cache.plan`, the only place that touches the cache's table) and the load goes through `cache.fetch` -- the frames the pool holds are taken
    from it, the others decoded by one call and stored; the same bytes.
    `stats`: chunks loaded, `cholect.load_files_device` calls that actually ran (`decode_calls`: at most one per chunk of the device transform
    -- none for a chunk the cache holds entirely --, none in the host transform, whose frames Pillow decodes one by one), frames loaded, frames
    those calls decoded (`frames_decoded`) and frames taken from the cache (`hits`)."""

    def __init__(self, F, batches, labels, tables: SampleTables, size, aug_rng, prefetch: int = 2, cache=None):
        from . import drivers
        if int(prefetch) < 1:
            raise ValueError("FrameLoader needs prefetch >= 1 (--prefetch 0 is the synchronous `_frame_batch` path)")
        self.F, self.batches, self.labels, self.tables, self.size, self.rng = F, list(batches), labels, tables, tuple(size), aug_rng
        self.device_transform = drivers._device_transform(F)
        self.chunks = plan_chunks(len(self.batches), max((len(b) for b in self.batches), default=1), int(prefetch))
        self.cache = cache if self.device_transform else None
        self.stats = {"chunks": 0, "decode_calls": 0, "frames": 0, "frames_decoded": 0, "hits": 0}
        self._lock = threading.Lock()
        self.in_flight = 0                       # loads running on a helper (or, for a single chunk, on the consumer) right now
        self._it = None
        self._handed = 0                         # batches handed out

    def check_drained(self):
        """after the `with` block: the epoch boundary --resume saves `aug_rng` at.  Every batch was handed out -- so every chunk was drawn and
        loaded -- and no helper is still running: the generator is in the state the epoch's `_frame_batch` calls leave.  RuntimeError
        otherwise (a loop left early)"""
        if self._handed != len(self.batches) or self.in_flight:
            raise RuntimeError(f"FrameLoader: {self._handed} of {len(self.batches)} batches handed out, {self.in_flight} loads in flight: aug_rng "
                               "is not at the epoch's end")

    # ------------------------------------------------------------------------------------------------ one chunk
    def _samples(self, b0, b1):
        return [s for b in self.batches[b0:b1] for s in b]

    def _paths(self, samples):
        return [os.path.join(self.F.data_dir, "data", v, "{}.png".format(str(int(self.labels[v]["ivt"][i, 0])).zfill(6))) for v, i in samples]

    def _draw(self, b0, b1):
        """consumer thread, chunk order: the draws of every frame of the chunk and, with a cache, the chunk's plan (device transform); the host
        transform draws inside its load"""
        if not self.device_transform:
            return None
        from . import augment
        params = augment.draw_params(self.rng, self.F.augmentation_list, sum(len(b) for b in self.batches[b0:b1]), self.size[0], self.size[1])
        plan = self.cache.plan(self._paths(self._samples(b0, b1)), self.size[0], self.size[1]) if self.cache is not None else None
        return params, plan

    def _load(self, b0, b1, prepared):
        import torch
        with self._lock:
            self.in_flight += 1
        try:
            F, (h, w), samples = self.F, self.size, self._samples(b0, b1)
            if self.device_transform:
                from . import augment, cholect
                params, plan = prepared
                decoded = []                                 # frames of every `load_files_device` call that ran

                def load(paths):
                    decoded.append(len(paths))
                    return cholect.load_files_device(paths, h, w, workers=F.decode_workers, decode=F.png_decode)
                x = cholect.fetch_files(self.cache, self._paths(samples), plan, load)
                frames = augment.train_transform_device(x, params)
            else:
                from .drivers import load_train_frames_u8
                frames = torch.from_numpy(np.concatenate([load_train_frames_u8(F.data_dir, v, [self.labels[v]["ivt"][i, 0]], h, w, self.rng,
                                                                               F.augmentation_list) for v, i in samples])).cuda()
                decoded = []
            lab, tp, tf = self.tables.take(samples)
            with self._lock:
                self.stats["chunks"] += 1
                self.stats["decode_calls"] += len(decoded)
                self.stats["frames"] += len(samples)
                self.stats["frames_decoded"] += sum(decoded)
                self.stats["hits"] += len(samples) - sum(decoded) if self.device_transform else 0
            return frames, lab, tp, tf
        finally:
            with self._lock:
                self.in_flight -= 1

    # ------------------------------------------------------------------------------------------------ iteration
    def _batches_of(self):
        from . import extract
        depth = 2 if self.device_transform else 1          # host transform: one thread owns the generator, chunks strictly in order
        loads = extract.iter_chunks(self.chunks, self._load, depth, prepare=self._draw)
        try:
            for (b0, b1), (frames, lab, tp, tf) in zip(self.chunks, loads):
                o = 0
                for b in self.batches[b0:b1]:              # batches are views into the chunk's tensors
                    e = o + len(b)
                    self._handed += 1
                    yield frames[o:e], [t[o:e] for t in lab], [t[o:e] for t in tp], [t[o:e] for t in tf]
                    o = e
        finally:
            loads.close()                                  # (left early: `iter_chunks` waits for the loads in flight)

    def __iter__(self):
        if self._it is not None:
            raise RuntimeError("a FrameLoader is iterated once (one per epoch)")
        self._it = self._batches_of()
        return self._it

    def close(self):
        """stop early: loads in flight finish (their buffers must outlive their kernels), nothing new is submitted"""
        if self._it is not None:
            self._it.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
