"""CholecT45/T50 on-disk layout (SURVEY 8(b) "Labels"): `<data_dir>/data/VIDnn/%06d.png`,
`<data_dir>/{triplet,instrument,verb,target}/VIDnn.txt` (CSV int: col 0 frame id, cols 1.. multi-hot).
Split tables as in `Spatial_cnn/dataloader.py:112-148`; the extraction variant lists ALL videos
(`dataloader_test.py:87-88`).  CPU side only (PNG decode + resize): the normalisation runs on the GPU."""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import numpy as np

# official cross-validation folds / fixed splits (dataset metadata)
_SPLITS = {
    "cholect45-crossval": {1: [79, 2, 51, 6, 25, 14, 66, 23, 50], 2: [80, 32, 5, 15, 40, 47, 26, 48, 70],
                           3: [31, 57, 36, 18, 52, 68, 10, 8, 73], 4: [42, 29, 60, 27, 65, 75, 22, 49, 12],
                           5: [78, 43, 62, 35, 74, 1, 56, 4, 13]},
    "cholect50-crossval": {1: [79, 2, 51, 6, 25, 14, 66, 23, 50, 111], 2: [80, 32, 5, 15, 40, 47, 26, 48, 70, 96],
                           3: [31, 57, 36, 18, 52, 68, 10, 8, 73, 103], 4: [42, 29, 60, 27, 65, 75, 22, 49, 12, 110],
                           5: [78, 43, 62, 35, 74, 1, 56, 4, 13, 92]},
    "cholect50": {"train": [1, 15, 26, 40, 52, 65, 79, 2, 18, 27, 43, 56, 66, 92, 4, 22, 31, 47, 57, 68, 96, 5, 23, 35, 48, 60, 70,
                            103, 13, 25, 36, 49, 62, 75, 110], "val": [8, 12, 29, 50, 78], "test": [6, 51, 10, 73, 14, 74, 32, 80, 42, 111]},
    "cholect50-challenge": {"train": [1, 15, 26, 40, 52, 79, 2, 27, 43, 56, 66, 4, 22, 31, 47, 57, 68, 23, 35, 48, 60, 70, 13, 25, 49, 62,
                                      75, 8, 12, 29, 50, 78, 6, 51, 10, 73, 14, 32, 80, 42], "val": [5, 18, 36, 65, 74],
                            "test": [92, 96, 103, 110, 111]},
    "cholect45-challenge": {"train": [1, 15, 26, 40, 52, 79, 2, 27, 43, 56, 66, 4, 22, 31, 47, 57, 5, 23, 35, 48, 60, 18, 13, 25, 49, 62,
                                      65, 8, 12, 29, 50, 78, 6, 51, 10, 36, 14, 32, 80, 42], "val": [68, 70, 73, 74, 75],
                            "test": [92, 96, 103, 110, 111]},
}
_SPLITS["cholect45"] = _SPLITS["cholect45-crossval"]


def video_name(v: int) -> str:
    return "VID{}".format(str(v).zfill(2))


def split_videos(variant: str, test_fold: int) -> Tuple[List[str], List[str], List[str]]:
    """(train, val, test) video names; crossval: val = last 5 train videos (`dataloader.py:77-84`)."""
    if variant not in _SPLITS:
        raise ValueError(f"{variant} is not a valid dataset variant")
    sp = _SPLITS[variant]
    if "crossval" in variant or variant == "cholect45":
        train = [v for k in sp if k != test_fold for v in sp[k]]
        test = list(sp[test_fold])
        train, val = train[:-5], train[-5:]
    else:
        train, val, test = list(sp["train"]), list(sp["val"]), list(sp["test"])
    return [video_name(v) for v in train], [video_name(v) for v in val], [video_name(v) for v in test]


def extraction_videos(variant: str, test_fold: int) -> List[str]:
    """all videos in the order train + test + val (`dataloader_test.py:88`)"""
    tr, va, te = split_videos(variant, test_fold)
    return tr + te + va


def load_labels(data_dir: str, video: str) -> Dict[str, np.ndarray]:
    out = {}
    for key, sub in (("ivt", "triplet"), ("i", "instrument"), ("v", "verb"), ("t", "target")):
        a = np.loadtxt(os.path.join(data_dir, sub, f"{video}.txt"), dtype=np.int64, delimiter=",", ndmin=2)
        out[key] = a
    return out


_WARNED_PNG = False


def load_frames_u8(data_dir: str, video: str, frame_ids, height: int = 256, width: int = 448) -> np.ndarray:
    """decode + `Resize((height,width))` (bilinear, as torchvision does on PIL images; `dataloader.py:155-159`) -> uint8 [N,H,W,3]"""
    from PIL import Image
    out = np.empty((len(frame_ids), height, width, 3), np.uint8)
    for i, fid in enumerate(frame_ids):
        with Image.open(os.path.join(data_dir, "data", video, "{}.png".format(str(int(fid)).zfill(6)))) as im:
            im = im.convert("RGB")
            if im.size != (width, height):
                im = im.resize((width, height), Image.BILINEAR)
            out[i] = np.asarray(im)
    return out


def load_frames_device(data_dir: str, video: str, frame_ids, height: int = 256, width: int = 448, device="cuda", workers: int = 0,
                       decode: str = "host"):
    """Same bytes as `load_frames_u8`, as a uint8 [N,H,W,3] tensor on the GPU: the PNGs are decoded on the host at their native size
    and `Resize((height,width))` runs on the device (`ops.resize_bilinear_u8`, byte-identical to Pillow's bilinear resize).  Frames
    of one native size go through one launch pair; a video mixing sizes falls back to one group per size.  workers > 1: the PNGs
    are decoded by that many threads (Pillow releases the GIL while it inflates; the reference's loader has 3 worker processes,
    `Spatial_cnn/test.py:240-241`)."""
    paths = [os.path.join(data_dir, "data", video, "{}.png".format(str(int(fid)).zfill(6))) for fid in frame_ids]
    return load_files_device(paths, height, width, device=device, workers=workers, decode=decode)


def load_files_device(paths, height: int = 256, width: int = 448, device="cuda", workers: int = 0, decode: str = "host"):
    """`load_frames_device` over PNG paths (the frames of a shuffled training batch come from many videos)"""
    import struct

    import torch
    from PIL import Image

    from . import _lib, ops

    if len(paths) == 0:
        return torch.empty((0, height, width, 3), dtype=torch.uint8, device=device)
    if decode == "device":
        # decode = "device": the files are only read; inflate + unfiltering run on the GPU (`pngdec.decode_batch`, 8-bit RGB non-interlaced PNGs --
        # what the dataset ships; anything else raises `pngdec.UnsupportedPng`).  Same bytes as the Pillow path.
        from . import pngdec
        try:
            try:      # one frame size (a video): the files go to the device as they lie on disk, no host copy of the compressed bytes
                x = pngdec.decode_files(paths, device, workers=max(8, workers))
                return x if tuple(x.shape[1:3]) == (height, width) else ops.resize_bilinear_u8(x, height, width)
            except pngdec.MixedSizes:
                pass
            files = []
            for p in paths:
                with open(p, "rb") as fh:
                    files.append(fh.read())
            sizes: Dict[tuple, List[int]] = {}
            for i, f in enumerate(files):
                w0, h0, _ = pngdec._idat_spans(f)
                sizes.setdefault((h0, w0), []).append(i)
            out = torch.empty((len(files), height, width, 3), dtype=torch.uint8, device=device)
            for (h0, w0), idx in sizes.items():
                x = pngdec.decode_batch([files[i] for i in idx], device, workers=max(8, workers))
                y = x if (h0, w0) == (height, width) else ops.resize_bilinear_u8(x, height, width)
                out[torch.tensor(idx, device=device)] = y
            return out
        except (pngdec.UnsupportedPng, pngdec.DecodeError, _lib.Mt4Error, struct.error) as e:
            # a PNG flavour the device decoder does not cover (palette, grey, alpha, 16-bit, interlaced, wider than 4096), a malformed chunk
            # list, a stream it reports as bad, or a launch the library refuses (Pillow then has the last word on the file): this batch goes
            # through Pillow; said once
            global _WARNED_PNG
            if not _WARNED_PNG:
                print(f"[cholect] --png_decode device: {e}; such files are decoded by Pillow on the host", flush=True)
                _WARNED_PNG = True
            decode = "host"
    assert decode == "host"

    def decode_one(path):
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))
    if workers > 1 and len(paths) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=workers) as ex:
            raw = list(ex.map(decode_one, paths))
    else:
        raw = [decode_one(p) for p in paths]
    out = torch.empty((len(raw), height, width, 3), dtype=torch.uint8, device=device)
    groups: Dict[tuple, List[int]] = {}
    for i, a in enumerate(raw):
        groups.setdefault(a.shape[:2], []).append(i)
    for (h0, w0), idx in groups.items():
        x = torch.from_numpy(np.stack([raw[i] for i in idx])).to(device)
        y = x if (h0, w0) == (height, width) else ops.resize_bilinear_u8(x, height, width)
        out[torch.tensor(idx, device=device)] = y
    return out


class FrameCache:
    """The resized uint8 frames of a run kept in HBM across epochs (`--frame_cache GB`): what `load_files_device(paths, h, w)` returns is a pure
    function of the file and the size, so epochs 2 ... N of a frame trainer -- and every validation after the first -- take their frames from a
    pool on the device instead of reading, inflating, unfiltering and resizing every PNG again.  Only what FOLLOWS is random (the train
    transform), so no byte of any batch changes.

    The pool is one uint8 [slots, h, w, 3] tensor, slots = budget_bytes // (h * w * 3), allocated on the first `plan`, whose (h, w) fixes the
    frame size; a request at another size bypasses the cache, and so does every request if the allocation ran out of memory (said once).  Keys
    are the path strings.  A slot is free, ASSIGNED (handed to a path by `plan`, being written by that chunk's `fetch`) or READABLE; first come,
    first served, nothing is ever evicted.

    `plan(paths, h, w)` -> (take_slots, put_slots) int32 [n], on the CONSUMER thread only, in chunk order: it is the only place that touches
    the table.  `fetch(paths, plan, load)` runs wherever the load runs (a helper thread and side stream of `extract.iter_chunks`), decodes the
    misses with ONE `load(miss_paths)` call (none at all on a full hit), stores the rows that got a slot (`ops.put_frames`) and takes the hits
    (`ops.take_frames`): exactly `load(paths)`.  `seal()` makes the assigned slots readable, after one device-wide synchronize that orders
    every later stream behind the stores; the drivers call it after every training epoch and every validation.  Nothing becomes readable
    between two `seal()` calls, so a chunk never reads a slot another chunk in flight on another side stream is still writing -- a path seen
    again before `seal()` is decoded again and not stored.
    `stats`: hits, misses, stored (frames), slots and bytes of the pool."""

    def __init__(self, budget_bytes, device="cuda"):
        self.budget, self.device = max(0, int(budget_bytes)), device
        self.size = None                    # (h, w) of the pool, fixed by the first plan
        self.pool = None
        self.table: Dict[str, int] = {}     # path -> slot, assigned or readable
        self.readable = 0                   # slots [0, readable) are readable, [readable, len(table)) assigned: slots are handed out in order
        self.stats = {"hits": 0, "misses": 0, "stored": 0, "slots": 0, "bytes": 0}

    # ------------------------------------------------------------------------------------------------ device side (replaced by numpy in the CPU tests)
    def _alloc(self, slots, h, w):
        import torch
        return torch.empty((slots, h, w, 3), dtype=torch.uint8, device=self.device)

    def _put(self, slots, frames):
        from . import ops
        ops.put_frames(self.pool, slots, frames)

    def _take(self, slots, out):
        from . import ops
        ops.take_frames(self.pool, slots, out)

    def _empty(self, n):
        import torch
        return torch.empty((n,) + tuple(self.pool.shape[1:]), dtype=torch.uint8, device=self.pool.device)

    def _scatter(self, out, rows, frames):
        import torch
        out[torch.from_numpy(rows).to(out.device)] = frames

    def _synchronize(self):
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------------ host logic
    def _open(self, h, w):
        """the first plan: the pool at this size, or an empty cache (a budget below one frame, or no memory for the pool)"""
        self.size = (int(h), int(w))
        slots = self.budget // (int(h) * int(w) * 3)
        if slots > 0:
            try:
                self.pool = self._alloc(slots, int(h), int(w))
            except (MemoryError, RuntimeError) as e:
                if not isinstance(e, MemoryError) and "out of memory" not in str(e).lower():
                    raise
                print(f"[cholect] --frame_cache: no memory for a pool of {slots} frames of {h} x {w} ({slots * h * w * 3 / 2 ** 30:.1f} GiB); "
                      "the run goes on without the cache", flush=True)
                slots = 0
        self.stats["slots"], self.stats["bytes"] = slots, slots * int(h) * int(w) * 3

    def plan(self, paths, h, w):
        n = len(paths)
        take, put = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        if self.size is None:
            self._open(h, w)
        if (int(h), int(w)) != self.size or not self.stats["slots"]:
            self.stats["misses"] += n
            return take, put
        for i, p in enumerate(paths):
            s = self.table.get(p)
            if s is None:
                if len(self.table) < self.stats["slots"]:
                    s = self.table[p] = len(self.table)
                    put[i] = s
                    self.stats["stored"] += 1
            elif s < self.readable:
                take[i] = s
        hits = int((take >= 0).sum())
        self.stats["hits"] += hits
        self.stats["misses"] += n - hits
        return take, put

    def seal(self):
        if len(self.table) > self.readable:
            self._synchronize()
            self.readable = len(self.table)

    def fetch(self, paths, plan, load):
        take, put = plan
        miss = np.flatnonzero(take < 0)
        if len(miss) == len(paths):                          # nothing to take (the first epoch, a bypass, an empty cache)
            out = load(list(paths))
            if len(paths) and (put >= 0).any():
                self._put(put, out)
            return out
        out = self._empty(len(paths))
        if len(miss):
            decoded = load([paths[i] for i in miss])
            self._scatter(out, miss, decoded)
            if (put[miss] >= 0).any():
                self._put(np.ascontiguousarray(put[miss]), decoded)
        self._take(take, out)
        return out


def fetch_files(cache, paths, plan, load):
    """`load(paths)` through `cache` (a `FrameCache` with the `plan` of these paths), or directly without one"""
    return load(list(paths)) if cache is None else cache.fetch(paths, plan, load)
