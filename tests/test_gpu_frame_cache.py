"""GPU: the frame pool kernels (`mt4_put_frames_u8` / `mt4_take_frames_u8`: the 16-byte path, the byte-wise path, offsets past 2^31 and 2^32,
the refusals) and `cholect.FrameCache` behind the loaders (--frame_cache): a cached run must yield, batch for batch and epoch after epoch, the
bytes and values of the uncached run and leave the augmentation generator in the same state, while epochs 2 and 3 decode nothing the pool
holds; the synchronous path, the validation pass, and the student trainer end to end.  No test measures time."""
import argparse
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from computervision_codes_amd import cholect, featfile, loader

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_augment import NAMES, _teacher_files  # noqa: E402     (the default augmentation list, teacher files of the student trainer)
from test_gpu_scripts import _make_dataset  # noqa: E402              (the synthetic CholecT45-shaped dataset)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5
SIZE = (32, 48)
FRAME = SIZE[0] * SIZE[1] * 3


# ------------------------------------------------------------------------------------------------ the kernels
def _put_take(cuda, row_shape, offset=0):
    """pool of 9 slots, 5 frames, slots [4, -1, 0, 8, -1]: put, then take into a buffer of 0xA5 -> compared with torch indexing on the same tensors.
    offset: `frames` (and the take buffer) start that many bytes behind a 16-byte boundary"""
    from computervision_codes_amd import ops
    fb = int(np.prod(row_shape))
    g = torch.Generator().manual_seed(11)
    pool = torch.randint(0, 256, (9,) + row_shape, dtype=torch.uint8, generator=g).to(cuda)
    before = pool.clone()

    def rows(fill=None):
        base = torch.empty(5 * fb + 16, dtype=torch.uint8, device=cuda)
        assert base.data_ptr() % 16 == 0
        v = base[offset:offset + 5 * fb].view((5,) + row_shape)
        if fill is None:
            v.copy_(torch.randint(0, 256, (5,) + row_shape, dtype=torch.uint8, generator=g))
        else:
            v.fill_(fill)
        assert v.is_contiguous() and v.data_ptr() % 16 == offset
        return v
    frames = rows()
    slots = np.array([4, -1, 0, 8, -1], np.int32)
    idx, named = torch.tensor([0, 2, 3], device=cuda), torch.tensor([4, 0, 8], device=cuda)
    ops.put_frames(pool, slots, frames)
    want = before.clone()
    want[named] = frames[idx]
    assert torch.equal(pool, want)                                 # the rows not named still hold their pre-fill
    out = rows(0xA5)
    assert ops.take_frames(pool, slots, out) is out
    assert torch.equal(out[idx], pool[named]) and torch.equal(out[idx], frames[idx])
    assert bool((out[torch.tensor([1, 4], device=cuda)] == 0xA5).all())
    assert torch.equal(pool, want)


def test_kernel_vector_path(cuda):
    _put_take(cuda, (16 * 3,))


@pytest.mark.parametrize("offset", [0, 1])
def test_kernel_bytewise_path(cuda, offset):
    """frame_bytes = 105: no multiple of 16, slots 1 .. 8 of the pool are misaligned; once more with the frames 1 byte off a 16-byte boundary"""
    _put_take(cuda, (5, 7, 3), offset)


def test_kernel_vector_path_more_than_one_piece_group(cuda):
    """a row of 1024 + 3 pieces: two workgroups per frame, the second one short (the same assertions on a shape of a real frame's kind)"""
    _put_take(cuda, (13, 79, 16))
    assert 13 * 79 * 16 == 16 * 1027


def test_kernel_64_bit_offsets(cuda):
    """12485 slots x 344064 bytes (a 256 x 448 frame): slots 6241 | 6242 straddle the 2 GiB byte mark, 12484 lies past 4 GiB"""
    from computervision_codes_amd import ops
    free = torch.cuda.mem_get_info()[0]
    if free < 6e9:
        pytest.skip(f"needs 6 GB of free device memory for a 4.3 GB pool, {free / 1e9:.1f} GB are free")
    fb, n = 256 * 448 * 3, 12485
    assert 6241 * fb < 2 ** 31 < 6242 * fb and 12483 * fb < 2 ** 32 < 12484 * fb + fb and fb % 16 == 0
    pool = torch.empty((n, fb), dtype=torch.uint8, device=cuda)
    g = torch.Generator().manual_seed(12)
    frames = torch.randint(0, 256, (4, fb), dtype=torch.uint8, generator=g).to(cuda)
    guard = torch.randint(0, 256, (2, fb), dtype=torch.uint8, generator=g).to(cuda)
    pool[6240], pool[12483] = guard[0], guard[1]
    slots = np.array([0, 6241, 6242, 12484], np.int32)
    ops.put_frames(pool, slots, frames)
    for i, s in enumerate(slots.tolist()):
        assert torch.equal(pool[s], frames[i]), s
    out = torch.full((4, fb), 0xA5, dtype=torch.uint8, device=cuda)
    ops.take_frames(pool, slots, out)
    assert torch.equal(out, frames)
    assert torch.equal(pool[6240], guard[0]) and torch.equal(pool[12483], guard[1])
    del pool
    torch.cuda.empty_cache()


def test_kernel_refusals(cuda):
    from computervision_codes_amd import _lib, ops
    big = torch.full((12, 48), 7, dtype=torch.uint8, device=cuda)
    pool = big[:9]
    frames = torch.full((2, 48), 9, dtype=torch.uint8, device=cuda)
    none = np.empty(0, np.int32)
    ops.put_frames(pool, none, frames[:0])                          # n = 0: a successful no-op
    assert ops.take_frames(pool, none, frames[:0]).shape[0] == 0
    for bad in ([0, 9], [12, 1]):
        with pytest.raises(_lib.Mt4Error):                         # refused on the host, before the launch
            ops.put_frames(pool, np.array(bad, np.int32), frames)
        with pytest.raises(_lib.Mt4Error):
            ops.take_frames(pool, np.array(bad, np.int32), frames)
    with pytest.raises(_lib.Mt4Error):
        ops.put_frames(pool.cpu(), np.array([0, 1], np.int32), frames)
    torch.cuda.synchronize()
    assert bool((big == 7).all()) and bool((frames == 9).all())
    dev_slots = torch.tensor([10, 1], dtype=torch.int32, device=cuda)
    args = (pool.data_ptr(), dev_slots.data_ptr(), frames.data_ptr())
    for fn in (_lib.lib.mt4_put_frames_u8, _lib.lib.mt4_take_frames_u8):
        assert fn(*args, 2, 0, 9, None) == -1                      # frame_bytes = 0: MT4_EINVAL
        assert fn(*args, -1, 48, 9, None) == -1 and fn(*args, 2, 48, 0, None) == -1
        assert fn(*args, 0, 48, 9, None) == 0
    # the C entry point itself skips a slot >= pool_slots (slot 10 of a 9-slot pool, which here is the head of a 12-slot buffer): row 1 goes
    # to slot 1, nothing else changes
    stream = torch.cuda.current_stream().cuda_stream
    assert _lib.lib.mt4_put_frames_u8(*args, 2, 48, 9, stream) == 0
    torch.cuda.synchronize()
    want = torch.full((12, 48), 7, dtype=torch.uint8, device=cuda)
    want[1] = 9
    assert torch.equal(big, want)


# ------------------------------------------------------------------------------------------------ the loaders
class Dataset:
    """6 videos x 7 PNG frames (two of the videos at another native size), labels and teacher rows: 42 samples, shuffled anew every epoch into
    batches of 4 (the last of 2)"""

    def __init__(self, root):
        from PIL import Image
        self.data = str(root / "CholecT45")
        self.vids = _make_dataset(self.data, n_frames=7, h=64, w=96)[:6]
        g = np.random.default_rng(4)
        for v in self.vids[:2]:
            for i in range(7):
                Image.fromarray(g.integers(0, 255, (60, 100, 3), dtype=np.uint8)).save(os.path.join(self.data, "data", v, f"{i:06d}.png"))
        self.labels = {v: cholect.load_labels(self.data, v) for v in self.vids}
        g = np.random.default_rng(2)
        self.tpred = {t: {featfile.video_key(v): g.standard_normal((7, k)).astype(np.float32) for v in self.vids} for t, k in (("i", 6), ("v", 10), ("t", 15))}
        self.tfeat = {t: {featfile.video_key(v): g.standard_normal((7, 16)).astype(np.float32) for v in self.vids} for t in "ivt"}
        self.samples = [(v, i) for v in self.vids for i in range(7)]
        self.tables = loader.SampleTables(self.labels, self.tpred, self.tfeat)
        self.paths = {os.path.join(self.data, "data", v, "{:06d}.png".format(int(self.labels[v]["ivt"][i, 0]))) for v, i in self.samples}
        self.runs = {}

    def namespace(self, png_decode, train_transform="device"):
        return argparse.Namespace(data_dir=self.data, augmentation_list=NAMES, png_decode=png_decode, decode_workers=4, train_transform=train_transform)

    def epochs(self, png_decode, prefetch, cache, each_epoch=None):
        """three epochs -> ([the batches of every epoch], [the loader's stats per epoch], the generator's final state); prefetch 0 is the
        synchronous `_frame_batch` path.  The cache is sealed after every epoch, as the drivers do"""
        from computervision_codes_amd import drivers
        F = self.namespace(png_decode)
        order_rng, rng = random.Random(7), random.Random(SEED * 1000003)
        out, stats = [], []
        for epoch in range(3):
            order = list(self.samples)
            order_rng.shuffle(order)
            batches = [order[s:s + 4] for s in range(0, len(order), 4)]
            if each_epoch:
                each_epoch(epoch)
            if prefetch > 0:
                with loader.FrameLoader(F, batches, self.labels, self.tables, SIZE, rng, prefetch=prefetch, cache=cache) as fl:
                    out.append(list(fl))
                assert fl.in_flight == 0
                stats.append(dict(fl.stats))
            else:
                out.append([drivers._frame_batch(F, b, self.labels, self.tpred, self.tfeat, SIZE, rng, cache) for b in batches])
                stats.append(dict(cache.stats) if cache is not None else {})
            if cache is not None:
                cache.seal()
        return out, stats, rng.getstate()

    def uncached(self, png_decode, prefetch):
        """the reference of a (decoder, path) pair, computed once and left unchanged"""
        if (png_decode, prefetch) not in self.runs:
            self.runs[(png_decode, prefetch)] = self.epochs(png_decode, prefetch, None)
        return self.runs[(png_decode, prefetch)]


@pytest.fixture(scope="module")
def ds(cuda, tmp_path_factory):
    return Dataset(tmp_path_factory.mktemp("frame_cache"))


def _same_epochs(got, want):
    assert [len(e) for e in got] == [len(e) for e in want] == [11, 11, 11]
    for eg, ew in zip(got, want):
        for (fg, lg, pg, tg), (fw, lw, pw, tw) in zip(eg, ew):
            assert fg.is_cuda and fg.dtype == torch.uint8 and tuple(fg.shape[1:]) == SIZE + (3,)
            assert torch.equal(fg, fw)
            assert len(lg) == len(lw) == 4 and len(pg) == len(pw) == 3 and len(tg) == len(tw) == 3
            for a, b in zip(list(lg) + list(pg) + list(tg), list(lw) + list(pw) + list(tw)):
                assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.fixture()
def decoded(monkeypatch):
    """every path `cholect.load_files_device` is asked for, call by call"""
    calls, real = [], cholect.load_files_device

    def spy(paths, *a, **kw):
        calls.append(list(paths))
        return real(paths, *a, **kw)
    monkeypatch.setattr(cholect, "load_files_device", spy)
    return calls


@pytest.mark.parametrize("png_decode", ["device", "host"])
def test_loader_bytes_with_and_without_the_cache(ds, png_decode):
    want, base_stats, state = ds.uncached(png_decode, 2)
    assert all(s["frames_decoded"] == 42 and s["hits"] == 0 and s["decode_calls"] == s["chunks"] == 6 for s in base_stats)
    cache = cholect.FrameCache(1000 * FRAME)
    got, stats, end = ds.epochs(png_decode, 2, cache)
    _same_epochs(got, want)
    assert end == state
    assert stats[0]["frames_decoded"] == 42 and stats[0]["hits"] == 0 and stats[0]["decode_calls"] == 6
    for s in stats[1:]:
        assert s["decode_calls"] == 0 and s["frames_decoded"] == 0 and s["hits"] == s["frames"] == 42 and s["chunks"] == 6
    assert cache.stats == {"hits": 84, "misses": 42, "stored": 42, "slots": 1000, "bytes": 1000 * FRAME}
    assert tuple(cache.pool.shape) == (1000,) + SIZE + (3,) and cache.pool.dtype == torch.uint8


def test_loader_partial_budget(ds, decoded):
    """room for half the frames: the same bytes, and from epoch 2 on exactly the frames without a slot are decoded"""
    want, _, state = ds.uncached("device", 2)
    del decoded[:]
    cache = cholect.FrameCache(21 * FRAME + FRAME // 2)
    marks = []
    got, stats, end = ds.epochs("device", 2, cache, each_epoch=lambda e: marks.append(len(decoded)))
    _same_epochs(got, want)
    assert end == state
    assert cache.stats["slots"] == cache.stats["stored"] == len(cache.table) == 21 and set(cache.table) < ds.paths
    first, second, third = decoded[marks[0]:marks[1]], decoded[marks[1]:marks[2]], decoded[marks[2]:]
    assert sorted(p for c in first for p in c) == sorted(ds.paths)
    for calls, s in ((second, stats[1]), (third, stats[2])):
        assert sorted(p for c in calls for p in c) == sorted(ds.paths - set(cache.table))
        assert s["frames_decoded"] == 21 and s["hits"] == 21 and s["decode_calls"] == len(calls) <= 6
    assert cache.stats["hits"] == 42 and cache.stats["misses"] == 42 + 21 + 21


def test_synchronous_path(ds, decoded):
    """--prefetch 0: `_frame_batch` through the same plan + fetch"""
    want, _, state = ds.uncached("device", 0)
    del decoded[:]
    cache = cholect.FrameCache(1000 * FRAME)
    marks = []
    got, stats, end = ds.epochs("device", 0, cache, each_epoch=lambda e: marks.append(len(decoded)))
    _same_epochs(got, want)
    assert end == state
    assert len(decoded) == marks[1] == 11                          # one call per batch in epoch 1, none afterwards
    assert [(s["hits"], s["misses"]) for s in stats] == [(0, 42), (42, 42), (84, 42)]


def test_validation_pass_twice(ds, decoded):
    from computervision_codes_amd import drivers
    F = argparse.Namespace(data_dir=ds.data, png_decode="device", decode_workers=4, loss_type="all", metrics="host", batch=4, device_batch=5,
                           prefetch=2, dataset_variant="cholect45-crossval")
    forward = lambda fr: fr.float().reshape(fr.shape[0], -1)[:, :100] / 255.0 - 0.5
    vids = ds.vids[1:4]                                            # (one of them at the other native size)
    plain = drivers._frame_validation(F, vids, ds.labels, SIZE, 256, forward)
    del decoded[:]
    cache = cholect.FrameCache(1000 * FRAME)
    one = drivers._frame_validation(F, vids, ds.labels, SIZE, 256, forward, None, cache)
    assert sum(len(c) for c in decoded) == 21 and cache.stats["stored"] == 21 and cache.readable == 21       # (sealed by the pass itself)
    del decoded[:]
    two = drivers._frame_validation(F, vids, ds.labels, SIZE, 256, forward, None, cache)
    assert decoded == [] and cache.stats["hits"] == 21
    assert one[1] == two[1] == plain[1] and repr(one[0]) == repr(two[0]) == repr(plain[0])
    F.prefetch = 0                                                 # the inline span loop plans and fetches the same way
    assert drivers._frame_validation(F, vids, ds.labels, SIZE, 256, forward, None, cache)[1] == plain[1] and decoded == []


# ------------------------------------------------------------------------------------------------ the trainer
def _digits(log):
    """(loss digits per epoch, mAP digits per validation, the `| cache` notes) of a trainer's log"""
    epochs = [ln for ln in log.splitlines() if "Traning | lr:" in ln]
    maps = [ln.split("mAP =>")[1].strip() for ln in log.splitlines() if "mAP =>" in ln]
    return [ln.split("| loss")[1].split("|")[0].strip() for ln in epochs], maps, [ln.split("| cache ")[1].strip() if "| cache " in ln else None for ln in epochs]


@pytest.fixture(scope="module")
def student(cuda, tmp_path_factory):
    """`Spatial_cnn/run.py -t --prefetch 2 --epochs 2` on the tiny dataset with further flags -> (stdout, log); every run in a tree of its own.

    The learning rates are 0.  Two runs of one and the same command, without the flag, do not log the same digits once the weights move: the
    weight gradients close with float atomics (tests/test_gpu_loader.py says the same of --prefetch 0 against 2), and this tiny network at 32 x 64
    amplifies their order.  Measured on one MI355X with `-l 1e-2 5e-3 1e-3`, no --frame_cache anywhere: five runs of the --prefetch 0 line logged
    the losses (4.6941, 4.3431), (4.6942, 4.3345), (4.6942, 4.3330), (4.6942, 4.3325), (4.6942, 4.3330) and ivt mAPs 0.74889 ... 0.75889 in
    epoch 2; five of the --prefetch 2 line (4.6942, 4.3344), (4.6903, 4.3379) and three times (4.6942, 4.3330).  No loader can be held to digits
    the trainer itself does not repeat.  With the weights fixed every logged digit -- two epochs of training losses over differently shuffled and
    augmented batches, two validation mAPs -- is a function of the bytes the loader delivers and of nothing else, which is what the cache could
    change; the comparison asks the full equality of the digits there."""
    base = tmp_path_factory.mktemp("student")
    data = str(base / "CholecT45")
    vids = _make_dataset(data, n_frames=2, h=40, w=56)
    runs = {}

    def run(*extra):
        if extra not in runs:
            tree = base / f"run{len(runs)}" / "MT4MTLKD"
            shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
            _teacher_files(tree / "0-5fold" / "data_feats", vids, 2)
            r = subprocess.run([sys.executable, "run.py", "-t", "--rates", "1", "1", "1", "--temp", "4", "--network", "resnet18", "--teacher_feat_version",
                                "T", "--teacher_pred_version", "TP", "--student_dim", "512", "--loss_type", "all", "--epochs", "2", "--batch", "8", "-l",
                                "0", "0", "0", "--version", "S", "--val_interval", "1", "--data_dir", data, "--image_height", "32",
                                "--image_width", "64", "--kfold", "1", "--prefetch", "2"] + list(extra),
                               cwd=tree / "Spatial_cnn", env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
            runs[extra] = (r.stdout, open(tree / "Spatial_cnn" / "__checkpoint__" / "run_S" / "rendezvous_lcholect45-crossval_cholect1.log").read())
        return runs[extra]
    return run


def _finite(digits):
    assert all(np.isfinite(float(d)) for d in digits), digits


def test_student_trainer_with_the_cache_logs_the_same_digits(student):
    out0, log0 = student("--train_transform", "device")
    out1, log1 = student("--train_transform", "device", "--frame_cache", "1")
    loss0, map0, note0 = _digits(log0)
    loss1, map1, note1 = _digits(log1)
    assert len(loss0) == 2 and len(map0) == 2 and note0 == [None, None] and "--frame_cache" not in out0
    _finite(loss0)
    assert loss0[0] != loss0[1]                                    # (the epochs see other shuffles and draws: the digits do depend on the batches)
    assert loss1 == loss0 and map1 == map0
    assert note1 == ["0/62", "62/62"]                              # 31 training videos x 2 frames: epoch 2 takes every frame from the pool
    assert "--frame_cache" not in out1


def test_student_trainer_host_transform_says_so_and_logs_the_same_digits(student):
    out0, log0 = student("--train_transform", "host")              # the same line without --frame_cache
    out2, log2 = student("--train_transform", "host", "--frame_cache", "1")
    assert out2.count("--frame_cache: the train transform runs in Pillow on the host") == 1 and "--frame_cache" not in out0
    loss0, map0, _ = _digits(log0)
    loss2, map2, note2 = _digits(log2)
    _finite(loss0)
    assert len(loss0) == 2 and loss2 == loss0 and map2 == map0
    assert loss0 == _digits(student("--train_transform", "device")[1])[0]      # (host and device transform: the same bytes for the same draws)
    assert note2 == ["0/0", "0/0"]                                 # no training frame went through the cache; the validation frames did
