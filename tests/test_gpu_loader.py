"""GPU: `mt4_take_rows_f32` (rows of up to 16 fp32 tables from one launch) and the prefetching frame loader (`loader.FrameLoader`), which must
yield, batch for batch, the bytes and values `drivers._frame_batch` returns with a twin generator and leave the generator in the same state;
its early exit, its error hand-over, and the student trainer with `--prefetch 2`.  No test measures time."""
import argparse
import os
import random
import sys
import threading

import numpy as np
import pytest
import torch

from computervision_codes_amd import cholect, featfile, loader

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_augment import NAMES, _run_student  # noqa: E402        (the default augmentation list, the student trainer on a synthetic dataset)
from test_gpu_scripts import _make_dataset  # noqa: E402              (the synthetic CholecT45-shaped dataset)

pytestmark = pytest.mark.gpu
SEED = 5
WIDTHS = (6, 10, 15, 100, 6, 10, 15, 16, 16, 1536)


# ------------------------------------------------------------------------------------------------ the gather kernel
@pytest.fixture(scope="module")
def tables(cuda):
    g = torch.Generator().manual_seed(3)
    return [torch.randn((37, c), generator=g).to(cuda) for c in WIDTHS]


@pytest.mark.parametrize("n", [1, 5, 65])
def test_take_rows_equals_indexing(cuda, tables, n):
    """ten segments in one launch: widths that take the 16-byte path (100, 16, 1536) and the dword path (6, 10, 15: rows that are not 16-byte
    aligned); 65 rows = more than one row group, the last one short; repeated and descending indices"""
    from computervision_codes_amd import ops
    idx = {1: [36], 5: [36, 7, 7, 0, 3], 65: list(range(36, -1, -1)) + [36, 36, 0, 0] + list(range(30, 6, -1))}[n]
    assert len(idx) == n
    rows = torch.tensor(idx, dtype=torch.int64, device=cuda)
    outs = ops.take_rows(tables, rows)
    assert len(outs) == len(tables)
    for t, o in zip(tables, outs):
        assert o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == (n, t.shape[1])
        assert torch.equal(o, t[rows]), t.shape


def test_take_rows_empty_and_refusals(cuda, tables):
    from computervision_codes_amd import _lib, ops
    outs = ops.take_rows(tables, torch.empty(0, dtype=torch.int64, device=cuda))
    assert [tuple(o.shape) for o in outs] == [(0, c) for c in WIDTHS]
    rows = torch.zeros(3, dtype=torch.int64, device=cuda)
    with pytest.raises(_lib.Mt4Error):
        ops.take_rows(tables + tables, rows)                       # 20 tables: more than one launch carries
    with pytest.raises(_lib.Mt4Error):
        ops.take_rows([], rows)
    with pytest.raises(_lib.Mt4Error):
        ops.take_rows(tables[:1], rows.cpu())
    # a single table whose storage is only 4-byte aligned goes through the dword path although its width is a multiple of 4
    base = torch.randn(37 * 16 + 1, device=cuda)
    odd = base[1:].view(37, 16)
    assert odd.data_ptr() % 16 == 4
    idx = torch.tensor([5, 36, 0], dtype=torch.int64, device=cuda)
    assert torch.equal(ops.take_rows([odd], idx)[0], odd[idx])


# ------------------------------------------------------------------------------------------------ the loader against `_frame_batch`
class Dataset:
    """6 videos x 3 PNG frames, labels, teacher rows of width 6 / 10 / 15 and 16: 18 shuffled samples in batches of 4 (the last of 2)"""

    def __init__(self, root, h=64, w=96, odd_videos=0):
        from PIL import Image
        self.data = str(root / "CholecT45")
        self.vids = _make_dataset(self.data, n_frames=3, h=h, w=w)[:6]
        g = np.random.default_rng(4)
        for v in self.vids[:odd_videos]:                             # these videos' frames at another native size: a chunk then mixes sizes
            for i in range(3):
                Image.fromarray(g.integers(0, 255, (60, 100, 3), dtype=np.uint8)).save(os.path.join(self.data, "data", v, f"{i:06d}.png"))
        self.labels = {v: cholect.load_labels(self.data, v) for v in self.vids}
        g = np.random.default_rng(2)
        self.tpred = {t: {featfile.video_key(v): g.standard_normal((3, k)).astype(np.float32) for v in self.vids} for t, k in (("i", 6), ("v", 10), ("t", 15))}
        self.tfeat = {t: {featfile.video_key(v): g.standard_normal((3, 16)).astype(np.float32) for v in self.vids} for t in "ivt"}
        samples = [(v, i) for v in self.vids for i in range(3)]
        random.Random(1).shuffle(samples)
        self.batches = [samples[s:s + 4] for s in range(0, len(samples), 4)]
        assert [len(b) for b in self.batches] == [4, 4, 4, 4, 2]
        self.tables = loader.SampleTables(self.labels, self.tpred, self.tfeat)

    def namespace(self, png_decode, train_transform):
        return argparse.Namespace(data_dir=self.data, augmentation_list=NAMES, png_decode=png_decode, decode_workers=4, train_transform=train_transform)

    def reference(self, F, size, upto=None):
        """`_frame_batch` batch after batch with one generator -> (the batches, the generator's final state)"""
        from computervision_codes_amd import drivers
        rng = random.Random(SEED * 1000003)
        out = [drivers._frame_batch(F, b, self.labels, self.tpred, self.tfeat, size, rng) for b in self.batches[:upto]]
        return out, rng.getstate()


@pytest.fixture(scope="module")
def ds(cuda, tmp_path_factory):
    return Dataset(tmp_path_factory.mktemp("loader"))


def _same_batch(got, want, n):
    (fg, lg, pg, tg), (fw, lw, pw, tw) = got, want
    assert fg.is_cuda and fg.dtype == torch.uint8 and tuple(fg.shape) == tuple(fw.shape) and fg.shape[0] == n
    assert torch.equal(fg, fw)
    assert len(lg) == 4 and len(pg) == len(pw) == 3 and len(tg) == len(tw) == 3
    for a, b in zip(list(lg) + list(pg) + list(tg), list(lw) + list(pw) + list(tw)):
        assert a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and tuple(a.shape) == tuple(b.shape)
        assert torch.equal(a.float().cpu(), b.float().cpu())


def _compare(ds, F, size, k):
    want, state = ds.reference(F, size)
    rng = random.Random(SEED * 1000003)
    with loader.FrameLoader(F, ds.batches, ds.labels, ds.tables, size, rng, prefetch=k) as fl:
        got = list(fl)
    assert len(got) == len(want) == 5
    for g, w, b in zip(got, want, ds.batches):
        _same_batch(g, w, len(b))
    assert rng.getstate() == state
    assert fl.in_flight == 0 and fl.stats["frames"] == 18
    return fl


@pytest.mark.parametrize("train_transform", ["host", "device"])
@pytest.mark.parametrize("png_decode", ["host", "device"])
def test_loader_equals_frame_batch(ds, png_decode, train_transform):
    fl = _compare(ds, ds.namespace(png_decode, train_transform), (48, 80), 2)
    assert fl.stats["chunks"] == 3
    # one `load_files_device` call per chunk of the device transform (with --png_decode device: one inflate call); Pillow decodes the host
    # transform's frames one by one whatever --png_decode says, as in `_frame_batch`
    assert fl.stats["decode_calls"] == (3 if train_transform == "device" else 0)


@pytest.mark.parametrize("k,chunks", [(1, 5), (16, 1)])
def test_loader_chunk_of_one_batch_and_single_chunk(ds, k, chunks):
    fl = _compare(ds, ds.namespace("device", "device"), (48, 80), k)
    assert fl.stats["chunks"] == fl.stats["decode_calls"] == chunks


def test_loader_square_size_of_the_q2l_trainer(ds):
    _compare(ds, ds.namespace("device", "device"), (32, 32), 2)


def test_loader_chunk_mixing_native_sizes(cuda, tmp_path):
    mixed = Dataset(tmp_path, odd_videos=2)
    assert any(len({v in mixed.vids[:2] for b in mixed.batches[c:c + 2] for v, _ in b}) == 2 for c in (0, 2))      # a chunk holds both sizes
    _compare(mixed, mixed.namespace("device", "device"), (48, 80), 2)


@pytest.mark.parametrize("train_transform", ["host", "device"])
def test_early_exit_leaves_no_load_running(ds, train_transform):
    F, size = ds.namespace("device", train_transform), (48, 80)
    want, _ = ds.reference(F, size, upto=1)
    fl = loader.FrameLoader(F, ds.batches, ds.labels, ds.tables, size, random.Random(SEED * 1000003), prefetch=1)
    for got in fl:
        _same_batch(got, want[0], 4)
        break
    fl.close()                                                       # returns: the loads in flight have finished
    assert fl.in_flight == 0
    torch.cuda.synchronize()
    helpers = [t for t in threading.enumerate() if t.name.startswith("mt4-load-")]
    assert all(not t.daemon for t in helpers)                        # idle pool threads of `extract.iter_chunks`, joined at interpreter exit
    fl.close()                                                       # (a second close is a no-op)
    with loader.FrameLoader(F, ds.batches, ds.labels, ds.tables, size, random.Random(SEED * 1000003), prefetch=2) as again:
        _same_batch(next(iter(again)), want[0], 4)
    assert again.in_flight == 0


@pytest.mark.parametrize("train_transform", ["host", "device"])
def test_error_of_a_load_reaches_the_consumer_in_order(cuda, tmp_path, train_transform):
    d = Dataset(tmp_path)
    F, size = d.namespace("device", train_transform), (48, 80)
    want, _ = d.reference(F, size, upto=4)
    v, i = d.batches[4][1]
    os.remove(os.path.join(d.data, "data", v, "{:06d}.png".format(int(d.labels[v]["ivt"][i, 0]))))
    got = []
    with pytest.raises(FileNotFoundError):
        with loader.FrameLoader(F, d.batches, d.labels, d.tables, size, random.Random(SEED * 1000003), prefetch=2) as fl:
            for fb in fl:
                got.append(fb)
    assert len(got) == 4 and fl.in_flight == 0
    for g, w in zip(got, want):
        _same_batch(g, w, 4)


def test_sample_outside_the_tables_is_refused_on_the_host(ds):
    with pytest.raises(ValueError):
        ds.tables.take([(ds.vids[0], 0), (ds.vids[1], 3)])
    lab, tp, tf = ds.tables.take([(ds.vids[5], 2), (ds.vids[0], 0)])
    assert [tuple(t.shape) for t in lab + tp + tf] == [(2, c) for c in (6, 10, 15, 100, 6, 10, 15, 16, 16, 16)]
    assert np.array_equal(lab[3].cpu().numpy(), np.stack([ds.labels[ds.vids[5]]["ivt"][2, 1:], ds.labels[ds.vids[0]]["ivt"][0, 1:]]).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the trainer
def test_spatial_cnn_trainer_with_prefetch(cuda, tmp_path):
    """`Spatial_cnn/run.py -t --loss_type all --train_transform device --png_decode device --prefetch 2`: return code 0, a finite logged loss and
    a finite `_latest.pth` (losses are not compared with a --prefetch 0 run: the weight gradients close with float atomics; the batch-equality
    tests above carry the identity claim)"""
    out = _run_student(tmp_path, ["--png_decode", "device", "--prefetch", "2"])
    assert "has no device form" not in out
