"""GPU: the 'brightness' augmentation on the device: `mt4_aug_sharpen_u8` alone against the 'sharp' stage of `augment.reference_u8`, the
whole device transform against the Pillow path (`drivers.load_train_frames_u8`) byte for byte, `_frame_batch`, the prefetching loader and
the Spatial_cnn trainer with a list that names it."""
import argparse
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from computervision_codes_amd import augment, cholect

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["original", "vflip", "hflip", "contrast", "rot90"]
FULL = ["original", "vflip", "hflip", "contrast", "brightness", "rot90"]
SHARP_FIRST = ["brightness", "contrast", "rot90"]
FLAT = ["vflip", "brightness", "hflip"]
SEED = 5
R, C = augment.SHARP_ROWS, augment.SHARP_COLS


def _frames(b, h, w, seed=1):
    """uniform random bytes; frame 1 has a constant green channel, frame 2 a narrow value range"""
    x = np.random.default_rng(seed).integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    x[1 % b, ..., 1] = 77
    x[2 % b] = x[2 % b] // 3 + 40
    return x


def _write_frames(tmp_path, n, h0, w0, seed=0):
    from PIL import Image
    d = tmp_path / "data" / "VID01"
    os.makedirs(d, exist_ok=True)
    for i, a in enumerate(_frames(n, h0, w0, seed)):
        Image.fromarray(a).save(d / f"{i:06d}.png")
    return str(tmp_path), "VID01", list(range(n))


def _pillow_sharp(a):
    from PIL import Image, ImageEnhance
    return np.asarray(ImageEnhance.Sharpness(Image.fromarray(np.ascontiguousarray(a))).enhance(1.6))


def _table(b, h, w, contrast, sharpen):
    """identity rows with the given contrast / sharpen columns"""
    t = np.zeros((b, augment.NPARAMS), np.int32)
    t[:] = (0, 0, 65536, 0, 32768, 0, 65536, 32768, w, h, 0, 0)
    t[:, 10], t[:, 11] = contrast, sharpen
    return augment.Params(t, h, w, False)


# ------------------------------------------------------------------------------------------------ 6. the kernel alone
@pytest.mark.parametrize("h,w", [(37, 53), (64, 48), (3, 3), (2, 5), (R - 1, 2 * C + 4), (R, C), (R + 1, C + 1), (2 * R + 1, C - 1)])
def test_sharpen_kernel_equals_its_reference_stage(cuda, h, w):
    b = 5
    x = _frames(b, h, w)
    xd = torch.from_numpy(x).to(cuda)
    if h >= 3 and w >= 3:                                             # Pillow itself on the random frame: both clamps of the blend occur
        inner = _pillow_sharp(x[0])[1:-1, 1:-1]
        assert np.array_equal(augment.sharpen_u8(x[0]), _pillow_sharp(x[0]))
        if inner.size >= 1000:
            assert (inner == 0).mean() >= 0.01 and (inner == 255).mean() >= 0.01
    # the autocontrast first: frames 0, 1 (constant channel), 2 (narrow range) read through their LUTs, frame 3 is sharpened as stored
    # ("autocontrast after": luts ignored), frame 4 did not draw it
    p = _table(b, h, w, [1, 1, 1, 1, 1], [2, 2, 2, 1, 0])
    luts = augment.reference_luts(x, p)
    table = torch.from_numpy(p.table).to(cuda)
    ld = torch.from_numpy(luts).to(cuda)
    want = augment.reference_sharp(x, luts, p)
    got = augment.sharpen_device(xd, ld, table).cpu().numpy()
    for i in range(b):
        assert np.array_equal(got[i], want[i]), (i, np.argwhere(got[i] != want[i])[:4])
    assert np.array_equal(got[4], x[4])                               # undrawn: bit for bit
    assert np.array_equal(got[3], augment.sharpen_u8(x[3]))           # (not through its LUTs)
    if h >= 3 and w >= 3:
        assert np.array_equal(got[3], _pillow_sharp(x[3])) and not np.array_equal(got[3], x[3])
        lut0 = np.stack([luts[0, c][x[0, ..., c]] for c in range(3)], -1)
        assert np.array_equal(got[0], _pillow_sharp(lut0))
    else:
        assert np.array_equal(got[3], x[3])
    # without LUTs: every drawn frame as stored, whatever its row says
    want = augment.reference_sharp(x, None, p)
    got = augment.sharpen_device(xd, None, table).cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(got[0], augment.sharpen_u8(x[0]))
    # the 'sharp' stage of the reference for drawn rows
    q = augment.draw_params(random.Random(1), ["contrast", "brightness"], b, h, w)                  # (seed 1: all three values in five rows)
    assert set(q.table[:, 11].tolist()) == {0, 1, 2}
    st = augment.reference_u8(x, q, stages=True)
    got = augment.sharpen_device(xd, torch.from_numpy(st["luts"]).to(cuda), torch.from_numpy(q.table).to(cuda)).cpu().numpy()
    assert np.array_equal(got, st["sharp"])


def test_sharpen_refusals_launch_nothing(cuda):
    from computervision_codes_amd import ops
    b, h, w = 2, 8, 8
    x = torch.from_numpy(_frames(b, h, w)).to(cuda)
    table = torch.from_numpy(_table(b, h, w, 0, 1).table).to(cuda)
    out = torch.full((b * h * w * 3 + 8,), 7, dtype=torch.uint8, device=cuda)
    f = ops.lib.mt4_aug_sharpen_u8
    assert f(None, None, table.data_ptr(), out.data_ptr(), b, h, w, None) != 0
    assert f(x.data_ptr(), None, None, out.data_ptr(), b, h, w, None) != 0
    assert f(x.data_ptr(), None, table.data_ptr(), None, b, h, w, None) != 0
    assert f(x.data_ptr(), None, table.data_ptr(), out.data_ptr(), 0, h, w, None) != 0
    assert f(x.data_ptr(), None, table.data_ptr(), out.data_ptr() + 1, b, h, w, None) != 0          # misaligned out
    assert f(x.data_ptr() + 2, None, table.data_ptr(), out.data_ptr(), 1, h, w, None) != 0          # misaligned frames
    assert f(x.data_ptr(), None, table.data_ptr(), x.data_ptr(), b, h, w, None) != 0                # in place
    assert f(x.data_ptr(), None, table.data_ptr(), out.data_ptr(), b, h, 4097, None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                     # nothing was launched
    assert f(x.data_ptr(), None, table.data_ptr(), out.data_ptr(), b, h, w, None) == 0
    assert np.array_equal(out[:b * h * w * 3].view(b, h, w, 3).cpu().numpy(), augment.reference_sharp(x.cpu().numpy(), None, _table(b, h, w, 0, 1)))
    assert bool((out[b * h * w * 3:] == 7).all())


# ------------------------------------------------------------------------------------------------ 7. the whole transform
@pytest.mark.parametrize("names", [FULL, SHARP_FIRST, FLAT])
@pytest.mark.parametrize("n,h,w", [(12, 37, 53), (4, 256, 448)])
def test_device_transform_equals_pillow_path(cuda, tmp_path, n, h, w, names):
    from computervision_codes_amd import drivers
    data, video, ids = _write_frames(tmp_path, n, h + 11, w - 9)
    want = drivers.load_train_frames_u8(data, video, ids, h, w, random.Random(SEED), names)
    p = augment.draw_params(random.Random(SEED), names, n, h, w)
    assert p.table[:, 11].any()
    if n == 12:
        assert set(p.table[:, 11].tolist()) == ({0, 1, 2} if names is FULL else {0, 1})
        if "contrast" in names:
            assert {(bool(c), bool(s)) for c, s in p.table[:, 10:12].tolist()} == {(False, False), (False, True), (True, False), (True, True)}
    rng = random.Random(SEED)
    got = augment.load_train_batch_device(data, [(video, i) for i in ids], h, w, rng, names, decode="host", workers=4)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    ref = random.Random(SEED)
    augment.draw_params(ref, names, n, h, w)
    assert rng.getstate() == ref.getstate()
    # every stage against the numpy reference
    x = cholect.load_frames_u8(data, video, ids, h, w)
    st = augment.reference_u8(x, p, stages=True)
    dev = augment.train_transform_device(torch.from_numpy(x).to(cuda), p, stages=True)
    for k in ("sharp", "luts", "canvas", "out"):
        assert np.array_equal(dev[k].cpu().numpy(), st[k]), k
    assert np.array_equal(st["out"], want)


def test_contrast_and_sharpening_drawn_everywhere_in_both_orders(cuda, tmp_path):
    """the constant channel and the narrow range through autocontrast AND sharpening, scripted draws"""
    from computervision_codes_amd import drivers

    class Scripted:
        def __init__(self, randoms, angles):
            self.randoms, self.angles = list(randoms), list(angles)

        def random(self):
            return self.randoms.pop(0)

        def uniform(self, a, b):
            return self.angles.pop(0)

    h, w = 37, 53
    data, video, ids = _write_frames(tmp_path, 4, h + 11, w - 9)
    for names in (["contrast", "brightness", "rot90"], SHARP_FIRST, ["contrast", "brightness"]):
        randoms, angles = [0.1, 0.1] * 4, [33.0, -71.5, 0.0, 90.0]
        want = drivers.load_train_frames_u8(data, video, ids, h, w, Scripted(randoms, angles), names)
        got = augment.load_train_batch_device(data, [(video, i) for i in ids], h, w, Scripted(randoms, angles), names, decode="host")
        assert np.array_equal(got.cpu().numpy(), want), names


def test_default_list_is_untouched(cuda):
    b, h, w = 6, 37, 53
    x = _frames(b, h, w)
    p = augment.draw_params(random.Random(SEED), DEFAULT, b, h, w)
    assert not p.table[:, 11].any()
    ref = augment.reference_u8(x, p, stages=True)
    st = augment.train_transform_device(torch.from_numpy(x).to(cuda), p, stages=True)
    assert "sharp" not in st and "sharp" not in ref and sorted(st) == ["canvas", "hpass", "luts", "out"]
    assert np.array_equal(st["out"].cpu().numpy(), ref["out"]) and np.array_equal(st["canvas"].cpu().numpy(), ref["canvas"])


# ------------------------------------------------------------------------------------------------ 8. plumbing
def _make_dataset(d, n_frames=3, h=64, w=96):
    """a CholecT45-shaped dataset of random PNG frames and label files -> its videos"""
    from PIL import Image
    rng = np.random.default_rng(3)
    vids = cholect.extraction_videos("cholect45-crossval", 1)
    for sub in ("triplet", "instrument", "verb", "target"):
        os.makedirs(os.path.join(d, sub))
    for v in vids:
        os.makedirs(os.path.join(d, "data", v))
        for sub, k in (("triplet", 100), ("instrument", 6), ("verb", 10), ("target", 15)):
            lab = np.concatenate([np.arange(n_frames)[:, None], (rng.random((n_frames, k)) < 0.15).astype(int)], 1)
            np.savetxt(os.path.join(d, sub, v + ".txt"), lab, fmt="%d", delimiter=",")
        for i in range(n_frames):
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, "data", v, f"{i:06d}.png"))
    return vids


class Dataset:
    """6 videos x 3 PNG frames with labels and teacher rows: 18 shuffled samples in batches of 4 (the last of 2)"""

    def __init__(self, root):
        from computervision_codes_amd import featfile, loader
        self.data = str(root / "CholecT45")
        self.vids = _make_dataset(self.data)[:6]
        self.labels = {v: cholect.load_labels(self.data, v) for v in self.vids}
        g = np.random.default_rng(2)
        self.tpred = {t: {featfile.video_key(v): g.standard_normal((3, k)).astype(np.float32) for v in self.vids} for t, k in (("i", 6), ("v", 10), ("t", 15))}
        self.tfeat = {t: {featfile.video_key(v): g.standard_normal((3, 16)).astype(np.float32) for v in self.vids} for t in "ivt"}
        samples = [(v, i) for v in self.vids for i in range(3)]
        random.Random(1).shuffle(samples)
        self.batches = [samples[s:s + 4] for s in range(0, len(samples), 4)]
        self.tables = loader.SampleTables(self.labels, self.tpred, self.tfeat)

    def namespace(self, png_decode, train_transform, names=FULL):
        return argparse.Namespace(data_dir=self.data, augmentation_list=names, png_decode=png_decode, decode_workers=4, train_transform=train_transform)


@pytest.fixture(scope="module")
def ds(cuda, tmp_path_factory):
    return Dataset(tmp_path_factory.mktemp("sharpness"))


@pytest.mark.parametrize("png_decode", ["host", "device"])
def test_frame_batch_device_equals_host(ds, png_decode):
    from computervision_codes_amd import drivers
    batch = [s for b in ds.batches for s in b]
    outs = {}
    for mode in ("host", "device"):
        rng = random.Random(SEED * 1000003)
        outs[mode] = drivers._frame_batch(ds.namespace(png_decode, mode), batch, ds.labels, ds.tpred, ds.tfeat, (48, 80), rng) + (rng.getstate(),)
    (fh, lh, ph, th, sh), (fd, ld, pd, td, sd) = outs["host"], outs["device"]
    assert fd.is_cuda and fd.dtype == torch.uint8 and tuple(fd.shape) == (18, 48, 80, 3)
    assert torch.equal(fh, fd) and sh == sd
    p = augment.draw_params(random.Random(SEED * 1000003), FULL, 18, 48, 80)
    assert set(p.table[:, 11].tolist()) == {0, 1, 2}                 # the batch sharpened some frames, before and after an autocontrast
    for a, b in zip(lh + ph + th, ld + pd + td):
        assert torch.equal(a, b)


@pytest.mark.parametrize("names", [FULL, SHARP_FIRST])
def test_loader_equals_frame_batch(ds, names):
    from computervision_codes_amd import drivers, loader
    F, size = ds.namespace("device", "device", names), (48, 80)
    rng = random.Random(SEED * 1000003)
    want = [drivers._frame_batch(F, b, ds.labels, ds.tpred, ds.tfeat, size, rng) for b in ds.batches]
    state = rng.getstate()
    rng = random.Random(SEED * 1000003)
    with loader.FrameLoader(F, ds.batches, ds.labels, ds.tables, size, rng, prefetch=2) as fl:
        got = list(fl)
    assert len(got) == len(want) == 5 and rng.getstate() == state and fl.in_flight == 0 and fl.stats["frames"] == 18
    for (fg, lg, pg, tg), (fw, lw, pw, tw) in zip(got, want):
        assert torch.equal(fg, fw)
        for a, b in zip(list(lg) + list(pg) + list(tg), list(lw) + list(pw) + list(tw)):
            assert torch.equal(a.float().cpu(), b.float().cpu())
    # and the host transform's loader draws the same
    rng = random.Random(SEED * 1000003)
    with loader.FrameLoader(ds.namespace("device", "host", names), ds.batches, ds.labels, ds.tables, size, rng, prefetch=2) as fl:
        host = list(fl)
    assert rng.getstate() == state and all(torch.equal(h[0], w[0]) for h, w in zip(host, want))


def _teacher_files(base, vids, n):
    from computervision_codes_amd import featfile
    rng = np.random.default_rng(2)
    for t, k in (("i", 6), ("v", 10), ("t", 15)):
        featfile.write_feats(str(base / "run_T" / f"k1_{t}_feats.pkl"), {v[-2:]: rng.standard_normal((n, 1536)).astype(np.float32) for v in vids})
        featfile.write_feats(str(base / "run_TP" / f"k1_{t}_pred.pkl"), {v[-2:]: rng.standard_normal((n, k)).astype(np.float32) for v in vids})


_RECORDING_RUN = """
import hashlib, json, os, runpy, sys
from computervision_codes_amd.spatial_cnn_train import SpatialCnnTrainer
steps, inner = [], SpatialCnnTrainer.train_step
def train_step(self, frames, *args, **kw):
    assert frames.is_cuda and frames.dtype.is_floating_point is False
    steps.append(hashlib.sha256(frames.cpu().numpy().tobytes()).hexdigest())      # the bytes this step consumes
    return inner(self, frames, *args, **kw)
SpatialCnnTrainer.train_step = train_step
sys.argv = ["run.py"] + sys.argv[1:]
try:
    runpy.run_path("run.py", run_name="__main__")
finally:
    json.dump(steps, open(os.environ["MT4_TEST_STEPS"], "w"))
"""


def _run_student(tmp_path, tag, extra, record=False):
    """one epoch of `Spatial_cnn/run.py -t` (ResNet-18 student, --loss_type all) -> (stdout, the logged epoch loss, and with record=True the
    SHA-256 of the uint8 batch every `train_step` of that process was handed, in order)"""
    import json
    work = tmp_path / tag
    tree = work / "MT4MTLKD"
    shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
    data = str(work / "CholecT45")
    vids = _make_dataset(data, n_frames=2, h=40, w=56)
    _teacher_files(tree / "0-5fold" / "data_feats", vids, 2)
    env = dict(os.environ, PYTHONPATH=ROOT)
    head = [sys.executable, "run.py"]
    if record:
        (work / "recording_run.py").write_text(_RECORDING_RUN)
        env["MT4_TEST_STEPS"] = str(work / "steps.json")
        head = [sys.executable, str(work / "recording_run.py")]
    r = subprocess.run(head + ["-t", "--rates", "1", "1", "1", "--temp", "4", "--network", "resnet18", "--teacher_feat_version", "T",
                               "--teacher_pred_version", "TP", "--student_dim", "512", "--loss_type", "all", "--epochs", "1", "--batch", "8", "-l", "1e-2",
                               "5e-3", "1e-3", "--version", "S", "--val_interval", "1", "--data_dir", data, "--image_height", "32", "--image_width", "64",
                               "--kfold", "1"] + extra, cwd=tree / "Spatial_cnn", env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    log = open(tree / "Spatial_cnn" / "__checkpoint__" / "run_S" / "rendezvous_lcholect45-crossval_cholect1.log").read()
    lines = [ln for ln in log.splitlines() if "Traning | lr:" in ln]
    assert len(lines) == 1, log[-800:]
    loss = float(lines[0].split("| loss")[1].split("|")[0])
    assert np.isfinite(loss), lines[0]
    return r.stdout, loss, (json.load(open(env["MT4_TEST_STEPS"])) if record else None)


def test_spatial_cnn_trainer_consumes_the_host_paths_batches(cuda, tmp_path):
    """One epoch of the trainer under `--train_transform device` and one under `host`, each in a process of its own: every `train_step` of
    the device run is handed the bytes the host run's step is handed.  The logged losses are printed, not compared: the trainer reduces
    weight gradients, batch statistics and loss sums with float atomics, so two runs on the same bytes differ from the eighth digit of the
    first step's loss on, host against host as well ("Train transform on the device")."""
    out_d, loss_d, steps_d = _run_student(tmp_path, "device", ["--train_transform", "device", "--augmentation_list"] + FULL, record=True)
    out_h, loss_h, steps_h = _run_student(tmp_path, "host", ["--train_transform", "host", "--augmentation_list"] + FULL, record=True)
    print("epoch loss: device", loss_d, "host", loss_h)
    assert "has no device form" not in out_d
    assert len(steps_h) == 8 and len(set(steps_h)) == 8               # (8 batches of 8, all different)
    assert steps_d == steps_h


def test_brightness_after_rot90_trains_through_the_host_fallback_and_says_so_once(cuda, tmp_path):
    out, _, _ = _run_student(tmp_path, "fallback", ["--train_transform", "device", "--augmentation_list", "original", "vflip", "rot90", "brightness"])
    assert out.count("--train_transform device: the augmentation list") == 1 and "has no device form" in out
