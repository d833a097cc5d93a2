"""GPU: the device train transform (csrc/augment_kernels.hip behind `augment.py`) returns the bytes of the Pillow path
(`drivers.load_train_frames_u8`) for the same rng; every kernel alone against its stage of `augment.reference_u8`; `_frame_batch` and the
two frame trainers with `--train_transform device`."""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import Scripted, _write_frames  # noqa: E402   (the scripted rng and the PNG writer of the CPU tests)
from test_gpu_scripts import _make_dataset  # noqa: E402             (the synthetic CholecT45-shaped dataset)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["original", "vflip", "hflip", "contrast", "rot90"]
SIZES = [(256, 448), (384, 384), (37, 53)]
SEED = 5


def _frames(b, h, w, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    x[1 % b, ..., 1] = 77
    x[2 % b] = x[2 % b] // 3 + 40
    return x


@pytest.mark.parametrize("h,w", SIZES)
def test_device_transform_equals_pillow_path(cuda, tmp_path, h, w):
    from computervision_codes_amd import drivers
    data, video, ids = _write_frames(tmp_path, 12, h + 11, w - 9)
    want = drivers.load_train_frames_u8(data, video, ids, h, w, random.Random(SEED), NAMES)
    p = augment.draw_params(random.Random(SEED), NAMES, 12, h, w)
    for col in (0, 1, 10):                                            # vflip, hflip, contrast: both values occur in the batch
        assert set(p.table[:, col].tolist()) == {0, 1}, col
    assert p.table[1, 10] == 1 and len(set(p.sizes())) > 1           # the constant channel goes through autocontrast; mixed canvas sizes
    rng = random.Random(SEED)
    got = augment.load_train_batch_device(data, [(video, i) for i in ids], h, w, rng, NAMES, decode="host", workers=4)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)
    ref = random.Random(SEED)
    augment.draw_params(ref, NAMES, 12, h, w)
    assert rng.getstate() == ref.getstate()
    # batch 1, frame by frame with one rng: what `_frame_batch` of the host path does
    rng = random.Random(SEED)
    for i in ids[:4]:
        one = augment.load_train_batch_device(data, [(video, i)], h, w, rng, NAMES, decode="host")
        assert np.array_equal(one.cpu().numpy()[0], want[i]), i
    # the angles a uniform draw (almost) never gives, contrast on everywhere
    angles = [0.0, 90.0, -90.0, 180.0, 89.999999, -89.999999, 1e-9, 45.0]
    randoms = [v for fl in [(0.9, 0.9), (0.1, 0.9), (0.9, 0.1), (0.1, 0.1)] * 2 for v in (fl[0], fl[1], 0.2)]
    want = drivers.load_train_frames_u8(data, video, ids[:8], h, w, Scripted(randoms, angles), NAMES)
    got = augment.load_train_batch_device(data, [(video, i) for i in ids[:8]], h, w, Scripted(randoms, angles), NAMES, decode="host")
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("names", [NAMES, ["hflip", "contrast", "vflip"], ["rot90", "vflip", "hflip"]])
@pytest.mark.parametrize("h,w", SIZES)
def test_each_kernel_equals_its_reference_stage(cuda, h, w, names):
    b = 6
    x = _frames(b, h, w)
    p = augment.draw_params(random.Random(SEED), names, b, h, w)
    ref = augment.reference_u8(x, p, stages=True)
    xd = torch.from_numpy(x).to(cuda)
    table = torch.from_numpy(p.table).to(cuda)
    hc, wc = augment.canvas_dims(p)
    # the LUTs
    luts = augment.channel_luts_device(xd, table)
    assert np.array_equal(luts.cpu().numpy(), ref["luts"])
    assert np.array_equal(ref["luts"][1 % b, 1], np.arange(256))      # (the constant channel: identity)
    # the canvas, zero fill included, from the REFERENCE's LUTs
    canvas = augment.flip_lut_rotate_device(xd, torch.from_numpy(ref["luts"]).to(cuda), table, hc, wc)
    assert np.array_equal(canvas.cpu().numpy(), ref["canvas"])
    if not p.rotated:
        assert (hc, wc) == (h, w) and np.array_equal(augment.train_transform_device(xd, p).cpu().numpy(), ref["out"])
        return
    # each resize pass from the REFERENCE's input of that pass
    ft, pool, (kh, kv) = augment.frame_tables(p, cuda)
    hp = augment.resize_pass_device(torch.from_numpy(ref["canvas"]).to(cuda), pool, ft, w, kh, 0).cpu().numpy()
    hin = np.zeros((b, hc, w, 3), np.uint8)
    for i, (nh, _) in enumerate(p.sizes()):
        assert np.array_equal(hp[i, :nh], ref["hpass"][i]), i
        hin[i, :nh] = ref["hpass"][i]
    # a launch whose LDS is sized for a narrower table than the frames' (ksize_max 1 < ksize): the coefficients come from the pool, same bytes
    hp1 = augment.resize_pass_device(torch.from_numpy(ref["canvas"]).to(cuda), pool, ft, w, 1, 0).cpu().numpy()
    assert kh > 1 and all(np.array_equal(hp1[i, :nh], ref["hpass"][i]) for i, (nh, _) in enumerate(p.sizes()))
    # an image pointer off a dword boundary is refused before any launch
    from computervision_codes_amd import ops
    cv = torch.from_numpy(ref["canvas"]).to(cuda)
    y = torch.empty((b, hc, w, 3), dtype=torch.uint8, device=cuda)
    assert ops.lib.mt4_aug_resize_pass_u8(cv.data_ptr() + 1, y.data_ptr(), pool.data_ptr(), ft.data_ptr(), b, hc, wc, hc, w, kh, 0, None) != 0
    out = augment.resize_pass_device(torch.from_numpy(hin).to(cuda), pool, ft, h, kv, 1)
    assert np.array_equal(out.cpu().numpy(), ref["out"])
    # and chained
    st = augment.train_transform_device(xd, p, stages=True)
    assert np.array_equal(st["out"].cpu().numpy(), ref["out"]) and np.array_equal(st["canvas"].cpu().numpy(), ref["canvas"])


@pytest.mark.parametrize("png_decode", ["host", "device"])
def test_frame_batch_device_equals_host(cuda, tmp_path, png_decode):
    from computervision_codes_amd import drivers, featfile
    data = str(tmp_path / "CholecT45")
    vids = _make_dataset(data, n_frames=3, h=64, w=96)[:6]
    labels = {v: cholect.load_labels(data, v) for v in vids}
    g = np.random.default_rng(2)
    tpred = {t: {featfile.video_key(v): g.standard_normal((3, k)).astype(np.float32) for v in vids} for t, k in (("i", 6), ("v", 10), ("t", 15))}
    tfeat = {t: {featfile.video_key(v): g.standard_normal((3, 16)).astype(np.float32) for v in vids} for t in "ivt"}
    batch = [(v, i) for i in (2, 0, 1) for v in vids]
    outs = {}
    for mode in ("host", "device"):
        F = argparse.Namespace(data_dir=data, augmentation_list=NAMES, png_decode=png_decode, decode_workers=4, train_transform=mode)
        rng = random.Random(SEED * 1000003)
        outs[mode] = drivers._frame_batch(F, batch, labels, tpred, tfeat, (48, 80), rng) + (rng.getstate(),)
    (fh, lh, ph, th, sh), (fd, ld, pd, td, sd) = outs["host"], outs["device"]
    assert fh.is_cuda and fd.is_cuda and fh.dtype == fd.dtype == torch.uint8 and tuple(fd.shape) == (len(batch), 48, 80, 3)
    assert torch.equal(fh, fd) and sh == sd
    for a, b in zip(lh + ph + th, ld + pd + td):
        assert torch.equal(a, b)
    assert len(ph) == len(th) == 3


def _teacher_files(base, vids, n):
    from computervision_codes_amd import featfile
    rng = np.random.default_rng(2)
    for t, k in (("i", 6), ("v", 10), ("t", 15)):
        featfile.write_feats(str(base / "run_T" / f"k1_{t}_feats.pkl"), {v[-2:]: rng.standard_normal((n, 1536)).astype(np.float32) for v in vids})
        featfile.write_feats(str(base / "run_TP" / f"k1_{t}_pred.pkl"), {v[-2:]: rng.standard_normal((n, k)).astype(np.float32) for v in vids})


def _finite_loss(log):
    lines = [ln for ln in log.splitlines() if "Traning | lr:" in ln]
    assert len(lines) == 1, log[-800:]
    loss = float(lines[0].split("| loss")[1].split("|")[0])
    assert np.isfinite(loss), lines[0]


def _run_student(tmp_path, extra):
    tree = tmp_path / "MT4MTLKD"
    shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
    data = str(tmp_path / "CholecT45")
    vids = _make_dataset(data, n_frames=2, h=40, w=56)
    _teacher_files(tree / "0-5fold" / "data_feats", vids, 2)
    r = subprocess.run([sys.executable, "run.py", "-t", "--rates", "1", "1", "1", "--temp", "4", "--network", "resnet18", "--teacher_feat_version", "T",
                        "--teacher_pred_version", "TP", "--student_dim", "512", "--loss_type", "all", "--epochs", "1", "--batch", "8", "-l", "1e-2", "5e-3",
                        "1e-3", "--version", "S", "--val_interval", "1", "--data_dir", data, "--image_height", "32", "--image_width", "64", "--kfold", "1",
                        "--train_transform", "device"] + extra,
                       cwd=tree / "Spatial_cnn", env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    run = tree / "Spatial_cnn" / "__checkpoint__" / "run_S"
    sd = torch.load(run / "rendezvous_lcholect45-crossval_cholect1_latest.pth", map_location="cpu")
    assert all(torch.isfinite(v.float()).all() for v in sd.values())
    _finite_loss(open(run / "rendezvous_lcholect45-crossval_cholect1.log").read())
    return r.stdout


@pytest.mark.parametrize("png_decode", ["host", "device"])
def test_spatial_cnn_trainer_with_device_transform(cuda, tmp_path, png_decode):
    out = _run_student(tmp_path, ["--png_decode", png_decode])
    assert "has no device form" not in out


def test_unsupported_list_trains_through_the_host_fallback_and_says_so_once(cuda, tmp_path):
    out = _run_student(tmp_path, ["--augmentation_list", "original", "vflip", "rot90", "contrast"])
    assert out.count("--train_transform device: the augmentation list") == 1 and "has no device form" in out


def test_q2l_trainer_with_device_transform(cuda, tmp_path):
    from computervision_codes_amd import shapes, synth
    tree = tmp_path / "MT4MTLKD"
    shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
    data = str(tmp_path / "CholecT45")
    _make_dataset(data, n_frames=2, h=40, w=56)
    table = shapes.q2l_param_shapes("swin_T_224_1k", 224, 768, "t")
    up = {k[len("backbone.0."):]: v for k, v in synth.fill_from_shapes(table, seed=5).items() if k.startswith("backbone.0.")}
    up["head.weight"], up["head.bias"] = torch.zeros(1000, 768), torch.zeros(1000)
    os.makedirs(tree / "Pretrain")
    torch.save({"model": up}, tree / "Pretrain" / "swin_tiny_patch4_window7_224.pth")
    r = subprocess.run([sys.executable, "run.py", "-t", "--img_size", "224", "--backbone", "swin_T_224_1k", "--hidden_dim", "768", "--loss_type", "t",
                        "--epochs", "1", "--batch", "16", "-l", "1e-2", "5e-3", "1e-5", "--version", "T", "--val_interval", "1", "--data_dir", data,
                        "--kfold", "1", "--train_transform", "device"],
                       cwd=tree / "Spatial_transformer", env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    d = tree / "Spatial_transformer" / "__checkpoint__" / "run_T_t"
    sd = torch.load(d / "rendezvous_lcholect45-crossval_cholect1_latest.pth", map_location="cpu")
    assert [k for k in sd] == [k for k, _ in table] and all(torch.isfinite(v).all() for v in sd.values())
    _finite_loss(open(d / "rendezvous_lcholect45-crossval_cholect1.log").read())
