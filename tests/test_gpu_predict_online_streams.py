"""GPU: `predict.py --online --online_streams S` on three small videos of different lengths (the tiny frames and checkpoints of
test_gpu_predict_online.py): answering them two or three at a time writes the bytes of answering them one after another, and says so in one
closing line; without the flag the log is what it was."""
import os

import numpy as np
import pytest
import torch

from computervision_codes_amd import drivers, shapes, synth
from test_gpu_predict_online import H, K, W, _load

pytestmark = pytest.mark.gpu
LENGTHS = {"clip_a": 12, "clip_b": 7, "clip_c": 3}
MODES = {"one": ["--online_chunk", "5"], "two": ["--online_chunk", "5", "--online_streams", "2"], "three": ["--online_streams", "3", "--online_chunk", "1"]}


@pytest.fixture(scope="module")
def runs(cuda, tmp_path_factory):
    """random PNGs, the smallest student (ResNet-18) and a 3 / 2 / 3-stage head; ONE run of each mode, its log kept"""
    from PIL import Image
    tmp = tmp_path_factory.mktemp("online_streams")
    rng = np.random.default_rng(6)
    dirs = []
    for name, n in LENGTHS.items():
        os.makedirs(tmp / name)
        for i in range(n):
            Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(tmp / name / f"{i:06d}.png")
        dirs += ["--frames_dir", str(tmp / name)]
    student, temporal = str(tmp / "student.pth"), str(tmp / "temporal.pth")
    torch.save(synth.fill_from_shapes(shapes.spatial_cnn_shapes("resnet18"), seed=11), student)
    torch.save(synth.fill_from_shapes(shapes.tenco_shapes(3, 2, 3, 512, 512, 100, fpn=True), seed=12), temporal)
    common = dirs + ["--student_ckpt", student, "--temporal_ckpt", temporal, "--image_height", str(H), "--image_width", str(W), "--fpn",
                     "--input_dim", "512", "--num_layers_PG", "3", "--num_layers_R", "2", "--topk", str(K), "--save_scores", "--segments",
                     "--causal", "--online"]
    return dict(tmp=tmp, common=common)


@pytest.fixture(scope="module")
def logs(runs):
    import contextlib
    import io
    out = {}
    for mode, extra in MODES.items():
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = drivers.predict(runs["common"] + extra + ["--out", str(runs["tmp"] / mode)])
        assert list(res) == list(LENGTHS)
        out[mode] = buf.getvalue()
    return out


@pytest.mark.parametrize("mode", ["two", "three"])
def test_several_streams_write_the_bytes_of_one(runs, logs, mode):
    for name, n in LENGTHS.items():
        a, b = _load(str(runs["tmp"] / "one" / name)), _load(str(runs["tmp"] / mode / name))
        assert sorted(a) == sorted(b) and a["topk_ids"].shape == (n, K) and a["scores_ivt"].shape == (n, 100)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (name, k)
        for ext in (".csv", ".segments.csv"):
            assert open(runs["tmp"] / "one" / (name + ext)).read() == open(runs["tmp"] / mode / (name + ext)).read(), (name, ext)


def test_log_lines(logs):
    one = logs["one"].strip().splitlines()
    assert "online_streams" not in logs["one"] and "streams" not in logs["one"] and "tick" not in logs["one"]
    assert len(one) == 1 + len(LENGTHS) and "--causal:" in one[0]                           # what --online said before the flag existed
    # two at a time, five frames each: 5 + 5, 5 + 2 (clip_b ends, clip_c opens), 2 + 3; three at a time, one frame each: 3 x 3, 4 x 2, 5 x 1
    for mode, s, ticks, per_tick in (("two", 2, 3, 7), ("three", 3, 12, 2)):
        lines = logs[mode].strip().splitlines()
        assert len(lines) == 2 + len(LENGTHS)
        for name, n in LENGTHS.items():
            (ln,) = [x for x in lines if x.startswith(name + ":")]
            assert f"{name}: {n} frames |" in ln and "frames per chunk: median" in ln and "ms per chunk" in ln
        assert lines[-1].startswith(f"online, {s} streams: {ticks} ticks | median ") and " ms per tick | " in lines[-1] and "max " in lines[-1]
        assert lines[-1].endswith(f"median {per_tick} frames per tick")
