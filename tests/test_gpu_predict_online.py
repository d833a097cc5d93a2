"""GPU: `predict.py --online` on a dozen small frames: the chunk size does not change a bit of the output, the scores agree with the offline
--causal run, and without --causal predict.py says and computes what it did before the flag existed."""
import os

import numpy as np
import pytest
import torch

from computervision_codes_amd import drivers, shapes, synth

pytestmark = pytest.mark.gpu
H, W, N_FRAMES, K = 64, 96, 12, 5
HEADS = ("ivt", "i", "v", "t")


def _load(stem):
    with np.load(stem + ".npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(cuda, tmp_path_factory):
    """12 random PNGs, the smallest student (ResNet-18) and a 3 / 2 / 3-stage head; ONE run of each mode"""
    from PIL import Image
    tmp = tmp_path_factory.mktemp("online")
    frames = tmp / "clip"
    os.makedirs(frames)
    rng = np.random.default_rng(5)
    for i in range(N_FRAMES):
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(frames / f"{i:06d}.png")
    student, temporal = str(tmp / "student.pth"), str(tmp / "temporal.pth")
    torch.save(synth.fill_from_shapes(shapes.spatial_cnn_shapes("resnet18"), seed=11), student)
    torch.save(synth.fill_from_shapes(shapes.tenco_shapes(3, 2, 3, 512, 512, 100, fpn=True), seed=12), temporal)
    common = ["--frames_dir", str(frames), "--student_ckpt", student, "--temporal_ckpt", temporal, "--image_height", str(H), "--image_width", str(W),
              "--fpn", "--input_dim", "512", "--num_layers_PG", "3", "--num_layers_R", "2", "--topk", str(K), "--save_scores"]
    out = {}
    for name, extra in (("plain", []), ("causal", ["--causal"]), ("online1", ["--causal", "--online"]),
                        ("online5", ["--causal", "--online", "--online_chunk", "5"])):
        drivers.predict(common + extra + ["--out", str(tmp / name)])
        out[name] = str(tmp / name / "clip")
    return dict(out=out, common=common, tmp=tmp, student=student, temporal=temporal, frames=str(frames))


def test_chunk_size_does_not_change_a_bit(runs):
    a, b = _load(runs["out"]["online1"]), _load(runs["out"]["online5"])
    assert sorted(a) == sorted(b) and a["topk_ids"].shape == (N_FRAMES, K) and a["scores_ivt"].shape == (N_FRAMES, 100)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert open(runs["out"]["online1"] + ".csv").read() == open(runs["out"]["online5"] + ".csv").read()
    assert [str(f) for f in a["frames"]] == [f"{i:06d}.png" for i in range(N_FRAMES)]


def test_online_scores_agree_with_the_offline_causal_run(runs):
    on, off = _load(runs["out"]["online1"]), _load(runs["out"]["causal"])
    assert sorted(on) == sorted(off)                      # the files of the offline run
    for h in HEADS:
        err = float(np.abs(on[f"scores_{h}"] - off[f"scores_{h}"]).max())
        print(f"{h}: online - offline scores {err:.3e}")
        assert err < 1e-3, h


def test_online_log_line_reports_chunk_latencies(runs, capsys):
    drivers.predict(runs["common"] + ["--causal", "--online", "--online_chunk", "5", "--out", str(runs["tmp"] / "again")])
    out = capsys.readouterr().out
    assert "--causal:" in out and "online, 5 frames per chunk: median" in out and "max" in out


def test_without_causal_nothing_changes(runs, capsys):
    """the default run: no new line, and the scores of the symmetric head computed the way the driver did before (`Predictor.logits`: the
    whole-video forward of a model built without the `causal` argument) -- which the causal head's are not"""
    from computervision_codes_amd import predict as P
    from computervision_codes_amd.temporal_tenco import VideoNas
    F = drivers._predict_parser().parse_known_args(runs["common"])[0]
    assert F.causal is False and F.online is False
    F.test_ckpt = None
    student = drivers._eval_model("spatial_cnn", F, [runs["student"]])
    sd = torch.load(runs["temporal"], map_location="cpu")
    temporal = VideoNas(F, 3, 2, 3, 512, 512, 100).eval().load_state_dict(sd)
    paths = [os.path.join(runs["frames"], f) for f in sorted(os.listdir(runs["frames"]))]
    want = P.Predictor(student, temporal, height=H, width=W, topk=K).predict_paths(paths, keep_scores=True)._arrays()
    capsys.readouterr()
    drivers.predict(runs["common"] + ["--out", str(runs["tmp"] / "plain2")])
    out = capsys.readouterr().out
    assert "causal" not in out and "online" not in out and len(out.strip().splitlines()) == 1
    got = _load(runs["out"]["plain"])
    assert sorted(got) == sorted(want)
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    assert not np.array_equal(got["scores_ivt"], _load(runs["out"]["causal"])["scores_ivt"])
