"""GPU: `predict.py --localize` on two small videos (96 x 160 frames: a 3 x 5 layer4 grid; the smallest student): the saved localisation arrays
are `ops.class_maps` on the map `extract_u8(..., return_map=True)` hands out, gathered by the saved top-K; every online mode writes the bytes of
the whole-video run; the maps average to the logits; `extract_u8` without the argument is what it was; the command line writes the files."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from computervision_codes_amd import cholect, drivers, ops, shapes, synth
from computervision_codes_amd import predict as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, K, FRAC = 96, 160, 5, 0.4
CELLS = (3, 5)
LENGTHS = {"clip_a": 7, "clip_b": 4}
LOC = ("loc_peak", "loc_box", "loc_area", "loc_range", "loc_maps")
U = 2.0 ** -24


def _load(stem):
    with np.load(stem + ".npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("localize")
    rng = np.random.default_rng(8)
    dirs = []
    for name, n in LENGTHS.items():
        os.makedirs(tmp / name)
        for i in range(n):
            Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(tmp / name / f"{i:06d}.png")
        dirs += ["--frames_dir", str(tmp / name)]
    student, temporal = str(tmp / "student.pth"), str(tmp / "temporal.pth")
    torch.save(synth.fill_from_shapes(shapes.spatial_cnn_shapes("resnet18"), seed=11), student)
    torch.save(synth.fill_from_shapes(shapes.tenco_shapes(3, 2, 3, 512, 512, 100, fpn=True), seed=12), temporal)
    base = dirs + ["--student_ckpt", student, "--image_height", str(H), "--image_width", str(W), "--topk", str(K), "--localize_frac", str(FRAC),
                   "--save_maps"]
    head = ["--temporal_ckpt", temporal, "--fpn", "--input_dim", "512", "--num_layers_PG", "3", "--num_layers_R", "2", "--causal"]
    F = drivers._predict_parser().parse_known_args(base)[0]
    F.test_ckpt = None
    model = drivers._eval_model("spatial_cnn", F, [student])
    frames = {name: cholect.load_files_device([str(tmp / name / f"{i:06d}.png") for i in range(n)], H, W) for name, n in LENGTHS.items()}
    return dict(tmp=tmp, base=base, head=head, model=model, frames=frames, student=student, dirs=dirs)


@pytest.fixture(scope="module")
def runs(world):
    """ONE run of every mode and localising head: the student's own heads, the whole-video causal head, and the online modes on that head"""
    out = {}
    for loc in ("i", "ivt"):
        for mode, extra in (("student", []), ("whole", world["head"]), ("online1", world["head"] + ["--online"]),
                            ("online3", world["head"] + ["--online", "--online_chunk", "3"]),
                            ("streams2", world["head"] + ["--online", "--online_chunk", "3", "--online_streams", "2"])):
            d = str(world["tmp"] / f"{mode}_{loc}")
            drivers.predict(world["base"] + extra + ["--localize", loc, "--out", d])
            out[mode, loc] = {name: _load(os.path.join(d, name)) for name in LENGTHS}
    return out


@pytest.mark.parametrize("loc", ["i", "ivt"])
@pytest.mark.parametrize("mode", ["student", "whole"])
def test_saved_arrays_are_class_maps_of_the_returned_map_gathered_by_the_saved_topk(world, runs, mode, loc):
    model = world["model"]
    lo, hi = model._head_slices[loc]
    for name, n in LENGTHS.items():
        z = runs[mode, loc][name]
        _, fmap = model.extract_u8(world["frames"][name], return_map=True)
        assert tuple(fmap.shape) == (n,) + CELLS + (512,) and fmap.dtype == torch.float32
        maps, regions, rng = (t.cpu().numpy() for t in ops.class_maps(fmap, model._p["heads.rows"], lo, hi - lo, FRAC))
        cols = z["topk_ids"] if loc == "ivt" else z["topk_ivt"][..., 0]
        assert cols.shape == (n, K) and cols.min() >= 0 and cols.max() < hi - lo
        rows = np.arange(n)[:, None]
        assert np.array_equal(z["loc_maps"], maps[rows, cols]) and z["loc_maps"].shape == (n, K) + CELLS
        assert np.array_equal(z["loc_peak"], regions[rows, cols][..., 0:2]) and np.array_equal(z["loc_box"], regions[rows, cols][..., 2:6])
        assert np.array_equal(z["loc_area"], regions[rows, cols][..., 6]) and np.array_equal(z["loc_range"], rng[rows, cols])
        assert tuple(z["loc_cells"]) == CELLS and tuple(z["loc_frame"]) == (H, W) and str(z["loc_head"]) == loc and float(z["loc_frac"]) == FRAC
        assert np.array_equal(z["loc_range"][..., 1], z["loc_maps"].max(axis=(2, 3))) and np.array_equal(z["loc_range"][..., 0], z["loc_maps"].min(axis=(2, 3)))
        want_r, want_g = ops.class_regions_host(z["loc_maps"], FRAC)
        assert np.array_equal(want_r[..., 0:2], z["loc_peak"]) and np.array_equal(want_r[..., 2:6], z["loc_box"]) and np.array_equal(want_g, z["loc_range"])


@pytest.mark.parametrize("loc", ["i", "ivt"])
@pytest.mark.parametrize("mode", ["online1", "online3", "streams2"])
def test_online_modes_write_the_bytes_of_the_whole_video_run(runs, mode, loc):
    for name in LENGTHS:
        a, b = runs["whole", loc][name], runs[mode, loc][name]
        assert sorted(a) == sorted(b)
        assert np.array_equal(a["topk_ids"], b["topk_ids"]), "the two runs rank differently: their localisation rows are of different columns"
        for k in LOC + ("loc_cells", "loc_frame", "loc_head", "loc_frac"):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)
    for name in LENGTHS:                                                                   # and the chunk size / the bank change no byte of any array
        a, b = runs["online1", loc][name], runs[mode, loc][name]
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_maps_average_to_the_students_logits(world):
    """student-only, fp32.  Both sides are roundings of S = mean_p sum_k W[c, k] F[p, k] + b_c, evaluated here in float64 from the returned map:
      the maps' side   mean (in float64) of map cells, each an fp32 inner product of length C: |A - S| <= gamma_C * Abs,
                       Abs = mean_p sum_k |W[c, k] F[p, k]|;
      the logit        an fp32 mean over h w cells (h w - 1 additions and the scaling: gamma_(hw + 1) on mean_p |F|), an fp32 inner product of
                       length C with the weights (gamma_C) and the bias addition (one rounding): |B - S| <= gamma_(C + hw + 2) * (Abs + |b_c|),
    gamma_n = n u / (1 - n u), u = 2^-24 (Higham 3.1, 3.4: the factors compose as gamma_a + gamma_b + gamma_a gamma_b <= gamma_(a + b)); whatever
    order either kernel sums in.  |A - B| is then within the sum of the two."""
    model = world["model"]
    pr = P.Predictor(model, None, height=H, width=W, topk=K, localize="ivt", localize_frac=FRAC, localize_maps=True)
    name, n = "clip_a", LENGTHS["clip_a"]
    pred = pr.predict_paths([str(world["tmp"] / name / f"{i:06d}.png") for i in range(n)])
    out, fmap = model.extract_u8(world["frames"][name], return_map=True)
    logits = out[3][1].cpu().numpy().astype(np.float64)                                    # [n, 100]
    lo, hi = model._head_slices["ivt"]
    w64, b64 = model._p["heads.rows"][lo:hi].double(), model._p["heads.b"][lo:hi].double().cpu().numpy()
    f64 = fmap.double().reshape(n, -1, 512)
    s64 = (torch.einsum("npk,ck->nc", f64, w64) / f64.shape[1]).cpu().numpy() + b64
    abs64 = (torch.einsum("npk,ck->nc", f64.abs(), w64.abs()) / f64.shape[1]).cpu().numpy()
    rows, ids = np.arange(n)[:, None], pred.topk_ids
    c, hw = 512, CELLS[0] * CELLS[1]
    gamma = lambda m: m * U / (1.0 - m * U)
    a = pred.loc_maps.astype(np.float64).mean(axis=(2, 3)) + b64[ids]
    b = logits[rows, ids]
    bound_a = gamma(c) * abs64[rows, ids] + 2.0 ** -50 * (np.abs(s64[rows, ids]) + abs64[rows, ids])      # (+ the float64 mean and additions of this test)
    bound_b = gamma(c + hw + 2) * (abs64[rows, ids] + np.abs(b64[ids]))
    print(f"maps side: max |A - S| / bound {float((np.abs(a - s64[rows, ids]) / bound_a).max()):.3f}; logit side: max |B - S| / bound "
          f"{float((np.abs(b - s64[rows, ids]) / bound_b).max()):.3f}; max |A - B| {float(np.abs(a - b).max()):.3e}")
    assert (np.abs(a - s64[rows, ids]) <= bound_a).all()
    assert (np.abs(b - s64[rows, ids]) <= bound_b).all()
    assert (np.abs(a - b) <= bound_a + bound_b).all()
    assert np.array_equal(pred.topk_scores, torch.sigmoid(torch.from_numpy(logits[rows, ids]).float()).numpy())    # (the logits ARE this run's)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_extract_u8_without_return_map_is_unchanged(world, dtype):
    F = drivers._predict_parser().parse_known_args(world["base"] + (["--dtype", "bf16"] if dtype == torch.bfloat16 else []))[0]
    F.test_ckpt = None
    model = drivers._eval_model("spatial_cnn", F, [world["student"]]) if dtype == torch.bfloat16 else world["model"]
    fr = world["frames"]["clip_a"]
    plain = model.extract_u8(fr)
    with_map, fmap = model.extract_u8(fr, return_map=True)
    assert fmap.dtype == dtype and tuple(fmap.shape) == (fr.shape[0],) + CELLS + (512,) and fmap.is_contiguous()
    for (a0, a1), (b0, b1) in zip(plain, with_map):
        assert torch.equal(a1, b1)
        assert torch.equal(a0, b0) if torch.is_tensor(a0) else a0 == b0
    assert torch.equal(with_map[3][0], ops.global_avgpool(fmap))                           # exactly the tensor that was pooled
    again = model.extract_u8(fr, streams=2)
    assert torch.equal(again[3][1], plain[3][1]) and torch.equal(again[3][0], plain[3][0])
    with pytest.raises(ValueError, match="return_map"):
        model.extract_u8(fr, streams=2, return_map=True)


def test_command_line_writes_the_files_with_the_flag_and_todays_files_without(world):
    env = dict(os.environ, PYTHONPATH=ROOT)
    script = os.path.join(ROOT, "MT4MTLKD", "predict.py")
    argv = [a for a in world["base"] if a != "--save_maps"]
    today = sorted(["frames", "threshold", "topk_ids", "topk_scores", "n_active", "topk_ivt"] + [f"top_{h}_{w}" for h in "ivt" for w in ("ids", "scores")])
    loc_keys = ["loc_peak", "loc_box", "loc_area", "loc_range", "loc_cells", "loc_frame", "loc_head", "loc_frac"]
    with_flag, without = str(world["tmp"] / "cli_loc"), str(world["tmp"] / "cli_plain")
    r = subprocess.run([sys.executable, script] + argv + ["--localize", "i", "--out", with_flag], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "--localize i: each top-K triplet is localised by the student's instrument head" in r.stdout
    r0 = subprocess.run([sys.executable, script] + argv + ["--out", without], env=env, capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0, r0.stdout[-2000:] + r0.stderr[-2000:]
    assert "localize" not in r0.stdout and "localis" not in r0.stdout
    for name, n in LENGTHS.items():
        z = _load(os.path.join(with_flag, name))
        assert sorted(z) == sorted(today + loc_keys) and z["loc_peak"].shape == (n, K, 2) and z["loc_box"].shape == (n, K, 4)
        rows = open(os.path.join(with_flag, name + ".loc.csv")).read().splitlines()
        assert rows[0] == "frame,rank,triplet,column,peak_x,peak_y,x0,y0,x1,y1,area" and len(rows) - 1 == n * K
        first = rows[1].split(",")
        assert first[:3] == ["000000.png", "0", str(int(z["topk_ids"][0, 0]))] and first[3] == str(int(z["topk_ivt"][0, 0, 0]))
        assert float(first[4]) == (z["loc_peak"][0, 0, 1] + 0.5) * W / CELLS[1] and float(first[9]) == (z["loc_box"][0, 0, 2] + 1) * H / CELLS[0]
        z0 = _load(os.path.join(without, name))
        assert sorted(z0) == today and not os.path.exists(os.path.join(without, name + ".loc.csv"))
        for k in today:
            assert z0[k].tobytes() == z[k].tobytes(), (name, k)                            # the flag changes no byte of what was there
        assert open(os.path.join(without, name + ".csv")).read() == open(os.path.join(with_flag, name + ".csv")).read()
