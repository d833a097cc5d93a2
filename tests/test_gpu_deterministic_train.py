"""GPU: `TencoTrainer(deterministic=True)` and `SpatialCnnTrainer(deterministic=True)` -- a step is a pure function of its inputs: two independently built trainers, eager or replayed as a
hipGraph, give the same loss floats, the same parameters and the same gradients bit for bit, at a length where the weight gradients split over
workgroups; the mode still meets the reference-autograd fixtures at the default mode's tolerances; and separate `run.py -t --deterministic` processes
of both stages log the same losses and write the same checkpoint bytes -- for the student also between the host and the device data path."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_train as tg
import test_gpu_train2d as t2
from computervision_codes_amd import cholect, shapes, synth
from conftest import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _det_trainer(cfg):
    """`test_gpu_train._trainer` with the mode on"""
    from computervision_codes_amd.tenco_train import TencoTrainer
    table = shapes.tenco_shapes(cfg["num_layers_PG"], cfg["num_layers_R"], cfg["num_R"], cfg["num_f_maps"], cfg["dim"], 100, fpn=True)
    sd = synth.fill_from_shapes(table, seed=cfg["seed"])
    tr = TencoTrainer(cfg["num_layers_PG"], cfg["num_layers_R"], cfg["num_R"], cfg["num_f_maps"], cfg["dim"], lr=cfg["lr"], weight_decay=1e-5,
                      hier=bool(cfg.get("hier", False)), deterministic=True)
    return tr.load_state_dict(sd), sd, table


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("hier", [False, True], ids=["flat", "hier"])
def test_two_trainers_and_graph_replay_give_the_same_bits(cuda, hier):
    """the `tenco_train_small` configuration at 600 frames (levels of 600 / 198 / 64 / 20 with --hier): 600 rows split three ways"""
    from computervision_codes_amd import ops
    _, cfg = load_golden("tenco_train_small")
    cfg = dict(cfg, T=600, hier=hier)
    c = cfg["num_f_maps"]
    assert ops.wgrad_conv1d_plan(1, 600, c, c, 3, True).nparts == 3 and ops.wgrad_conv1d_plan(1, 600, c, c, 1, True).nparts == 3
    x = synth.synthetic_features(cfg["T"], cfg["dim"], seed=cfg["seed"]).to(cuda)
    labels = tg._labels(cfg["seed"], cfg["T"])
    a, b, g = _det_trainer(cfg)[0], _det_trainer(cfg)[0], _det_trainer(cfg)[0]
    assert a._ws is not None and a._ws.numel() * 4 == a.workspace_bytes() and a._ws.data_ptr() != b._ws.data_ptr()
    for step in range(2):
        ra = a.train_step(x, labels, draws=(41, step))
        rb = b.train_step(x, labels, draws=(41, step))
        rg = g.train_step(x, labels, draws=(41, step), use_graph=True)
        assert ra == rb == rg, (step, ra, rb, rg)                       # (loss, {head: term}) as floats
        assert torch.equal(a.G, b.G) and torch.equal(a.G, g.G) and torch.equal(a.P, b.P) and torch.equal(a.P, g.P), step
    assert len(g._graphs) == 1
    _same(a.state_dict(), b.state_dict())
    _same(a.state_dict(), g.state_dict())
    _same(a.grads(), b.grads())
    _same(a.grads(), g.grads())
    # explicit masks: the other way to pin the draw
    masks = a.draw_masks(cfg["T"], torch.Generator().manual_seed(5))
    assert a.train_step(x, labels, masks=masks) == b.train_step(x, labels, masks=masks) and torch.equal(a.P, b.P) and torch.equal(a.G, b.G)


@pytest.mark.parametrize("name", ["tenco_train_small", "tenco_train_hier"])
def test_deterministic_step_meets_the_reference_autograd_fixture(cuda, monkeypatch, name):
    """the assertions of `test_gpu_train.test_train_step_vs_reference_autograd`, its trainer built with deterministic=True"""
    built = []

    def trainer(cfg):
        built.append(_det_trainer(cfg))
        return built[-1]
    monkeypatch.setattr(tg, "_trainer", trainer)
    tg.test_train_step_vs_reference_autograd(cuda, name)
    assert len(built) == 1 and built[0][0].deterministic and built[0][0]._ws is not None


# ------------------------------------------------------------------------------------------------ the driver
def _make_temporal_dataset(tree, data, n_frames):
    """label files and a feature pickle of `n_frames` frames for every video of fold 1 (the temporal stage reads no images)"""
    from computervision_codes_amd import featfile
    rng = np.random.default_rng(3)
    vids = cholect.extraction_videos("cholect45-crossval", 1)
    for sub, k in (("triplet", 100), ("instrument", 6), ("verb", 10), ("target", 15)):
        os.makedirs(os.path.join(data, sub))
        for v in vids:
            lab = np.concatenate([np.arange(n_frames)[:, None], (rng.random((n_frames, k)) < 0.15).astype(int)], 1)
            np.savetxt(os.path.join(data, sub, v + ".txt"), lab, fmt="%d", delimiter=",")
    featfile.write_feats(str(tree / "0-5fold" / "data_feats" / "run_S" / "k1_feats.pkl"),
                         {v[-2:]: rng.standard_normal((n_frames, 512)).astype(np.float32) for v in vids})


@pytest.fixture(scope="module")
def driver_runs(tmp_path_factory):
    """two processes of `Temporal_tenco/run.py -t --deterministic`, each in a tree of its own: (log text, checkpoint) per run"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = []
    for run in ("a", "b"):
        top = tmp_path_factory.mktemp("det_" + run)
        tree, data = top / "MT4MTLKD", str(top / "CholecT45")
        shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
        _make_temporal_dataset(tree, data, 300)                          # 300 rows: every weight gradient splits two ways
        r = subprocess.run([sys.executable, "run.py", "-t", "--fpn", "--mask", "--mask_draw", "device", "--deterministic", "--num_layers_PG", "3",
                            "--num_layers_R", "2", "--input_dim", "512", "--loss_type", "all", "--epochs", "2", "-l", "1e-2", "5e-3", "1e-2",
                            "-w", "9", "18", "200", "--version", "S_TCN", "--version1", "S", "--data_dir", data, "--kfold", "1", "--seed", "7"],
                           cwd=tree / "Temporal_tenco", env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        ck = tree / "Temporal_tenco" / "__checkpoint__" / "run_S_TCN" / "rendezvous_l8_cholectcholect45-crossval_k1_batchnorm_lowres_latest.pth"
        out.append((r.stdout, open(str(ck).replace("_latest.pth", ".log")).read(), torch.load(ck, map_location="cpu")))
    return out


def _loss_fields(log):
    return [ln.split("| loss ")[1].split(" |")[0] for ln in log.splitlines() if ln.startswith("Traning | lr:")]


def test_two_driver_runs_log_the_same_losses_and_write_the_same_checkpoint(driver_runs):
    from computervision_codes_amd import ops
    assert ops.wgrad_conv1d_plan(1, 300, 512, 512, 3, True).nparts == 2
    (out_a, log_a, sd_a), (out_b, log_b, sd_b) = driver_runs
    assert out_a.count("--deterministic: fixed-order sums") == 1         # said once at start
    la, lb = _loss_fields(log_a), _loss_fields(log_b)
    assert len(la) == 2 and la == lb, (la, lb)                           # string-equal, both epochs
    _same(sd_a, sd_b)


# ================================================================================================ the student trainer
def _student_class(monkeypatch, operand_dtype=torch.float32):
    """`test_gpu_train2d._trainer` builds `spatial_cnn_train.SpatialCnnTrainer`: switch the name to the class with the mode (and the operand type) on"""
    from computervision_codes_amd import spatial_cnn_train as sct
    base = sct.SpatialCnnTrainer

    class Deterministic(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **dict(k, deterministic=True, operand_dtype=operand_dtype))
    monkeypatch.setattr(sct, "SpatialCnnTrainer", Deterministic)
    return Deterministic


@pytest.mark.parametrize("network,operands", [("resnet18", torch.float32), ("resnet50", torch.float32), ("resnet50", torch.bfloat16)],
                         ids=["resnet18_fp32", "resnet50_fp32", "resnet50_bf16"])
def test_student_trainers_and_graph_replay_give_the_same_bits(cuda, monkeypatch, network, operands):
    """B = 6 uint8 frames of 64 x 96, three steps with the update: two trainers built independently from one state dict, and a third that replays
    the step as a hipGraph -- every loss term equal as a float, every tensor of state_dict() and grads() equal"""
    cls = _student_class(monkeypatch, operands)
    cfg = dict(network=network, B=6, H=64, W=96, seed=77, lr=0.05, rates=(1.0, 0.5, 2.0))
    _, labels, tpred, tfeat = t2._inputs(cfg)
    frames = synth.synthetic_frames(cfg["B"], cfg["H"], cfg["W"], seed=cfg["seed"]).to(cuda)
    assert frames.dtype == torch.uint8
    a, b, g = t2._trainer(cfg)[0], t2._trainer(cfg)[0], t2._trainer(cfg)[0]
    assert isinstance(a, cls) and a.deterministic and not a.epilogue_stats and a.op16 == (operands == torch.bfloat16)
    for step in range(3):
        ta = a.train_step(frames, labels, tpred, tfeat)
        tb = b.train_step(frames, labels, tpred, tfeat)
        tg_ = g.train_step(frames, labels, tpred, tfeat, use_graph=True)
        assert ta == tb == tg_, (step, ta, tb, tg_)
        assert torch.equal(a.G, b.G) and torch.equal(a.G, g.G) and torch.equal(a.P, b.P) and torch.equal(a.P, g.P), step
    assert a._ws is not None and a._ws.numel() * 4 >= a.workspace_bytes(6, 64, 96) and len(g._graphs) == 1
    for other in (b, g):
        _same(a.state_dict(), other.state_dict())
        _same(a.grads(), other.grads())


@pytest.mark.parametrize("name", ["cnn_train_resnet18", "cnn_train_resnet50_tiefree"])
def test_deterministic_student_step_meets_the_reference_autograd_fixture(cuda, monkeypatch, name):
    """the assertions of `test_gpu_train2d.test_train_step_vs_reference_autograd`, its trainer built with deterministic=True"""
    cls = _student_class(monkeypatch)
    built = []
    orig = cls.load_state_dict
    monkeypatch.setattr(cls, "load_state_dict", lambda self, sd: (built.append(self), orig(self, sd))[1])
    t2.test_train_step_vs_reference_autograd(cuda, name)
    assert len(built) == 1 and built[0].deterministic and built[0]._ws is not None


@pytest.fixture(scope="module")
def student_runs(tmp_path_factory):
    """three processes of `Spatial_cnn/run.py -t --network resnet18 --deterministic --png_decode device`, two epochs each on the tiny PNG dataset of
    tests/test_gpu_sharpness.py: A host transform, synchronous loader; B = A repeated; C device transform, prefetching loader, frame cache"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_sharpness as tsh
    out = {}
    for run, extra in (("A", ["--train_transform", "host", "--prefetch", "0"]), ("B", ["--train_transform", "host", "--prefetch", "0"]),
                       ("C", ["--train_transform", "device", "--prefetch", "2", "--frame_cache", "1"])):
        work = tmp_path_factory.mktemp("student_" + run)
        tree, data = work / "MT4MTLKD", str(work / "CholecT45")
        shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
        vids = tsh._make_dataset(data, n_frames=2, h=40, w=56)
        tsh._teacher_files(tree / "0-5fold" / "data_feats", vids, 2)
        r = subprocess.run([sys.executable, "run.py", "-t", "--rates", "1", "1", "1", "--temp", "4", "--network", "resnet18", "--teacher_feat_version", "T",
                            "--teacher_pred_version", "TP", "--student_dim", "512", "--loss_type", "all", "--epochs", "2", "--batch", "8", "-l", "1e-2", "5e-3",
                            "1e-3", "--version", "S", "--val_interval", "1", "--data_dir", data, "--image_height", "32", "--image_width", "64", "--kfold", "1",
                            "--deterministic", "--png_decode", "device"] + extra,
                           cwd=tree / "Spatial_cnn", env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        ck = tree / "Spatial_cnn" / "__checkpoint__" / "run_S"
        out[run] = (r.stdout, open(ck / "rendezvous_lcholect45-crossval_cholect1.log").read(),
                    torch.load(ck / "rendezvous_lcholect45-crossval_cholect1_latest.pth", map_location="cpu"))
    return out


def test_three_student_driver_runs_log_the_same_losses_and_write_the_same_checkpoint(student_runs):
    """what a user sees: the `Traning |` loss fields of both epochs string-equal and every tensor of `_latest.pth` equal -- between a run and its
    repetition, and between the host data path and the device one (transform, prefetching loader, frame cache: 'the same bytes, only faster')"""
    losses = {k: _loss_fields(v[1]) for k, v in student_runs.items()}
    assert len(losses["A"]) == 2 and losses["A"] == losses["B"] == losses["C"], losses
    assert student_runs["A"][0].count("--deterministic: fixed-order sums") == 1
    _same(student_runs["A"][2], student_runs["B"][2])
    _same(student_runs["A"][2], student_runs["C"][2])
