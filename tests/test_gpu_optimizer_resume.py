"""GPU: --resume with optimizer state through `Temporal_tenco/run.py -t --deterministic`, at the configuration tests/test_gpu_resume.py uses for
that stage: four epochs straight against two plus two, once with --momentum 0.9 and once with --optimizer adamw -- the same logged losses, the
same `_latest.pth` and best `.pth` bytes, the same final optimizer file bytes.  A resumed run whose momentum restarted at zero would end
elsewhere: that is the failure this test exists to catch.  A resume with the other rule's flags is refused before a model is built."""
import os
import shutil
import subprocess
import sys

import pytest
import torch

import test_gpu_deterministic_train as td
from test_gpu_resume import TENCO_NAME, TENCO_SEED, _assert_resumed_equals_straight, _bytes, _epochs, _files

pytestmark = pytest.mark.gpu
ROOT = td.ROOT
RULES = {"momentum": ["--momentum", "0.9"], "adamw": ["--optimizer", "adamw"]}


def _argv(data, epochs, rule):
    return ["--fpn", "--mask", "--mask_draw", "device", "--subclip", "reference", "--deterministic", "--resume", "--val_interval", "1",
            "--num_layers_PG", "3", "--num_layers_R", "2", "--input_dim", "512", "--loss_type", "all", "--epochs", str(epochs),
            "-l", "1e-2", "5e-3", "1e-3", "-w", "9", "18", "1", "--decay_rate", "0.9", "--version", "S_TCN", "--version1", "S",
            "--data_dir", data, "--kfold", "1", "--seed", str(TENCO_SEED)] + rule


def _run(cwd, argv):
    return subprocess.run([sys.executable, "run.py", "-t"] + argv, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("name", list(RULES))
def test_two_plus_two_epochs_write_the_bytes_of_four(cuda, tmp_path, name):
    out, stems = {}, {}
    for run, plan in (("s", [4]), ("r", [2, 4])):
        tree, data = tmp_path / run / "MT4MTLKD", str(tmp_path / run / "CholecT45")
        shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
        td._make_temporal_dataset(tree, data, 300)
        for epochs in plan:
            r = _run(tree / "Temporal_tenco", _argv(data, epochs, RULES[name]))
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
            assert r.stdout.count("update rule:") == 1
        stems[run] = str(tree / "Temporal_tenco" / "__checkpoint__" / "run_S_TCN" / TENCO_NAME)
        out[run] = _files(stems[run])
    _assert_resumed_equals_straight(out["s"], out["r"], TENCO_NAME)
    losses = [float(v[0]) for v in _epochs(out["s"]["log"])[0].values()]
    assert all(x == x and abs(x) != float("inf") for x in losses), losses
    optim = [f for f in out["r"]["dir"] if ".optim.e" in f]
    assert optim == [TENCO_NAME + "_latest.pth.optim.e2", TENCO_NAME + "_latest.pth.optim.e3"], out["r"]["dir"]
    final = "_latest.pth.optim.e3"
    assert _bytes(stems["s"] + final) == _bytes(stems["r"] + final)
    osd = torch.load(stems["r"] + final, map_location="cpu")
    assert osd["optim"]["kind"] == ("adamw" if name == "adamw" else "sgd") and any(bool(t.any()) for st in osd["state"].values() for t in st.values())
    # the other rule's flags on this tree: refused before a model is built, the file and the way out in the message
    other = RULES["momentum" if name == "adamw" else "adamw"]
    tree = tmp_path / "r" / "MT4MTLKD"
    r = _run(tree / "Temporal_tenco", _argv(str(tmp_path / "r" / "CholecT45"), 6, other))
    assert r.returncode != 0 and "changing the update rule" in r.stderr and ".optim.e3" in r.stderr and "drop --resume" in r.stderr, r.stderr[-1500:]
    assert _files(stems["r"]) == out["r"]                             # nothing was touched
