"""CPU: the flag table of the stage drivers (`drivers._FLAGS`, `drivers._parser`) against the defaults the entry points have always had and
against the flag lines of the shipped `MT4MTLKD/Scripts/*.sh`; the module surface the four inference models share (`statemodule.StateModule`)
with a stub and -- the Q2L and CNN rules -- the real classes with `_pack` patched out."""
import glob
import os
import re
import shlex
import types

import pytest
import torch

from computervision_codes_amd import drivers, shapes
from computervision_codes_amd.statemodule import StateModule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ("spatial_cnn", "spatial_transformer", "mstct", "tenco")


# ------------------------------------------------------------------------------------------------ flag table
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("stage", STAGES)
def test_parser_defaults_per_stage(stage, train):
    F, rest = drivers._parser(stage, train).parse_known_args(["--no_such_flag", "7", "-e"])
    assert rest == ["--no_such_flag", "7"] and F.test and not F.train                     # an unknown flag is ignored
    assert (F.loss_type, F.dtype, F.png_decode, F.kfold, F.device_batch) == ("all", "fp32", "host", 1, 512)
    assert getattr(F, "teacher_dim", None) == {"spatial_cnn": 1536, "spatial_transformer": 512}.get(stage)
    assert getattr(F, "img_size", None) == (384 if stage == "spatial_transformer" else None)
    assert getattr(F, "input_dim", None) == {"mstct": 1536, "tenco": 512}.get(stage)
    assert getattr(F, "num_clips", None) == (256 if (stage, train) == ("mstct", True) else None)
    assert getattr(F, "operand_dtype", None) == ("fp32" if train and stage != "tenco" else None)
    assert hasattr(F, "epochs") == train and hasattr(F, "warmups") == train               # the schedule flags: the trainer's parser only
    if stage == "spatial_cnn":
        assert (F.network, F.student_dim) == ("resnet18", 512)
    if stage == "spatial_transformer":
        assert (F.backbone, F.hidden_dim) == ("swin_L_384_22k", 1536) and getattr(F, "drop_path_rate", None) == (0.1 if train else None)
    if stage == "mstct":
        assert F.final_embedding_dim == 512
    if stage == "tenco":
        assert (F.num_layers_PG, F.num_layers_R, F.num_R, F.fpn, F.mask, F.output, F.hier) == (11, 10, 3, False, False, False, False)
        assert getattr(F, "mask_draw", None) == ("host" if train else None) and getattr(F, "subclip", None) == ("off" if train else None)
    if train and stage in ("spatial_cnn", "spatial_transformer"):
        assert (F.teacher_feat_version, F.teacher_pred_version, F.prefetch, F.train_transform, F.temp) == ("Q2L", "Q2LMSTCT", 0, "host", 4)
        assert F.rates == [1, 0, 0.1] and F.augmentation_list == ["original", "vflip", "hflip", "contrast", "rot90"] and F.pretrain_dir == ""


def test_every_stage_declares_a_flag_once():
    for stage in STAGES:
        names = [n for names, _ in drivers._FLAGS[stage][0] + drivers._FLAGS[stage][1] for n in names]
        assert len(names) == len(set(names)), stage


# script directory -> (stage, {script file: the parsers its line is read by})
_STAGE_OF = {"Spatial_cnn": "spatial_cnn", "Spatial_transformer": "spatial_transformer", "Temporal_mstct": "mstct", "Temporal_tenco": "tenco"}
# the flags of a script line its entry point does not declare and ignores -- the same ones as before the flag table: the reference's test.py /
# run.py -e lines carry the training flags along, `--soft_type` / `--spatialKD` are declared nowhere, and test_fold1_res2swin.sh hands the
# Swin flags to Spatial_cnn/test.py (kept as the reference has it).  (script, directory, file, train parser) -> flags
_IGNORED = {
    ("test_fold1.sh", "Spatial_cnn", "test.py", False): ["--rates", "--temp", "--soft_type"],
    ("test_fold1_res2swin.sh", "Spatial_cnn", "test.py", False): ["--rates", "--temp", "--soft_type", "--img_size", "--backbone", "--hidden_dim", "--spatialKD",
                                                                 "--epochs", "-l", "-w", "--val_interval"],
    ("train_fold1.sh", "Spatial_cnn", "run.py", False): ["--rates", "--temp", "--teacher_feat_version", "--teacher_pred_version", "--epochs", "-l", "--val_interval"],
    ("train_fold1.sh", "Spatial_cnn", "test.py", False): ["--rates", "--temp", "--epochs", "-l", "--val_interval"],
    ("train_fold1.sh", "Spatial_transformer", "run.py", False): ["--epochs", "-l", "--val_interval"],
    ("train_fold1.sh", "Spatial_transformer", "test.py", False): ["--epochs", "-l", "--val_interval"],
    ("train_fold1.sh", "Temporal_mstct", "run.py", False): ["--epochs", "-l", "-w", "--decay_rate", "--val_interval"],
    ("train_fold1.sh", "Temporal_mstct", "test.py", False): ["--epochs", "-l", "-w", "--decay_rate", "--val_interval"],
}


def _script_lines():
    """(script, directory, run.py | test.py, argv) of every python line of the shipped scripts, shell variables replaced by a value that parses"""
    out = []
    for sh in sorted(glob.glob(os.path.join(ROOT, "MT4MTLKD", "Scripts", "*.sh"))):
        directory = None
        for ln in open(sh).read().replace("\\\n", " ").splitlines():
            if ln.lstrip().startswith("#"):
                continue
            m = re.search(r'cd "\$here/\.\./(\w+)"', ln)
            directory = m.group(1) if m else directory
            m = re.search(r"\b(run|test)\.py\b(.*)$", ln)
            if m:
                tail = m.group(2).replace('"$@"', "").rstrip(" )")
                tail = re.sub(r"\$\{?(\w+)\}?", lambda mm: {"DTYPE": "fp32"}.get(mm.group(1), "1"), tail)
                out.append((os.path.basename(sh), directory, m.group(1) + ".py", shlex.split(tail)))
    return out


def test_script_flag_lines_are_parsed():
    lines = _script_lines()
    assert len(lines) == 13 and {d for _, d, _, _ in lines} == set(_STAGE_OF)
    for sh, directory, py, argv in lines:
        stage = _STAGE_OF[directory]
        # run.py -t: the trainer's parser, and with -e the evaluation's reads the same line; Temporal_tenco/run.py has the one parser
        parsers = [True] if stage == "tenco" else ([True, False] if "-t" in argv else [False])
        for train in parsers:
            F, rest = drivers._parser(stage, train).parse_known_args(argv)
            ignored = [t.split("=")[0] for t in rest if re.match(r"-{1,2}[A-Za-z]", t)]
            assert ignored == _IGNORED.get((sh, directory, py, train), []), (sh, directory, py, train, rest)
            given = {t.split("=")[0] for t in argv if re.match(r"--[A-Za-z]", t)} - set(ignored)
            assert all(hasattr(F, g[2:]) for g in given), (sh, directory, py, given)


# ------------------------------------------------------------------------------------------------ module surface
class Stub(StateModule):
    def __init__(self):
        self._table = [(f"l{i}.weight", (2, 3)) for i in range(6)]
        self._sd, self.packs, self.training = {}, 0, True

    def _pack(self):
        self.packs += 1


def _zeros(table, dtype=torch.float32):
    return {k: torch.zeros(tuple(s), dtype=dtype) for k, s in table}


def test_stub_surface_and_errors():
    m = Stub()
    assert m.eval() is m and m.training is False and m.cuda() is m and m.state_dict() == {}
    sd = _zeros(m._table, torch.float64)
    assert m.load_state_dict(sd) is m and m.packs == 1
    got = m.state_dict()
    assert list(got) == [k for k, _ in m._table] and all(v.dtype == torch.float32 for v in got.values())
    got.clear()
    assert len(m.state_dict()) == 6                                                        # (a copy of the dict)
    with pytest.raises(KeyError) as e:                                                     # missing: the first four names
        Stub().load_state_dict({"l5.weight": sd["l5.weight"]})
    assert "missing ['l0.weight', 'l1.weight', 'l2.weight', 'l3.weight'], unexpected []" in str(e.value)
    with pytest.raises(KeyError) as e:                                                     # unexpected: the first four names
        Stub().load_state_dict({**sd, **{f"x{i}": torch.zeros(1) for i in range(5)}})
    assert "missing [], unexpected ['x0', 'x1', 'x2', 'x3']" in str(e.value)
    with pytest.raises(ValueError) as e:
        Stub().load_state_dict({**sd, "l2.weight": torch.zeros(3, 2)})
    assert str(e.value) == "l2.weight: shape (3, 2) != (2, 3)"
    with pytest.raises(ValueError):                                                        # ... also without strict
        Stub().load_state_dict({"l2.weight": torch.zeros(3, 2)}, strict=False)


def test_stub_non_strict_loads_the_subset():
    m = Stub().load_state_dict(_zeros(Stub()._table))
    part = {"l1.weight": torch.ones(2, 3), "l4.weight": torch.full((2, 3), 2.0), "other": torch.zeros(7)}
    m.load_state_dict(part, strict=False)
    got = m.state_dict()
    assert m.packs == 2 and list(got) == [k for k, _ in m._table] and "other" not in got
    assert [float(got[f"l{i}.weight"].sum()) for i in range(6)] == [0.0, 6.0, 0.0, 0.0, 12.0, 0.0]
    fresh = Stub().load_state_dict(part, strict=False)
    assert sorted(fresh.state_dict()) == ["l1.weight", "l4.weight"]


def test_q2l_accepts_aliases_and_swin_buffers_under_strict(monkeypatch):
    from computervision_codes_amd.spatial_transformer import Qeruy2Label
    monkeypatch.setattr(Qeruy2Label, "_pack", lambda self: None)
    args = types.SimpleNamespace(backbone="swin_T_224_1k", img_size=224, hidden_dim=768, loss_type="all", teacher_dim=64)
    m = Qeruy2Label(args)
    sd = _zeros(shapes.q2l_param_shapes("swin_T_224_1k", 224, 768, "all", teacher_dim=64), torch.bfloat16)
    aliases = shapes.q2l_state_dict_aliases(768)
    sd.update({a: sd[s] for a, s in aliases})
    sd.update({"backbone.0.layers.0.blocks.1.attn_mask": torch.zeros(4), "backbone.0.layers.0.blocks.0.attn.relative_position_index": torch.zeros(4),
               "decoder_i.pe": torch.zeros(4)})
    m.load_state_dict(sd, strict=True)
    got = m.state_dict()
    assert list(got) == [k for k, _ in m._table] and all(v.dtype == torch.float32 for v in got.values()) and aliases[0][0] not in got
    with pytest.raises(KeyError) as e:
        m.load_state_dict({**sd, "decoder_i.fc.extra": torch.zeros(1)})
    assert "missing [], unexpected ['decoder_i.fc.extra']" in str(e.value)
    del sd[aliases[0][1]]                                                                  # the source of an alias is a parameter of the table
    with pytest.raises(KeyError):
        m.load_state_dict(sd)


def test_cnn_keeps_the_checkpoint_dtype_and_drops_its_trainer(monkeypatch):
    from computervision_codes_amd.spatial_cnn import VideoNas
    monkeypatch.setattr(VideoNas, "_pack", lambda self: None)
    m = VideoNas(args=types.SimpleNamespace(network="resnet18", loss_type="all", student_dim=512, teacher_dim=1536, train=False))
    sd = _zeros(shapes.spatial_cnn_shapes("resnet18"))
    sd["basemodel.basemodel.conv1.weight"] = sd["basemodel.basemodel.conv1.weight"].bfloat16()
    sd["basemodel.basemodel.bn1.num_batches_tracked"] = torch.tensor(3)
    m._trainer = object()
    m.load_state_dict(sd)
    got = m.state_dict()
    assert m._trainer is None and got["basemodel.basemodel.conv1.weight"].dtype == torch.bfloat16
    assert got["basemodel.basemodel.bn1.num_batches_tracked"].dtype == torch.int64 and got["basemodel.basemodel.bn1.weight"].dtype == torch.float32
    with pytest.raises(KeyError):                                                          # no key is tolerated here
        m.load_state_dict({**sd, "basemodel.basemodel.layer1.0.attn_mask": torch.zeros(1)})
    m._trainer = object()
    m.load_state_dict({"wi.bias": sd["wi.bias"]}, strict=False)
    assert m._trainer is None


def test_temporal_models_store_fp32(monkeypatch):
    from computervision_codes_amd import temporal_mstct, temporal_tenco
    monkeypatch.setattr(temporal_mstct.VideoNas, "_pack", lambda self: None)
    monkeypatch.setattr(temporal_tenco.VideoNas, "_pack", lambda self: None)
    ms = temporal_mstct.VideoNas(types.SimpleNamespace(loss_type="v"), *drivers._MSTCT_ARCH, 64, 512)
    tc = temporal_tenco.VideoNas(types.SimpleNamespace(fpn=True, output=False, hier=False), 5, 4, 3, 64, 64, 100)
    for m in (ms, tc):
        sd = _zeros(m._table, torch.bfloat16)
        assert all(v.dtype == torch.float32 for v in m.load_state_dict(sd).state_dict().values()) and len(m.state_dict()) == len(m._table)
        with pytest.raises(KeyError):
            m.load_state_dict({**sd, "decoder_i.transformer.x": torch.zeros(1)})          # (Q2L's tolerance is Q2L's alone)
        first = m._table[0][0]
        with pytest.raises(KeyError):
            m.load_state_dict({k: v for k, v in sd.items() if k != first})
