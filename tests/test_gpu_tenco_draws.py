"""GPU: the Temporal_tenco training draws made on the device (csrc/tenco_draw_kernels.hip) against their host form (`tenco_draws`), the
step that uses them -- eager, replayed as a hipGraph and against today's explicit-mask path -- and the driver's --mask_draw / --subclip."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from computervision_codes_amd import cholect, shapes, synth
from computervision_codes_amd import tenco_draws as td

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = (("", 100), ("_i", 6), ("_v", 10), ("_t", 15))
STATES = [(123, 0), (123, 7), (2 ** 40 + 5, 3)]


def _normal(seed, n):
    return synth.synthetic_features(1, n, seed=seed).flatten()


# ------------------------------------------------------------------------------------------------ mt4_dropout_mul_add_f32
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("n", [4, 1020, 1028, 70000])
def test_dropout_mul_add_equals_host_generator(cuda, n, p):
    """y = fma(a, m, c) / a * m with m from the host generator, bit for bit.  (The float64 product a * m is exact and so is the sum for
    p = 0.5, where m is 0 or 2; for p = 0.1 the float64 sum is rounded once more to float32, which can differ from the fused result only
    where it lies within 2^-29 of a float32 tie.)"""
    from computervision_codes_amd import ops
    a, c = _normal(1, n), _normal(2, n)
    slot = 7
    for seed, step in STATES:
        st = ops.draw_state(seed, step, cuda)
        m = torch.from_numpy(td.keep_mask(seed, step, slot, n, p))
        assert set(m.unique().tolist()) <= {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
        y = ops.dropout_mul_add(a.to(cuda), st, slot, p)
        assert torch.equal(y.cpu(), a * m)
        y = ops.dropout_mul_add(a.to(cuda), st, slot, p, c=c.to(cuda))
        assert torch.equal(y.cpu(), (a.double() * m.double() + c.double()).float())
        other = ops.dropout_mul_add(a.to(cuda), st, slot + 1, p)
        assert n == 4 or not torch.equal(other, ops.dropout_mul_add(a.to(cuda), st, slot, p))


def test_dropout_mul_add_follows_the_state_tensor(cuda):
    """only the device {seed, step} changes between two launches with the same arguments (what a replayed graph does)"""
    from computervision_codes_amd import ops
    n, slot = 1028, 3
    a = _normal(3, n).to(cuda)
    st = ops.draw_state(123, 0, cuda)
    y0 = ops.dropout_mul_add(a, st, slot)
    st.copy_(ops.draw_state(123, 7, cuda))
    y1 = ops.dropout_mul_add(a, st, slot)
    for y, step in ((y0, 0), (y1, 7)):
        assert torch.equal(y.cpu(), a.cpu() * torch.from_numpy(td.keep_mask(123, step, slot, n)))
    assert not torch.equal(y0, y1)


def test_draw_entry_points_reject_bad_arguments(cuda):
    from computervision_codes_amd import _lib, ops
    st = ops.draw_state(1, 2, cuda)
    a = torch.zeros(8, device=cuda)
    with pytest.raises(_lib.Mt4Error):
        ops.dropout_mul_add(a[:6], st, 0)               # n % 4 != 0
    with pytest.raises(_lib.Mt4Error):
        ops.dropout_mul_add(a, st, 4096)                # slot outside a step
    with pytest.raises(_lib.Mt4Error):
        ops.select_kth_key(8, 9, st, 0)                 # k > n
    with pytest.raises(_lib.Mt4Error):
        ops.tenco_input_draw(torch.zeros((2, 6), device=cuda), st, 0, None, 1)     # D % 4 != 0


# ------------------------------------------------------------------------------------------------ select + input draw
def _u64(t):
    return int(t.cpu().numpy().view(np.uint64)[0])


@pytest.mark.parametrize("T,D", [(1, 4), (8, 64), (10, 512), (37, 512), (257, 512), (2049, 512)])
def test_select_kth_key_equals_partition(cuda, T, D):
    """n = 4 / 512 / 5120 / 18 944 / 131 584 keys (1 to 65 workgroups) and 1 049 088 (a whole video: the capped grid, several keys per thread)"""
    from computervision_codes_amd import ops
    n = T * D
    for seed, step in STATES[1:]:
        st = ops.draw_state(seed, step, cuda)
        ks = td.keys(seed, step, td.SLOT_INPUT_KEYS, n)
        srt = np.sort(ks)
        for k in ((3 * n) // 4, 1, n):
            got = _u64(ops.select_kth_key(n, k, st, td.SLOT_INPUT_KEYS))
            assert got == int(np.partition(ks, k - 1)[k - 1]) == int(srt[k - 1]), (n, k)
        assert _u64(ops.select_kth_key(n, 0, st, td.SLOT_INPUT_KEYS)) == 0 and int(srt[0]) > 0       # k = 0 selects nothing


@pytest.mark.parametrize("T,D", [(1, 4), (8, 64), (10, 512), (37, 512), (257, 512)])
def test_input_draw_equals_host_mask_with_exact_count(cuda, T, D):
    from computervision_codes_amd import ops
    n, k = T * D, (3 * T * D) // 4
    x = _normal(5, n).view(1, T, D)
    for seed, step in STATES[1:]:
        st = ops.draw_state(seed, step, cuda)
        m = td.host_masks(seed, step, T, D, 8, [("PG", 1)], [T])
        keep = m["input_mask"][0].T.contiguous()           # [T][D]
        chan = m["channel_mask"][0].T                      # [1][D]
        assert int(keep.sum()) == k
        thr = ops.select_kth_key(n, k, st, td.SLOT_INPUT_KEYS)
        ones = ops.tenco_input_draw(torch.ones((T, D), device=cuda), st, td.SLOT_INPUT_KEYS, thr, td.SLOT_CHANNEL).cpu()
        assert torch.equal(ones, keep * chan)
        on = chan[0] != 0
        assert int((ones[:, on] != 0).sum()) == int(keep[:, on].sum())
        y = ops.tenco_input_draw(x.to(cuda), st, td.SLOT_INPUT_KEYS, thr, td.SLOT_CHANNEL).cpu()
        assert torch.equal(y[0], x[0] * keep * chan)
        y = ops.tenco_input_draw(x.to(cuda), st, td.SLOT_INPUT_KEYS, None, td.SLOT_CHANNEL).cpu()        # thr = NULL: Dropout2d alone
        assert torch.equal(y[0], x[0] * chan)


# ------------------------------------------------------------------------------------------------ the step
def _labels(seed, T):
    return {s: torch.from_numpy((synth.uniform01(seed, 900 + i, T * k) < 0.1).reshape(T, k).astype(np.int64)) for i, (s, k) in enumerate(HEADS)}


def _trainer(cfg, **kw):
    from computervision_codes_amd.tenco_train import TencoTrainer
    table = shapes.tenco_shapes(cfg["num_layers_PG"], cfg["num_layers_R"], cfg["num_R"], cfg["num_f_maps"], cfg["dim"], 100, fpn=True)
    sd = synth.fill_from_shapes(table, seed=cfg["seed"])
    tr = TencoTrainer(cfg["num_layers_PG"], cfg["num_layers_R"], cfg["num_R"], cfg["num_f_maps"], cfg["dim"], lr=cfg["lr"], weight_decay=1e-5,
                      hier=bool(cfg.get("hier", False)), **kw)
    return tr.load_state_dict(sd)


def _host_masks(tr, seed, step, T, input_mask=True):
    return td.host_masks(seed, step, T, tr.D, tr.C, tr._stages(), tr.level_lengths(T), input_mask=input_mask)


CFG = dict(num_layers_PG=3, num_layers_R=2, num_R=3, num_f_maps=64, dim=32, T=48, seed=79, lr=0.1)   # (of test_graph_replay_equals_eager)


def test_step_with_device_draws_eager_replayed_and_host_masks(cuda):
    a, b, c = _trainer(CFG), _trainer(CFG), _trainer(CFG)
    T, s = CFG["T"], 11
    x = synth.synthetic_features(T, CFG["dim"], seed=CFG["seed"]).to(cuda)
    labels = _labels(CFG["seed"], T)
    for k in range(3):
        la, _ = a.train_step(x, labels, draws=(s, k))
        lb, _ = b.train_step(x, labels, draws=(s, k), use_graph=True)
        lc, _ = c.train_step(x, labels, masks=_host_masks(c, s, k, T))
        assert abs(la - lb) < 1e-6 and abs(la - lc) < 1e-6, (k, la, lb, lc)
    assert len(b._graphs) == 1 and not a._graphs
    assert torch.equal(a.P, b.P)
    assert torch.equal(a.P, c.P)
    # a replay draws from the state it is handed
    g = []
    for k in (5, 5, 6):
        b.train_step(x, labels, draws=(s, k), use_graph=True, apply_update=False)
        g.append(b.G.clone())
    assert len(b._graphs) == 1 and torch.equal(g[0], g[1]) and not torch.equal(g[0], g[2])
    with pytest.raises(AssertionError):
        a.train_step(x, labels, draws=(s, 0), masks=_host_masks(a, s, 0, T))


def test_step_without_input_mask(cuda):
    """input_mask False (the driver without --mask): Dropout2d and the layer masks alone, replayed under a graph of its own"""
    a, b, c = _trainer(CFG), _trainer(CFG), _trainer(CFG)
    T, s = CFG["T"], 12
    x = synth.synthetic_features(T, CFG["dim"], seed=CFG["seed"]).to(cuda)
    labels = _labels(CFG["seed"], T)
    b.train_step(x, labels, draws=(s, 9), use_graph=True, apply_update=False)         # another mode at the same T: not this step's graph
    for k in range(2):
        la, _ = a.train_step(x, labels, draws=(s, k), input_mask=False)
        lb, _ = b.train_step(x, labels, draws=(s, k), input_mask=False, use_graph=True)
        lc, _ = c.train_step(x, labels, masks=_host_masks(c, s, k, T, input_mask=False))
        assert abs(la - lb) < 1e-6 and abs(la - lc) < 1e-6
    assert len(b._graphs) == 2 and torch.equal(a.P, b.P) and torch.equal(a.P, c.P)


def test_hier_step_with_device_draws_vs_host_masks(cuda):
    """--hier at T = 700: levels of 700 / 232 / 76 / 24 frames, every stage its own slots and length.  Weight gradients are atomic sums over
    several time splits here, so they are held to the bound of test_train_step_with_masks_vs_oracle (2e-4 of each tensor's max)"""
    cfg = dict(CFG, T=700, hier=True)
    a, c = _trainer(cfg), _trainer(cfg)
    T, s, k = 700, 21, 4
    assert a.level_lengths(T) == [700, 232, 76, 24]
    x = synth.synthetic_features(T, cfg["dim"], seed=cfg["seed"]).to(cuda)
    labels = _labels(cfg["seed"], T)
    la, _ = a.train_step(x, labels, draws=(s, k))
    lc, _ = c.train_step(x, labels, masks=_host_masks(c, s, k, T))
    print(f"hier T=700: loss device draws {la!r}, host masks {lc!r}")
    assert abs(la - lc) < 1e-6
    ga, gc = a.grads(), c.grads()
    assert set(ga) == set(gc)
    for name, ref in gc.items():
        err, bound = (ga[name] - ref).abs().max().item(), 2e-4 * max(ref.abs().max().item(), 1e-4)
        assert err <= bound, (name, err, bound)


def test_max_graphs_caps_the_cache(cuda):
    a, b = _trainer(CFG), _trainer(CFG, max_graphs=1)
    s = 31
    for k, T in enumerate((48, 40, 48, 40)):
        x = synth.synthetic_features(T, CFG["dim"], seed=CFG["seed"] + T).to(cuda)
        labels = _labels(CFG["seed"], T)
        la, _ = a.train_step(x, labels, draws=(s, k))
        lb, _ = b.train_step(x, labels, draws=(s, k), use_graph=True)
        assert abs(la - lb) < 1e-6
    assert [key[0] for key in b._graphs] == [("draws", 48, True)] and not a._graphs       # the second length ran eagerly
    assert torch.equal(a.P, b.P)


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_device_draws_and_reference_subclips(cuda, tmp_path):
    """`Temporal_tenco/run.py -t --mask --mask_draw device --subclip reference`: the epoch lines carry the `clips k/m` that `tenco_clip` gives
    for the run's seed, the whole-video steps share one cached graph; `--mask_draw host --subclip off` keeps the lines of the run without them"""
    from computervision_codes_amd import featfile
    from test_gpu_scripts import _make_dataset
    tree = tmp_path / "MT4MTLKD"
    shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
    data = str(tmp_path / "CholecT45")
    vids = _make_dataset(data, n_frames=12, h=8, w=8)
    rng = np.random.default_rng(1)
    featfile.write_feats(str(tree / "0-5fold" / "data_feats" / "run_S" / "k1_feats.pkl"), {v[-2:]: rng.standard_normal((12, 512)).astype(np.float32) for v in vids})
    env = dict(os.environ, PYTHONPATH=ROOT)
    table = shapes.tenco_shapes(11, 10, 3, 512, 512, 100, fpn=True)
    seed, epochs = 47, 4
    m = len(cholect.split_videos("cholect45-crossval", 1)[0])
    crng = random.Random(seed)
    want = [sum(td.tenco_clip(crng, 12)[1] != 12 for _ in range(m)) for _ in range(epochs)]
    assert 0 < sum(want) < epochs * m                                  # both branches occur for this seed

    def run(version, n_epochs, *flags):
        r = subprocess.run([sys.executable, "run.py", "-t", "--fpn", "--input_dim", "512", "--loss_type", "all", "--epochs", str(n_epochs), "-l", "1e-2", "5e-3",
                            "1e-2", "-w", "9", "18", "200", "--version", version, "--version1", "S", "--data_dir", data, "--kfold", "1", "--seed", str(seed),
                            *flags], cwd=tree / "Temporal_tenco", env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        ck = tree / "Temporal_tenco" / "__checkpoint__" / f"run_{version}" / "rendezvous_l8_cholectcholect45-crossval_k1_batchnorm_lowres_latest.pth"
        sd = torch.load(ck, map_location="cpu")
        assert list(sd.keys()) == [k for k, _ in table] and all(tuple(sd[k].shape) == tuple(s) for k, s in table)
        assert all(torch.isfinite(v).all() for v in sd.values())
        return sd, open(str(ck).replace("_latest.pth", ".log")).read()

    sd, log = run("D_TCN", epochs, "--mask", "--mask_draw", "device", "--subclip", "reference")
    lines = [ln for ln in log.splitlines() if ln.startswith("Traning | lr:")]
    assert [tuple(map(int, re.search(r"\| clips (\d+)/(\d+)$", ln).groups())) for ln in lines] == [(k, m) for k in want]
    note = [ln for ln in log.splitlines() if ln.startswith("mask_draw device")]
    assert len(note) == 1 and re.fullmatch(r"mask_draw device \| subclip reference \| cached graphs 1 \| reserved bytes added \d+", note[0]), note
    assert not torch.equal(sd["PG.conv_1x1.weight"], synth.fill_from_shapes(table, seed=seed)["PG.conv_1x1.weight"])
    _, log = run("H_TCN", 2, "--mask", "--mask_draw", "host", "--subclip", "off")
    assert log.count("Traning | lr:") == 2 and log.count("mAP => ivt:") == 2 and ">>> Saving checkpoint for epoch 1" in log
    assert "clips" not in log and "mask_draw" not in log
