"""GPU: `--metrics device` -- `ops.video_ap` / `ops.component_max` / `metrics_device.DeviceRecognition` against `metrics.Recognition`
(sklearn) on the same fp32 scores, and against an exact rational AP for short columns.

Tolerance (every AP comparison below): |AP_dev - AP_host| <= 4 (n + 4) 2^-53 for a column of n rows.  Each side sums at most n non-negative
terms whose total is <= 1 with at most three roundings per term: (n + 2) 2^-53 per side; the bound allows a factor of two over the pair
(3.6e-12 at n = 8192).  The NaN pattern (columns without positives, videos of 0 rows) must be identical."""
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from computervision_codes_amd import metrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PATTERNS = ("continuous", "quantised", "equal", "zeros", "no_positives", "all_positives", "last")


def _bound(n):
    return 4.0 * (n + 4) * 2.0 ** -53


def _column(pattern, n, rng):
    """(scores fp32 [n], labels 0/1 [n]) of one score pattern"""
    s = rng.random(n).astype(np.float32)
    z = (rng.random(n) < 0.3).astype(np.float32)
    z[rng.integers(n)] = 1.0
    if pattern == "quantised":                                     # 8 levels: heavy ties
        s = (np.floor(s * 8) / 8).astype(np.float32)
    elif pattern == "equal":                                       # one tie group: AP = P / n
        s[:] = np.float32(0.37)
    elif pattern == "zeros":                                       # +0.0 and -0.0 are ONE threshold; positives on both
        s = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        z[:2] = 1.0
    elif pattern == "no_positives":
        z[:] = 0.0
    elif pattern == "all_positives":
        z[:] = 1.0
    elif pattern == "last":                                        # a single positive, ranked last: AP = 1 / n
        z[:] = 0.0
        s[0] = np.float32(-1.5)
        z[0] = 1.0
    return s, z


def _videos(lengths, k, ld, seed):
    """scores / labels fp32 [sum(lengths), ld]: column c of video v carries pattern (c + v) % 7, so a 5-video launch sees every pattern in
    every column; the columns k..ld-1 hold values that would change every AP if they were read"""
    rng = np.random.default_rng(seed)
    S, Z = [], []
    for v, n in enumerate(lengths):
        s, z = np.full((n, ld), 0.99, np.float32), np.ones((n, ld), np.float32)
        for c in range(k if n else 0):
            s[:, c], z[:, c] = _column(PATTERNS[(c + v) % 7], n, rng)
        S.append(s)
        Z.append(z)
    return np.concatenate(S), np.concatenate(Z), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _host_ap(S, Z, offs, k):
    """the reference: `metrics.Recognition._ap_per_class` (sklearn) per video on float64 copies of the same fp32 scores"""
    return np.stack([metrics.Recognition._ap_per_class(Z[a:b, :k].astype(np.float64), S[a:b, :k].astype(np.float64)) for a, b in zip(offs[:-1], offs[1:])])


def _exact_ap(s, z):
    """AP from the definition in rationals: distinct thresholds descending, sum of (recall step) x precision"""
    P = int(z.sum())
    if P == 0:
        return None
    total, tp_prev = Fraction(0), 0
    for thr in sorted(set(float(x) for x in s), reverse=True):     # (-0.0 == 0.0: one element)
        hit = s >= thr
        tp, r = int(z[hit].sum()), int(hit.sum())
        total += Fraction(tp - tp_prev, P) * Fraction(tp, r)
        tp_prev = tp
    return total


def _device_ap(S, Z, offs, k):
    from computervision_codes_amd import ops
    s, z = torch.from_numpy(S).cuda(), torch.from_numpy(Z).cuda()
    a = ops.video_ap(s, z, offs, k)
    b = ops.video_ap(s, z, offs, k)
    torch.cuda.synchronize()
    assert a.dtype == torch.float64 and tuple(a.shape) == (len(offs) - 1, k)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "two launches on the same input differ in bits"
    return a.cpu().numpy()


def _check(lengths, k, ld, seed):
    S, Z, offs = _videos(lengths, k, ld, seed)
    dev, host = _device_ap(S, Z, offs, k), _host_ap(S, Z, offs, k)
    assert np.array_equal(np.isnan(dev), np.isnan(host)), (np.argwhere(np.isnan(dev) != np.isnan(host))[:5], lengths, k)
    for v, n in enumerate(lengths):
        err = np.nan_to_num(np.abs(dev[v] - host[v]), nan=0.0)
        print(f"video {v}: n {n} k {k}/{ld} max |dev - host| {err.max():.3e} bound {_bound(n):.3e}")
        assert (err <= _bound(n)).all(), (v, n, k, int(err.argmax()), PATTERNS[(int(err.argmax()) + v) % 7], float(err.max()), _bound(n))
        for c in range(k if n else 0):
            pat = PATTERNS[(c + v) % 7]
            s, z = S[offs[v]:offs[v + 1], c], Z[offs[v]:offs[v + 1], c]
            if pat == "no_positives":
                assert np.isnan(dev[v, c])
            elif pat in ("equal", "zeros"):                        # one tie group
                assert abs(dev[v, c] - int(z.sum()) / n) <= _bound(n), (pat, n, dev[v, c], int(z.sum()) / n)
            elif pat == "all_positives":
                assert abs(dev[v, c] - 1.0) <= _bound(n)
            elif pat == "last":
                assert abs(dev[v, c] - 1.0 / n) <= _bound(n)
            if n <= 64 and pat != "no_positives":
                exact = _exact_ap(s, z)
                assert abs(dev[v, c] - float(exact)) <= _bound(n), (pat, n, dev[v, c], float(exact))
        if n == 0:
            assert np.isnan(dev[v]).all()


def _cap():
    from computervision_codes_amd import ops
    return ops.video_ap_max_rows()


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1000, "cap", "half_cap_plus_1"])
def test_video_ap_one_video_every_row_count(cuda, n):
    """every pattern twice (k = 15) at each row count: below, at and above a power of two, the cap, and the first size padded to the cap"""
    cap = _cap()
    assert cap >= 8192
    n = {"cap": cap, "half_cap_plus_1": cap // 2 + 1}.get(n, n)
    _check([n], 15, 15, seed=n)


@pytest.mark.parametrize("k,ld", [(6, 6), (15, 15), (26, 26), (59, 59), (94, 100), (100, 100), (131, 132)])
@pytest.mark.parametrize("n", [65, 1000])
def test_video_ap_column_addressing(cuda, n, k, ld):
    _check([n], k, ld, seed=1000 * n + k)


@pytest.mark.parametrize("k,ld", [(6, 6), (94, 100), (131, 132)])
def test_video_ap_five_videos_of_unequal_lengths(cuda, k, ld):
    """one launch, videos of 300 / 0 / 1 / 65 / 1000 rows (a video of 0 rows writes NaN)"""
    _check([300, 0, 1, 65, 1000], k, ld, seed=k)


def test_video_ap_five_videos_up_to_the_cap(cuda):
    cap = _cap()
    _check([cap, 3, 0, cap // 2 + 1, 64], 6, 6, seed=5)


def test_video_ap_more_videos_than_one_launch_takes(cuda):
    """300 videos of 1 / 2 / 65 rows: the row offsets ride in the kernel arguments 255 videos at a time, so this is two launches, the second
    on re-based offsets and the rows of `ap_out` behind the first 255"""
    _check([65 if v in (3, 254, 255, 299) else 1 + v % 2 for v in range(300)], 6, 6, seed=9)


def test_component_max_is_bit_equal_to_disentangle(cuda):
    from computervision_codes_amd import ops
    rng = np.random.default_rng(11)
    scores = rng.random((257, 100)).astype(np.float32)
    labels = (rng.random((257, 100)) < 0.1).astype(np.float32)
    for comp, kc in (("i", 6), ("v", 10), ("t", 15), ("iv", 26), ("it", 59)):
        table, k = metrics.component_table(comp)
        assert k == kc
        for x in (scores, labels):
            got = ops.component_max(torch.from_numpy(x).cuda(), table, k).cpu().numpy()
            assert got.dtype == np.float32 and np.array_equal(got, metrics.disentangle(x, comp)), comp


@pytest.fixture(scope="module")
def three_videos(cuda):
    """three synthetic videos of 300 / 257 / 1 frames with the 100-way scores: (fp32 labels, fp32 scores) per video, the host metric fed
    with them and the device metric fed with the same rows on the GPU"""
    from computervision_codes_amd.metrics_device import DeviceRecognition
    rng = np.random.default_rng(21)
    vids = []
    for n in (300, 257, 1):
        s = rng.random((n, 100)).astype(np.float32)
        s[:, ::3] = np.floor(s[:, ::3] * 8) / 8                    # ties in a third of the columns
        vids.append(((rng.random((n, 100)) < 0.15).astype(np.float32), s))
    host, dev = metrics.Recognition(100), DeviceRecognition(100)
    for t, p in vids:
        for a in range(0, len(t), 128):                            # (fed in pieces, like the frame trainers' validation)
            host.update(t[a:a + 128], p[a:a + 128])
            dev.update(torch.from_numpy(t[a:a + 128]).cuda(), torch.from_numpy(p[a:a + 128]).cuda())
        host.video_end()
        dev.video_end()
    return host, dev


@pytest.mark.parametrize("ignore_null", [False, True])
@pytest.mark.parametrize("component", ["ivt", "i", "v", "t", "iv", "it"])
def test_device_recognition_matches_recognition(cuda, three_videos, component, ignore_null):
    """AP vector and mAP: nan-means (the same numpy lines on both sides) of per-video APs that each meet the bound of their video, so the
    means meet the bound of the longest video (300 rows): the mean's own rounding, a few 2^-53, lies inside the bound's factor of two"""
    host, dev = three_videos
    h, d = host.compute_video_AP(component, ignore_null=ignore_null), dev.compute_video_AP(component, ignore_null=ignore_null)
    assert d["AP"].shape == h["AP"].shape and d["AP"].dtype == np.float64 and isinstance(d["mAP"], float)
    assert np.array_equal(np.isnan(d["AP"]), np.isnan(h["AP"]))
    err = np.nan_to_num(np.abs(d["AP"] - h["AP"]), nan=0.0).max()
    print(f"{component} ignore_null {ignore_null}: max |AP_dev - AP_host| {err:.3e}, |mAP_dev - mAP_host| {abs(d['mAP'] - h['mAP']):.3e}, bound {_bound(300):.3e}")
    assert err <= _bound(300) and abs(d["mAP"] - h["mAP"]) <= _bound(300)


def test_device_recognition_to_host_topk_and_component_heads(cuda, three_videos):
    from computervision_codes_amd.metrics_device import DeviceRecognition
    host, dev = three_videos
    back = dev.to_host()
    assert isinstance(back, metrics.Recognition) and len(back.global_targets) == 3
    for a, b in zip(back.global_targets + back.global_predictions, host.global_targets + host.global_predictions):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    for c in ("ivt", "i", "v", "t", "iv", "it"):
        assert dev.topK(5, c) == host.topK(5, c) == back.topK(5, c)
    # a 6-way component head, and a metric with nothing recorded
    rng = np.random.default_rng(3)
    t, p = (rng.random((65, 6)) < 0.3).astype(np.float32), rng.random((65, 6)).astype(np.float32)
    h6, d6 = metrics.Recognition(6), DeviceRecognition(6)
    h6.update(t, p)
    h6.video_end()
    d6.update(torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda())
    d6.video_end()
    assert abs(h6.compute_video_AP()["mAP"] - d6.compute_video_AP()["mAP"]) <= _bound(65)
    with pytest.raises(ValueError):
        d6.compute_video_AP("i")
    none = DeviceRecognition(6).compute_video_AP()
    assert np.isnan(none["AP"]).all() and none["AP"].shape == (6,) and np.isnan(none["mAP"])


def test_a_video_above_the_cap_falls_back_to_the_host_metric(cuda, capsys):
    from computervision_codes_amd.metrics_device import DeviceRecognition
    cap = _cap()
    rng = np.random.default_rng(4)
    t, p = (rng.random((cap + 1, 6)) < 0.3).astype(np.float32), rng.random((cap + 1, 6)).astype(np.float32)
    h, d = metrics.Recognition(6), DeviceRecognition(6)
    h.update(t, p)
    h.video_end()
    d.update(torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda())
    d.video_end()
    want, got = h.compute_video_AP(), d.compute_video_AP()
    assert np.array_equal(want["AP"], got["AP"]) and want["mAP"] == got["mAP"]
    said = capsys.readouterr().out
    assert str(cap + 1) in said and str(cap) in said and said.count("\n") == 1


# ------------------------------------------------------------------------------------------------ the drivers under --metrics device
@pytest.fixture
def metric_calls(monkeypatch):
    """counts of the calls that tell the two metric paths apart: `ops.video_ap` / `ops.component_max` (device) and
    `Recognition._ap_per_class` (sklearn, host); the drivers ignore flags they do not know, so equal logs alone prove nothing"""
    from computervision_codes_amd import ops
    calls = {"video_ap": 0, "component_max": 0, "sklearn": 0}
    real = {"video_ap": ops.video_ap, "component_max": ops.component_max, "sklearn": metrics.Recognition._ap_per_class}

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return f
    monkeypatch.setattr(ops, "video_ap", counted("video_ap"))
    monkeypatch.setattr(ops, "component_max", counted("component_max"))
    monkeypatch.setattr(metrics.Recognition, "_ap_per_class", staticmethod(counted("sklearn")))
    return calls


def _taken(calls):
    got = dict(calls)
    for k in calls:
        calls[k] = 0
    return got


def _write_labels(data, vids, n, rng):
    for sub, k in (("triplet", 100), ("instrument", 6), ("verb", 10), ("target", 15)):
        os.makedirs(os.path.join(data, sub), exist_ok=True)
        for v in vids:
            lab = np.concatenate([np.arange(n[v])[:, None], (rng.random((n[v], k)) < 0.15).astype(int)], 1)
            np.savetxt(os.path.join(data, sub, v + ".txt"), lab, fmt="%d", delimiter=",")


def _same_pickled_metrics(a, b):
    """both `mAPs*.pckl`: {'ivt', 'i', 'v', 't'} -> `metrics.Recognition` with float64 arrays, the same videos"""
    assert sorted(a) == sorted(b) == ["i", "ivt", "t", "v"]
    for h in a:
        assert type(a[h]) is metrics.Recognition and type(b[h]) is metrics.Recognition and a[h].num_class == b[h].num_class
        for x, y in zip(a[h].global_targets + a[h].global_predictions, b[h].global_targets + b[h].global_predictions):
            assert isinstance(x, np.ndarray) and x.dtype == np.float64 and y.dtype == np.float64 and np.array_equal(x, y)
        assert len(a[h].global_targets) == len(b[h].global_targets) > 0


def _val_lines(log):
    return [ln.split("mAP =>")[1].strip() for ln in log.splitlines() if "mAP =>" in ln]


def test_tenco_driver_validates_and_reports_on_the_device(cuda, tmp_path, monkeypatch, metric_calls):
    """`Temporal_tenco/run.py -t -e --fpn --mask_draw device` (its `drivers.tenco_eval`, in this process so that the metric calls can be
    counted), two epochs on the tiny synthetic dataset, --metrics host against --metrics device.  The device run launches `ops.video_ap` and
    never enters sklearn, the host run the reverse; the validation scores as logged (5 decimals), the epochs whose state became the best
    `.pth` and the pickled metric objects are the same, the closing report's mean-AP rows (4 printed decimals) agree to one unit of the last
    digit (a rounding boundary).  (The device draws make the two trainings the same sequence of steps, and at 12 frames per video every
    reduction of a step is one workgroup per address -- no split-K float atomics -- so the two runs validate the same weights.)"""
    import pickle

    from test_gpu_scripts import _make_dataset, _report_rows
    from computervision_codes_amd import drivers, featfile
    tree = tmp_path / "MT4MTLKD"
    shutil.copytree(os.path.join(ROOT, "MT4MTLKD"), tree)
    data = str(tmp_path / "CholecT45")
    vids = _make_dataset(data, n_frames=12, h=8, w=8)
    rng = np.random.default_rng(1)
    featfile.write_feats(str(tree / "0-5fold" / "data_feats" / "run_S" / "k1_feats.pkl"), {v[-2:]: rng.standard_normal((12, 512)).astype(np.float32) for v in vids})
    monkeypatch.chdir(tree / "Temporal_tenco")
    logs, calls, pck = {}, {}, {}
    for mode in ("host", "device"):
        _taken(metric_calls)
        drivers.tenco_eval(["-t", "-e", "--fpn", "--mask_draw", "device", "--metrics", mode, "--input_dim", "512", "--loss_type", "all", "--epochs", "2",
                            "-l", "1e-2", "5e-3", "1e-2", "-w", "9", "18", "200", "--version", "M_" + mode, "--version1", "S", "--data_dir", data, "--kfold", "1"])
        calls[mode] = _taken(metric_calls)
        run = tree / "Temporal_tenco" / "__checkpoint__" / ("run_M_" + mode)
        stem = run / "rendezvous_l8_cholectcholect45-crossval_k1_batchnorm_lowres"
        logs[mode] = open(str(stem) + ".log").read()
        assert os.path.exists(str(stem) + ".pth")
        with open(run / "mAPs_k1.pckl", "rb") as f:
            pck[mode] = pickle.load(f)
    print(calls)
    assert calls["host"]["video_ap"] == 0 and calls["host"]["component_max"] == 0 and calls["host"]["sklearn"] > 0
    # two validations of two compute_video_AP() each + the nine AP sets of the report; five of those disentangle scores and labels
    assert calls["device"]["video_ap"] == 2 * 2 + 9 and calls["device"]["component_max"] == 2 * 5 and calls["device"]["sklearn"] == 0
    vh, vd = _val_lines(logs["host"]), _val_lines(logs["device"])
    print("host", vh, "device", vd)
    assert len(vh) == 2 and vh == vd
    saved = lambda log: [ln.split(" at ")[0] for ln in log.splitlines() if ln.startswith(">>> Saving checkpoint for epoch")]
    assert saved(logs["host"]) == saved(logs["device"]) and len(saved(logs["host"])) >= 1
    rh, rd = np.array(_report_rows(logs["host"])), np.array(_report_rows(logs["device"]))
    assert rh.shape == rd.shape == (2, 6) and np.abs(rh - rd).max() <= 1.0001e-4
    _same_pickled_metrics(pck["host"], pck["device"])


class _FakeMstct:
    """`forward_btd` of a single-task MS-TCT whose logits are the first K feature columns: ([1, T, K],) in the task's slot"""

    def __init__(self, gi, k):
        self.gi, self.k = gi, k

    def forward_btd(self, x):
        out = [None] * 4
        out[self.gi] = (3.0 * x[:, :, :self.k],)
        return out


@pytest.mark.parametrize("chlg", [False, True])
def test_mstct_scores_and_report_on_the_device(cuda, tmp_path, metric_calls, chlg):
    """`_mstct_scores` -> `_recognition` -> `_write_report('temporal_mstct')` as `_mstct_train.validate` and `Temporal_mstct/run.py -e` chain
    them, host against device, on three videos of 300 / 257 / 1 frames (two windows, a window of one frame over the 256, one short window)"""
    import pickle

    from computervision_codes_amd import drivers, featfile
    from computervision_codes_amd.metrics_device import DeviceRecognition
    rng = np.random.default_rng(2)
    vids = ["VID01", "VID02", "VID04"]
    n = dict(zip(vids, (300, 257, 1)))
    data = str(tmp_path / "data")
    _write_labels(data, vids, n, rng)
    feats = {featfile.video_key(v): rng.standard_normal((n[v], 128)).astype(np.float32) for v in vids}
    feats[featfile.video_key("VID01")][::2, :50] = 0.25                  # ties
    model, cache, res, pck = _FakeMstct(3, 100), {}, {}, {}
    for dev in (False, True):
        _taken(metric_calls)
        sc = drivers._mstct_scores(model, feats, vids, data, "ivt", dev, cache)
        if dev:
            first = {v: {h: cache[v][h].data_ptr() for h in cache[v]} for v in vids}
            sc = drivers._mstct_scores(model, feats, vids, data, "ivt", dev, cache)          # the next validation: no second upload
            assert first == {v: {h: cache[v][h].data_ptr() for h in cache[v]} for v in vids}
            assert all(t.is_cuda and p.is_cuda and t.dtype == p.dtype == torch.float32 and t.shape == p.shape
                       for v in vids for t, p in sc[v].values())
            assert sc["VID01"]["ivt"][0].data_ptr() == cache["VID01"]["ivt"].data_ptr()
        else:
            assert not cache and all(isinstance(p, np.ndarray) for v in vids for _, p in sc[v].values())
        m = drivers._recognition(sc, vids, dev)
        assert sorted(m) == ["i", "ivt", "t", "v"] and all(type(x) is (DeviceRecognition if dev else metrics.Recognition) for x in m.values())
        val = m["ivt"].compute_video_AP(ignore_null=chlg)["mAP"]                             # (`_mstct_train.validate`)
        pckl = str(tmp_path / f"mAPs_{dev}.pckl")
        res[dev] = dict(drivers._write_report(str(tmp_path / f"report_{dev}.log"), m, "ivt", chlg, "temporal_mstct", pckl=pckl), val=val)
        with open(pckl, "rb") as f:
            pck[dev] = pickle.load(f)
        got = _taken(metric_calls)
        assert (got["video_ap"] == 10 and got["component_max"] == 10 and got["sklearn"] == 0) if dev else (got["video_ap"] == 0 and got["sklearn"] > 0), got
    assert sorted(res[False]) == sorted(res[True])
    for key in res[False]:                                                                   # mean APs: the bound of the longest video
        print(key, res[False][key], res[True][key])
        assert abs(res[False][key] - res[True][key]) <= _bound(300), key
    _same_pickled_metrics(pck[False], pck[True])
    lines = [open(tmp_path / f"report_{dev}.log").read().splitlines() for dev in (False, True)]
    assert len(lines[0]) == len(lines[1]) > 10


def test_frame_validation_on_the_device(cuda, tmp_path, metric_calls):
    """`_frame_validation` (both frame trainers' validation) on two videos of 5 frames in device batches of 2: the head's scores stay on
    the GPU, the label rows are uploaded once per video and run"""
    from PIL import Image

    from computervision_codes_amd import cholect, drivers
    rng = np.random.default_rng(6)
    vids = ["VID01", "VID02"]
    data = str(tmp_path / "data")
    _write_labels(data, vids, {v: 5 for v in vids}, rng)
    for v in vids:
        os.makedirs(os.path.join(data, "data", v))
        for i in range(5):
            Image.fromarray(rng.integers(0, 255, (8, 8, 3), dtype=np.uint8)).save(os.path.join(data, "data", v, f"{i:06d}.png"))
    labels = {v: cholect.load_labels(data, v) for v in vids}
    forward = lambda fr: (fr.reshape(fr.shape[0], -1)[:, :100].float() - 128.0) / 32.0       # logits [B, 100] of the uint8 frames
    out, cache = {}, {}
    for mode in ("host", "device"):
        F = drivers._parser("spatial_cnn", True).parse_known_args(["--metrics", mode, "--data_dir", data, "-b", "2", "--device_batch", "2"])[0]
        _taken(metric_calls)
        out[mode] = drivers._frame_validation(F, vids, labels, (8, 8), 2, forward, cache)
        got = _taken(metric_calls)
        if mode == "device":
            assert got == {"video_ap": 1, "component_max": 0, "sklearn": 0} and sorted(cache) == vids and cache["VID01"]["ivt"].is_cuda
            first = {v: cache[v]["ivt"].data_ptr() for v in vids}
            again = drivers._frame_validation(F, vids, labels, (8, 8), 2, forward, cache)
            assert again == out[mode] and first == {v: cache[v]["ivt"].data_ptr() for v in vids}
        else:
            assert got["video_ap"] == 0 and got["sklearn"] == 2 and not cache
    print(out)
    assert abs(out["host"][0] - out["device"][0]) <= _bound(5) and out["host"][1] == out["device"][1] and out["host"][0] > 0
