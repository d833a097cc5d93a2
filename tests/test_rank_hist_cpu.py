"""CPU: top-K from rank histograms -- `metrics.rank_hist` (the stable rank by its definition, no sort) against `Recognition.topK` (the
reference's argsort loop), the merged metric object N ranks build from per-video AP rows and histograms
(`metrics_device.gather_device_recognition`), and the argument checks of `mt4_rank_hist_f32` that return before any launch.
Every comparison of a top-K number is `==`: both sides divide the same two Python integers once."""
import ctypes
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from computervision_codes_amd import metrics


def tie_heavy(rng, n, k):
    """scores on 4 values, exact 0.0 and 1.0 among them (saturated sigmoids), zeros of both signs"""
    p = rng.choice(np.array([0.0, 0.25, 0.75, 1.0], dtype=np.float32), size=(n, k))
    p[(p == 0) & (rng.random((n, k)) < 0.5)] = np.float32(-0.0)
    return p


def videos(K, seed, nan=True):
    """three videos (fp32 labels, fp32 scores) of 37 / 1 / 20 rows: random scores, tie-heavy scores, and a video with a row without
    positives, a row of positives only and one NaN score"""
    rng = np.random.default_rng(seed)
    lab = lambda n: (rng.random((n, K)) < 0.3).astype(np.float32)
    a = (lab(37), rng.random((37, K)).astype(np.float32))
    b = (lab(1), tie_heavy(rng, 1, K))
    t, p = lab(20), tie_heavy(rng, 20, K)
    t[3], t[4] = 0.0, 1.0
    p[7:12] = rng.random((5, K)).astype(np.float32)
    if nan:
        p[4, K // 2] = np.nan
        p[9, 0] = np.nan
    return [a, b, (t, p)]


def _recognition(vids, K):
    m = metrics.Recognition(K)
    return m.set_videos(vids)


@pytest.mark.parametrize("K", [1, 6, 10, 15, 100])
def test_rank_hist_gives_topk_for_every_k(K):
    vids = videos(K, seed=K)
    m = _recognition(vids, K)
    hist = sum(metrics.rank_hist(t, p) for t, p in vids)
    assert hist.dtype == np.int64 and hist.shape == (K,)
    positives = sum(int((t != 0).sum()) for t, _ in vids)
    assert int(hist.sum()) == positives > 0
    for k in (1, 5, 10, 20, K, K + 7):
        assert int(hist[:k].sum()) / max(int(hist.sum()), 1) == m.topK(k), k
    assert int(hist[:K].sum()) == positives                        # every positive has a rank below K


def test_rank_hist_of_the_first_k_columns_and_of_components():
    """k < ld reads the first k columns only (the ignore_null layout), and a disentangled component's histogram gives its top-K"""
    vids = videos(100, seed=5)
    for t, p in vids:
        assert np.array_equal(metrics.rank_hist(t, p, 94), metrics.rank_hist(t[:, :94].copy(), p[:, :94].copy()))
    m = _recognition(vids, 100)
    for c in ("i", "v", "t", "iv", "it"):
        hist = sum(metrics.rank_hist(metrics.disentangle(t.astype(np.float64), c), metrics.disentangle(p.astype(np.float64), c)) for t, p in videos(100, 5, nan=False))
        mc = _recognition(videos(100, 5, nan=False), 100)
        for k in (1, 5, 10, 20, 100):
            assert int(hist[:k].sum()) / max(int(hist.sum()), 1) == mc.topK(k, c), (c, k)
    assert m.topK(5) == int(sum(metrics.rank_hist(t, p) for t, p in vids)[:5].sum()) / sum(int((t != 0).sum()) for t, _ in vids)


def test_rank_hist_by_hand():
    """ranks spelled out: ties go to the lower class id, -0.0 ties with +0.0, NaN comes last (behind -inf) and ties with NaN"""
    p = np.array([[0.5, 0.5, 0.9, -0.0, 0.0, np.nan, -np.inf, np.nan]], dtype=np.float32)
    order = np.argsort(-p[0], kind="stable")
    assert order.tolist() == [2, 0, 1, 3, 4, 6, 5, 7]
    for c in range(8):
        t = np.zeros((1, 8), np.float32)
        t[0, c] = 1
        assert metrics.rank_hist(t, p).tolist() == [int(order[r] == c) for r in range(8)]
    assert metrics.rank_hist(np.zeros((4, 8)), np.tile(p, (4, 1))).tolist() == [0] * 8          # no positives: all bins 0
    assert metrics.rank_hist(np.ones((4, 8)), np.tile(p, (4, 1))).tolist() == [4] * 8           # all positive: every rank once per row
    assert metrics.rank_hist(np.zeros((0, 8)), np.zeros((0, 8))).tolist() == [0] * 8
    assert metrics.Recognition(8).topK(5) == 0.0                                                 # nothing recorded: 0 / 1


# ------------------------------------------------------------------------------------------------ the merged object of N ranks
ORDER = ["VID01", "VID02", "VID03", "VID04", "VID05"]
WIDTH = {"i": 6, "v": 10, "t": 15, "iv": 26, "it": 59, "ivt": 100}


def _hand_made(rank):
    """the summary one of two ranks would send: rank 0 holds videos 1, 3, 5 (not in file order), rank 1 holds 4, 2"""
    mine = (["VID05", "VID01", "VID03"], ["VID04", "VID02"])[rank]
    ap, hist = {}, {}
    for v in mine:
        rng = np.random.default_rng(int(v[3:]))
        ap[v] = {}
        for h, n in metrics.HEADS:
            ap[v][h] = {}
            for c in (WIDTH if n == 100 else ("ivt",)):
                row = rng.random(WIDTH[c] if n == 100 else n)
                row[rng.random(row.shape) < 0.3] = np.nan              # classes without positives in this video
                ap[v][h][c] = row
    for h, n in metrics.HEADS:
        rng = np.random.default_rng(100 + rank)
        hist[h] = {c: rng.integers(0, 50, WIDTH[c] if n == 100 else n).astype(np.int64) for c in (WIDTH if n == 100 else ("ivt",))}
    return {"ap": ap, "hist": hist}


def _check_merged(m):
    parts = [_hand_made(0), _hand_made(1)]
    ap = {**parts[0]["ap"], **parts[1]["ap"]}
    assert sorted(m) == ["i", "ivt", "t", "v"]
    for h, n in metrics.HEADS:
        for c in (WIDTH if n == 100 else ("ivt",)):
            rows = [ap[v][h][c] for v in ORDER]
            for ignore_null in (False, True):
                cut = 94 if (ignore_null and c == "ivt" and n == 100) else None
                want = metrics.video_mean([r[:cut] for r in rows], n)
                got = m[h].compute_video_AP(c, ignore_null=ignore_null)
                assert np.array_equal(got["AP"], want["AP"], equal_nan=True) and got["AP"].shape == ((cut or len(rows[0])),)
                assert got["mAP"] == want["mAP"] or (np.isnan(got["mAP"]) and np.isnan(want["mAP"]))
            hist = parts[0]["hist"][h][c] + parts[1]["hist"][h][c]
            for k in (1, 5, 10, 20, 100, 120):
                assert m[h].topK(k, c) == int(hist[:k].sum()) / max(int(hist.sum()), 1)
        if n != 100:
            with pytest.raises(ValueError):
                m[h].compute_video_AP("i")
            with pytest.raises(ValueError):
                m[h].topK(5, "iv")


def test_merged_recognition_from_hand_made_rows_without_a_process_group():
    from computervision_codes_amd import metrics_device
    both = {"ap": {**_hand_made(0)["ap"], **_hand_made(1)["ap"]},
            "hist": {h: {c: _hand_made(0)["hist"][h][c] + _hand_made(1)["hist"][h][c] for c in _hand_made(0)["hist"][h]} for h, _ in metrics.HEADS}}
    _check_merged(metrics_device.gather_device_recognition(both, ORDER))
    with pytest.raises(KeyError):
        metrics_device.gather_device_recognition(_hand_made(0), ORDER)
    # the report's lines come out of the merged objects like out of any other
    lines, res = metrics.final_report(metrics_device.gather_device_recognition(both, ORDER), "all", False, "spatial_cnn")
    assert sum(ln.startswith("top ") for ln in lines) == 3 and "top20_ivt" in res and "AP_ivt" in res


def _worker(rank, world, port, outdir):
    import torch.distributed as dist
    from computervision_codes_amd import metrics_device
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _check_merged(metrics_device.gather_device_recognition(_hand_made(rank), ORDER))
        open(os.path.join(outdir, f"ok{rank}"), "w").close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_merged_recognition_through_a_world2_gloo_group(tmp_path):
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert sorted(os.listdir(tmp_path)) == ["ok0", "ok1"]          # every rank holds the merged objects


# ------------------------------------------------------------------------------------------------ mt4_rank_hist_f32: refusals before a launch
def test_rank_hist_refuses_bad_arguments_before_any_launch():
    """on HOST buffers: every case here must be refused before a launch could read them"""
    from computervision_codes_amd import _lib
    buf = (ctypes.c_float * 256)()
    out = (ctypes.c_int64 * 256)()
    b, o = ctypes.addressof(buf), ctypes.addressof(out)
    call = _lib.lib.mt4_rank_hist_f32
    assert call(None, b, 1, 6, 6, o, None) == -1 and call(b, None, 1, 6, 6, o, None) == -1 and call(b, b, 1, 6, 6, None, None) == -1
    assert call(b, b, 0, 6, 6, o, None) == -1 and call(b, b, -3, 6, 6, o, None) == -1
    assert call(b, b, 1, 0, 6, o, None) == -1 and call(b, b, 1, -1, 6, o, None) == -1
    assert call(b, b, 1, 7, 6, o, None) == -1                      # ld < k
    assert call(b, b, 1, 129, 129, o, None) == _lib.MT4_EUNSUPPORTED == -4
    assert call(b, b, (1 << 40) + 1, 6, 6, o, None) == -4
    assert all(x == 0 for x in out)
