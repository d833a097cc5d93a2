"""CPU: the host side of `--metrics device` -- the component tables, the flag, the argument checks of `mt4_video_ap_f32` /
`mt4_component_max_f32` (they return before any launch) and the nan-mean helper the host and the device metric share."""
import ctypes

import numpy as np
import pytest

from computervision_codes_amd import metrics


@pytest.mark.parametrize("component,kc", [("i", 6), ("v", 10), ("t", 15), ("iv", 26), ("it", 59)])
def test_component_tables_reproduce_disentangle(component, kc):
    table, k = metrics.component_table(component)
    assert k == kc and table.dtype == np.int32 and table.shape == (100,) and table.min() == 0 and table.max() == kc - 1
    rng = np.random.default_rng(7)
    for x in (rng.random((50, 100)), (rng.random((50, 100)) < 0.1).astype(np.float64)):
        got = np.stack([x[:, table == c].max(axis=1) for c in range(kc)], axis=1)
        assert np.array_equal(got, metrics.disentangle(x, component))


@pytest.mark.parametrize("stage", ["spatial_cnn", "spatial_transformer", "mstct", "tenco"])
@pytest.mark.parametrize("train", [False, True])
def test_every_stage_parser_has_the_metrics_flag(stage, train):
    from computervision_codes_amd import drivers
    p = drivers._parser(stage, train)
    assert p.parse_known_args([])[0].metrics == "host"
    assert p.parse_known_args(["--metrics", "device"])[0].metrics == "device"
    with pytest.raises(SystemExit):
        p.parse_known_args(["--metrics", "gpu"])


def _ap_call(offsets, k, ld):
    """`mt4_video_ap_f32` on HOST buffers: every case here must be refused before a launch could read them"""
    from computervision_codes_amd import _lib
    buf = (ctypes.c_float * 16)()
    out = (ctypes.c_double * 16)()
    offs = (ctypes.c_int64 * len(offsets))(*offsets)
    return _lib.lib.mt4_video_ap_f32(ctypes.addressof(buf), ctypes.addressof(buf), offs, len(offsets) - 1, k, ld, ctypes.addressof(out), None)


def test_video_ap_refuses_bad_arguments_before_any_launch():
    from computervision_codes_amd import _lib
    cap = _lib.lib.mt4_video_ap_max_rows()
    assert cap >= 8192 and cap & (cap - 1) == 0
    assert _ap_call([0, 4], 7, 6) == -1                            # k > ld
    assert _ap_call([0, 4], 0, 6) == -1
    assert _ap_call([0, 4, 2], 6, 6) == -1                         # decreasing offsets
    assert _ap_call([-1, 4], 6, 6) == -1
    assert _ap_call([0, cap + 1], 6, 6) == _lib.MT4_EUNSUPPORTED == -4
    assert _ap_call([0, 3, 3, cap + 4], 6, 6) == -4
    assert _lib.lib.mt4_video_ap_f32(None, None, None, 1, 6, 6, None, None) == -1


def test_component_max_refuses_a_table_entry_outside_its_columns():
    from computervision_codes_amd import _lib
    buf = (ctypes.c_float * 100)()
    table, kc = metrics.component_table("v")
    call = lambda t, k: _lib.lib.mt4_component_max_f32(ctypes.addressof(buf), (ctypes.c_int32 * 100)(*t), k, ctypes.addressof(buf), 1, None)
    bad = table.copy()
    bad[17] = kc
    assert call(bad, kc) == -1
    bad[17] = -1
    assert call(bad, kc) == -1
    assert call(table, 101) == -1 and call(table, 0) == -1


def test_video_mean_is_what_compute_video_AP_returns():
    """a hand-built case: class 2 has no positives in any video (all NaN), class 1 only in the second video"""
    t0 = np.array([[1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]], dtype=np.float64)
    p0 = np.array([[.9, .1, .2], [.8, .2, .3], [.3, .3, .1], [.1, .4, .5]])
    t1 = np.array([[0, 1, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float64)
    p1 = np.array([[.5, .2, .2], [.4, .9, .3], [.6, .8, .1]])
    m = metrics.Recognition(3)
    for t, p in ((t0, p0), (t1, p1)):
        m.update(t, p)
        m.video_end()
    got = m.compute_video_AP()
    per_video = np.array([[(1 + 2 / 3) / 2, np.nan, np.nan], [1 / 3, (1 / 2 + 2 / 3) / 2, np.nan]])
    want = metrics.video_mean(per_video, 3)
    assert np.allclose(got["AP"][:2], [((1 + 2 / 3) / 2 + 1 / 3) / 2, (1 / 2 + 2 / 3) / 2], rtol=0, atol=1e-15) and np.isnan(got["AP"][2])
    assert np.array_equal(np.isnan(want["AP"]), np.isnan(got["AP"])) and np.allclose(want["AP"][:2], got["AP"][:2], rtol=0, atol=1e-15)
    assert abs(want["mAP"] - got["mAP"]) < 1e-15 and isinstance(want["mAP"], float)
    same = metrics.video_mean([m._ap_per_class(t0, p0), m._ap_per_class(t1, p1)], 3)
    assert np.array_equal(same["AP"], got["AP"], equal_nan=True) and same["mAP"] == got["mAP"]
    none = metrics.video_mean([], 3)                               # no videos: NaN per class, NaN mean (`Recognition` with nothing recorded)
    assert none["AP"].shape == (3,) and np.isnan(none["AP"]).all() and np.isnan(none["mAP"])
    empty = metrics.Recognition(3).compute_video_AP()
    assert np.isnan(empty["AP"]).all() and np.isnan(empty["mAP"])
