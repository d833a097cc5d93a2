"""CPU: the host side of localisation -- `ops.class_regions_host` (the contract `mt4_class_maps`' range and regions are held against on the GPU)
against an independent breadth-first search on hand-drawn maps, the C entry point's refusals, `Prediction` save / load with the localisation
arrays, the `.loc.csv` pixel arithmetic, and the refusals of the `predict.py` command line and of `Predictor` before any model runs."""
import csv
import ctypes

import numpy as np
import pytest
import torch

from class_map_patterns import FRACS, PATTERNS, bfs_region, tau_of
from computervision_codes_amd import _lib, drivers, ops
from computervision_codes_amd import predict as P


# ------------------------------------------------------------------------------------------------ class_regions_host
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_host_regions_equal_an_independent_search(name, frac):
    m = PATTERNS[name][0]
    regions, rng = ops.class_regions_host(m, frac)
    want, (mn, mx) = bfs_region(m, frac)
    assert regions.dtype == np.int32 and regions.shape == (8,) and rng.dtype == np.float32 and rng.shape == (2,)
    assert tuple(int(v) for v in regions) == want, (name, frac)
    assert rng[0] == mn and rng[1] == mx


def test_host_regions_take_a_stack_of_maps_and_tensors():
    ms = [PATTERNS[n][0] for n in ("two_blobs",)] * 2 + [np.flipud(PATTERNS["two_blobs"][0]).copy()]
    stack = np.stack(ms).reshape(3, 1, 6, 8)
    regions, rng = ops.class_regions_host(torch.from_numpy(stack), 0.5)
    assert regions.shape == (3, 1, 8) and rng.shape == (3, 1, 2)
    for i, m in enumerate(ms):
        assert tuple(int(v) for v in regions[i, 0]) == bfs_region(m, 0.5)[0]
    with pytest.raises(ValueError):
        ops.class_regions_host(stack, 1.5)
    with pytest.raises(ValueError):
        ops.class_regions_host(np.zeros(4, np.float32), 0.5)


def test_expected_shapes_of_the_drawn_cases():
    """what the drawings are for, stated once against the search itself (so a slip in a drawing does not pass silently on both sides)"""
    r = lambda n, f: bfs_region(PATTERNS[n][0], f)[0]
    assert r("two_blobs", 0.5) == (3, 5, 3, 4, 4, 6, 6, 0)                 # the peak's blob only: the other blob (values up to 7 >= tau = 3) is apart
    assert r("diagonal", 0.5) == (0, 0, 0, 0, 1, 1, 4, 0)                  # the corner contact does not join the blobs
    assert r("serpentine9", 0.5) == (0, 0, 0, 0, 8, 8, 49, 0)              # the whole path: 5 rows of 9 and 4 joints
    assert r("plateau", 1.0) == (1, 1, 1, 1, 1, 1, 1, 0)                   # tied maxima: the lowest index; the other maxima are apart
    assert r("plateau", 0.5) == (1, 1, 1, 1, 1, 3, 3, 0)
    assert r("constant", 0.5) == (0, 0, 0, 0, 3, 4, 20, 0) == r("constant", 1.0)
    assert r("borders", 0.5) == (5, 6, 0, 0, 5, 6, 22, 0)
    assert r("one_cell", 0.2) == (0, 0, 0, 0, 0, 0, 1, 0)
    assert r("row7", 0.5) == (0, 4, 0, 4, 0, 5, 2, 0) and r("row7", 0.0) == (0, 4, 0, 0, 0, 6, 7, 0)
    assert all(r(n, 0.0)[2:7] == (0, 0, m.shape[0] - 1, m.shape[1] - 1, m.size) for n, (m, _) in PATTERNS.items())     # frac 0: tau = min, the grid


def test_frac_one_whose_rounded_tau_exceeds_the_maximum_leaves_the_peak_alone():
    m = PATTERNS["frac1_above_max"][0]
    mn, mx = m.min(), m.max()
    assert tau_of(mn, mx, 1.0) > mx                                        # three rounded operations land one ulp above the maximum
    assert int((m == mx).sum()) == 3                                       # ... so not even the cells AT the maximum pass map >= tau
    regions, rng = ops.class_regions_host(m, 1.0)
    assert tuple(int(v) for v in regions) == (0, 2, 0, 2, 0, 2, 1, 0) and (rng[0], rng[1]) == (mn, mx)


# ------------------------------------------------------------------------------------------------ the C entry point without a device
def test_c_entry_point_refuses_before_any_launch():
    f = _lib.lib.mt4_class_maps
    p = 4096                                                               # (a non-null 16-byte aligned address: every case returns before it is looked at)
    ok = dict(feat=p, dtype=_lib.MT4_F32, w=p, col_lo=0, ncol=6, B=2, H=8, W=14, C=512, frac=0.5, maps=p, regions=p, range=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["feat"], a["dtype"], a["w"], a["col_lo"], a["ncol"], a["B"], a["H"], a["W"], a["C"], ctypes.c_float(a["frac"]), a["maps"], a["regions"],
                 a["range"], None)
    assert call(feat=None) == call(w=None) == call(maps=None) == call(regions=None) == call(range=None) == -1
    assert call(B=0) == call(H=0) == call(W=-1) == call(C=0) == call(ncol=0) == call(B=-3) == -1
    assert call(col_lo=-1) == -1
    assert call(frac=-0.01) == call(frac=1.01) == call(frac=float("nan")) == -1
    assert call(dtype=7) == -1
    assert call(feat=p + 8) == call(w=p + 4) == -2
    assert call(C=12) == call(C=4) == call(C=516) == -2
    assert call(H=33, W=32) == call(H=1025, W=1) == call(H=65536, W=65536) == -4
    assert call(ncol=257) == -4
    assert call(C=8200) == -4
    for dt in (_lib.MT4_F32, _lib.MT4_BF16):                               # the limits themselves are inside (checked as far as one can without a device:
        assert call(dtype=dt, feat=None, H=32, W=32, ncol=256, C=8192) == -1     # the null pointer is what is left to refuse)


def test_ops_class_maps_refuses_cpu_tensors_and_bad_arguments():
    feat, w = torch.zeros(1, 2, 3, 8), torch.zeros(6, 8)
    with pytest.raises(_lib.Mt4Error):
        ops.class_maps(feat, w, 0, 6, 0.5)


# ------------------------------------------------------------------------------------------------ Prediction with localisation
def _prediction(t=5, k=3, loc=True, maps=False, head="i", seed=0, cells=(2, 3), frame=(64, 96)):
    rng = np.random.default_rng(seed)
    s = rng.random((t, 100), dtype=np.float32)
    ids = np.argsort(-s, axis=1, kind="stable")[:, :k].astype(np.int32)
    z = (np.zeros(t, np.int32), np.zeros(t, np.float32))
    d = None
    if loc:
        h, w = cells
        y0, x0 = rng.integers(0, h, (t, k)), rng.integers(0, w, (t, k))
        y1, x1 = np.minimum(h - 1, y0 + rng.integers(0, h, (t, k))), np.minimum(w - 1, x0 + rng.integers(0, w, (t, k)))
        d = dict(peak=np.stack([y0, x0], -1), box=np.stack([y0, x0, y1, x1], -1), area=(y1 - y0 + 1) * (x1 - x0 + 1),
                 range=rng.standard_normal((t, k, 2)).astype(np.float32), cells=cells, frame=frame, head=head, frac=0.25,
                 maps=rng.standard_normal((t, k, h, w)).astype(np.float32) if maps else None)
    return P.Prediction([f"{i:06d}.png" for i in range(t)], ids, np.take_along_axis(s, ids, 1), (s > 0.5).sum(1), z, z, z, 0.5, None, d)


TODAY = sorted(["frames", "threshold", "topk_ids", "topk_scores", "n_active", "topk_ivt"] + [f"top_{h}_{w}" for h in "ivt" for w in ("ids", "scores")])
LOC_KEYS = ["loc_peak", "loc_box", "loc_area", "loc_range", "loc_cells", "loc_frame", "loc_head", "loc_frac"]


@pytest.mark.parametrize("maps", [False, True])
@pytest.mark.parametrize("head", ["i", "ivt"])
def test_prediction_with_localisation_round_trips(tmp_path, head, maps):
    pred = _prediction(maps=maps, head=head)
    stem = str(tmp_path / "VID01")
    pred.save(stem)
    assert sorted(np.load(stem + ".npz").files) == sorted(TODAY + LOC_KEYS + (["loc_maps"] if maps else []))
    back = P.Prediction.load(stem)
    for a, dt in (("loc_peak", np.int32), ("loc_box", np.int32), ("loc_area", np.int32), ("loc_range", np.float32)):
        assert getattr(back, a).dtype == dt and np.array_equal(getattr(back, a), getattr(pred, a)), a
    assert back.loc_peak.shape == (5, 3, 2) and back.loc_box.shape == (5, 3, 4) and back.loc_area.shape == (5, 3) and back.loc_range.shape == (5, 3, 2)
    assert (back.loc_cells, back.loc_frame, back.loc_head, back.loc_frac) == ((2, 3), (64, 96), head, 0.25)
    assert (back.loc_maps is None) == (not maps)
    if maps:
        assert back.loc_maps.dtype == np.float32 and np.array_equal(back.loc_maps, pred.loc_maps)
    assert np.array_equal(back.topk_ids, pred.topk_ids)


def test_prediction_without_localisation_keeps_todays_keys_and_writes_no_loc_csv(tmp_path):
    pred = _prediction(loc=False)
    stem = str(tmp_path / "VID02")
    pred.save(stem)
    assert sorted(np.load(stem + ".npz").files) == TODAY and not (tmp_path / "VID02.loc.csv").exists()
    back = P.Prediction.load(stem)
    assert back.loc_head is None and back.loc_peak is None and back.loc_maps is None


def test_prediction_refuses_localisation_arrays_of_the_wrong_shape():
    good = _prediction()
    d = dict(peak=good.loc_peak, box=good.loc_box, area=good.loc_area, range=good.loc_range, cells=(2, 3), frame=(64, 96), head="i", frac=0.5)
    z = (np.zeros(5, np.int32), np.zeros(5, np.float32))
    mk = lambda **kw: P.Prediction(good.frames, good.topk_ids, good.topk_scores, good.n_active, z, z, z, 0.5, None, dict(d, **kw))
    mk()
    for kw in (dict(peak=good.loc_peak[:, :2]), dict(box=good.loc_box[..., :3]), dict(area=good.loc_area[:4]), dict(head="v"),
               dict(maps=np.zeros((5, 3, 3, 2), np.float32))):
        with pytest.raises(ValueError):
            mk(**kw)


def test_loc_csv_is_in_resized_frame_pixels(tmp_path):
    """cell x covers [x W / w, (x + 1) W / w): a box is its outer edges, the peak its cell's centre; column = the head's column"""
    t, k = 2, 2
    ids = np.array([[17, 94], [0, 60]], dtype=np.int32)
    z = (np.zeros(t, np.int32), np.zeros(t, np.float32))
    peak = np.array([[[0, 0], [7, 13]], [[3, 5], [2, 2]]])
    box = np.array([[[0, 0, 0, 0], [6, 11, 7, 13]], [[0, 0, 7, 13], [2, 1, 4, 2]]])
    for head in ("i", "ivt"):
        d = dict(peak=peak, box=box, area=np.array([[1, 6], [112, 6]]), range=np.zeros((t, k, 2), np.float32), cells=(8, 14), frame=(256, 448), head=head,
                 frac=0.5)
        pred = P.Prediction(["a.png", "b.png"], ids, np.full((t, k), 0.5, np.float32), np.zeros(t, np.int32), z, z, z, 0.5, None, d)
        stem = str(tmp_path / f"v_{head}")
        pred.save(stem)
        rows = list(csv.reader(open(stem + ".loc.csv")))
        assert rows[0] == ["frame", "rank", "triplet", "column", "peak_x", "peak_y", "x0", "y0", "x1", "y1", "area"] and len(rows) - 1 == t * k
        col = (lambda tid: tid) if head == "ivt" else (lambda tid: P._TRIPLETS[tid][0])
        assert [r[:4] for r in rows[1:]] == [["a.png", "0", "17", str(col(17))], ["a.png", "1", "94", str(col(94))], ["b.png", "0", "0", str(col(0))],
                                            ["b.png", "1", "60", str(col(60))]]
        nums = [[float(v) for v in r[4:10]] for r in rows[1:]]
        assert nums[0] == [16.0, 16.0, 0.0, 0.0, 32.0, 32.0]                          # cell (0, 0) of 32 x 32 pixel cells
        assert nums[1] == [13.5 * 32, 7.5 * 32, 11 * 32, 6 * 32, 448.0, 256.0]        # the last cell's outer edge is the frame's
        assert nums[2] == [5.5 * 32, 3.5 * 32, 0.0, 0.0, 448.0, 256.0]
        assert nums[3] == [2.5 * 32, 2.5 * 32, 32.0, 64.0, 96.0, 160.0]
        assert [r[10] for r in rows[1:]] == ["1", "6", "112", "6"]
    d = dict(d, cells=(3, 4), frame=(64, 100), peak=np.zeros((t, k, 2), int), box=np.tile(np.array([0, 1, 2, 2]), (t, k, 1)))      # cells of 21.33 x 25 pixels
    pk, bx = P.Prediction(["a.png", "b.png"], ids, np.full((t, k), 0.5, np.float32), np.zeros(t, np.int32), z, z, z, 0.5, None, d).loc_pixels()
    assert np.allclose(pk[0, 0], [12.5, 64 / 6]) and np.allclose(bx[0, 0], [25.0, 0.0, 75.0, 64.0])


# ------------------------------------------------------------------------------------------------ refusals: the command line and the constructor
def test_predict_parser_localize_defaults():
    F = drivers._predict_parser().parse_known_args([])[0]
    assert (F.localize, F.localize_frac, F.save_maps) == ("off", 0.5, False)
    F = drivers._predict_parser().parse_known_args(["--localize", "ivt", "--localize_frac", "0.3", "--save_maps"])[0]
    assert (F.localize, F.localize_frac, F.save_maps) == ("ivt", 0.3, True)
    with pytest.raises(SystemExit):
        drivers._predict_parser().parse_known_args(["--localize", "v"])


def test_predict_refuses_bad_localize_flags_before_any_model_is_built(tmp_path, monkeypatch):
    def built(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(drivers, "_eval_model", built)
    ckpt = tmp_path / "student.pth"
    ckpt.write_bytes(b"x")
    frames = tmp_path / "vid"
    frames.mkdir()
    (frames / "000000.png").write_bytes(b"x")
    good = ["--student_ckpt", str(ckpt), "--frames_dir", str(frames), "--out", str(tmp_path / "out")]
    for argv, flag in ((good + ["--save_maps"], "--save_maps"),
                       (good + ["--localize", "i", "--localize_frac", "1.5"], "--localize_frac"),
                       (good + ["--localize", "ivt", "--localize_frac", "-0.1"], "--localize_frac"),
                       (good + ["--localize", "i", "--loss_type", "ivt"], "--localize"),
                       (good + ["--localize", "ivt", "--loss_type", "i"], "--localize")):
        with pytest.raises(ValueError) as e:
            drivers.predict(argv)
        assert flag in str(e.value), (argv, str(e.value))
    for tail in (["--localize", "i"], ["--localize", "ivt", "--loss_type", "ivt", "--save_maps"], ["--localize", "i", "--localize_frac", "1"]):
        with pytest.raises(AssertionError, match="a model was built"):                     # (good command lines do get that far)
            drivers.predict(good + tail)
    assert not (tmp_path / "out").exists()


class _Student:
    def __init__(self, heads):
        self._head_slices, self.loss_type, o = {}, "+".join(heads), 0
        for h, n in (("i", 6), ("v", 10), ("t", 15), ("ivt", 100)):
            if h in heads:
                self._head_slices[h] = (o, o + n)
                o += n

    def eval(self):
        return self


def test_predictor_refuses_in_the_constructor():
    full, only_ivt = _Student(("i", "v", "t", "ivt")), _Student(("ivt",))
    for head in (None, "i", "ivt"):
        assert P.Predictor(full, localize=head).localize == head
    assert P.Predictor(only_ivt, localize="ivt", localize_frac=1.0, localize_maps=True).localize_maps
    for student, kw in ((only_ivt, dict(localize="i")), (_Student(("i",)), dict(localize="ivt")), (full, dict(localize="v")),
                        (full, dict(localize="i", localize_frac=1.2)), (full, dict(localize="i", localize_frac=-0.5)), (full, dict(localize_maps=True))):
        with pytest.raises(ValueError, match="localize"):
            P.Predictor(student, **kw)
