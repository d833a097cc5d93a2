"""CPU: the 'brightness' augmentation (the reference's `RandomAdjustSharpness(1.6, p=0.5)`) on the host path (`drivers._augment`) and in
the host side of the device transform (`augment.py`): the draw, the parameter column, the integer arithmetic against
`ImageEnhance.Sharpness(im).enhance(1.6)` itself, and the lists that keep the host transform."""
import argparse
import os
import random

import numpy as np
import pytest

from computervision_codes_amd import augment

DEFAULT = ["original", "vflip", "hflip", "contrast", "rot90"]
LISTS = [["original", "vflip", "hflip", "contrast", "brightness", "rot90"], ["brightness", "contrast", "rot90"],
         ["vflip", "brightness", "hflip"], ["brightness"]]
NO_DEVICE_FORM = [["rot90", "brightness"], ["brightness", "brightness"]]
SIZES = [(37, 53), (256, 448), (384, 384)]
SEED = 5                                                               # (the tests assert that its draws cover every combination)


class Scripted:
    """an rng that returns what the test scripted: `random()` and `uniform()` pop from their own queues"""

    def __init__(self, randoms, angles):
        self.randoms, self.angles = list(randoms), list(angles)

    def random(self):
        return self.randoms.pop(0)

    def uniform(self, a, b):
        return self.angles.pop(0)


def _write_frames(tmp_path, n, h0, w0, seed=0):
    """n PNGs of h0 x w0 in the dataset's layout, uniform random bytes; frame 1 has a constant green channel, frame 2 a narrow value range"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    d = tmp_path / "data" / "VID01"
    os.makedirs(d, exist_ok=True)
    for i in range(n):
        a = rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)
        if i == 1:
            a[..., 1] = 77
        if i == 2:
            a = (a // 3 + 40).astype(np.uint8)
        Image.fromarray(a).save(d / f"{i:06d}.png")
    return str(tmp_path), "VID01", list(range(n))


def _pillow_sharp(a):
    from PIL import Image, ImageEnhance
    return np.asarray(ImageEnhance.Sharpness(Image.fromarray(np.ascontiguousarray(a))).enhance(1.6))


def _assert_both_clamps(want):
    """both clamps of the blend occur in at least 1 % of the interior bytes of PILLOW's result: arithmetic without them cannot pass"""
    inner = want[1:-1, 1:-1]
    assert (inner == 0).mean() >= 0.01 and (inner == 255).mean() >= 0.01, ((inner == 0).mean(), (inner == 255).mean())


# ------------------------------------------------------------------------------------------------ 1. the host path
def test_host_augment_sharpens_like_pillow():
    from PIL import Image
    from computervision_codes_amd import drivers
    im = Image.fromarray(np.random.default_rng(3).integers(0, 256, (37, 53, 3), dtype=np.uint8))
    want = _pillow_sharp(np.asarray(im))
    _assert_both_clamps(want)
    got = np.asarray(drivers._augment(im, Scripted([0.0], []), ["brightness"]))
    assert np.array_equal(got, want) and not np.array_equal(got, np.asarray(im))
    rng = Scripted([0.5], [])
    assert np.array_equal(np.asarray(drivers._augment(im, rng, ["brightness"])), np.asarray(im)) and not rng.randoms     # drawn, not taken
    rng = Scripted([0.0, 0.9], [])                                    # one draw per occurrence
    assert np.array_equal(np.asarray(drivers._augment(im, rng, ["brightness", "brightness"])), want) and not rng.randoms


# ------------------------------------------------------------------------------------------------ 2. the draws
@pytest.mark.parametrize("names", LISTS)
@pytest.mark.parametrize("seed", [1, 7, 47])
def test_draw_params_consumes_the_rng_like_augment(seed, names):
    from PIL import Image
    from computervision_codes_amd import drivers
    a, b = random.Random(seed), random.Random(seed)
    im = Image.fromarray(np.zeros((8, 12, 3), np.uint8))
    for _ in range(9):
        drivers._augment(im, a, names)
    p = augment.draw_params(b, names, 9, 8, 12)
    assert a.getstate() == b.getstate() and p.table.shape == (9, augment.NPARAMS) and augment.NPARAMS == 12


@pytest.mark.parametrize("names", LISTS)
def test_sharpen_column_takes_both_values_and_encodes_the_order(names):
    p = augment.draw_params(random.Random(SEED), names, 12, 8, 12)
    col = p.table[:, 11]
    assert (col == 0).any() and (col != 0).any()
    contrast_first = "contrast" in names and names.index("contrast") < names.index("brightness")
    for c, s in zip(p.table[:, 10].tolist(), col.tolist()):
        assert s in (0, 1, 2) and (s == 2) == (bool(s) and bool(c) and contrast_first)
    # the draw itself: random() < 0.5 at the name's position
    q = augment.draw_params(Scripted([0.49, 0.5], []), ["brightness"], 2, 8, 12)
    assert q.table[:, 11].tolist() == [1, 0]
    q = augment.draw_params(Scripted([0.1, 0.1, 0.9, 0.1, 0.1, 0.9, 0.9, 0.9], []), ["contrast", "brightness"], 4, 8, 12)
    assert q.table[:, 10].tolist() == [1, 0, 1, 0] and q.table[:, 11].tolist() == [2, 1, 0, 0]
    q = augment.draw_params(Scripted([0.1, 0.1, 0.1, 0.9], []), ["brightness", "contrast"], 2, 8, 12)
    assert q.table[:, 10].tolist() == [1, 0] and q.table[:, 11].tolist() == [1, 1]


def _parent_draw_params(rng, names, n, h, w):
    """the rows of the default list as the code before 'brightness' built them (column 11 = 0)"""
    table = np.zeros((n, 12), np.int32)
    for i in range(n):
        vflip = hflip = contrast = 0
        fx, nw, nh = [65536, 0, 32768, 0, 65536, 32768], w, h
        for name in names:
            if name == "vflip" and rng.random() < 0.4:
                vflip ^= 1
            elif name == "hflip" and rng.random() < 0.4:
                hflip ^= 1
            elif name == "contrast" and rng.random() < 0.5:
                contrast = 1
            elif name == "rot90":
                fx, nw, nh = augment.rotation_row(rng.uniform(-90.0, 90.0), h, w)
        table[i] = (vflip, hflip, *fx, nw, nh, contrast, 0)
    return table


@pytest.mark.parametrize("seed", [1, 7, 47])
def test_rows_of_the_default_list_are_unchanged(seed):
    p = augment.draw_params(random.Random(seed), DEFAULT, 12, 256, 448)
    assert np.array_equal(p.table, _parent_draw_params(random.Random(seed), DEFAULT, 12, 256, 448)) and not p.table[:, 11].any()
    small = augment.draw_params(random.Random(seed), DEFAULT, 12, 8, 8)
    assert "sharp" not in augment.reference_u8(np.zeros((12, 8, 8, 3), np.uint8), small, stages=True)


# ------------------------------------------------------------------------------------------------ 3. Pillow comparison
@pytest.mark.parametrize("names", LISTS)
@pytest.mark.parametrize("h,w", SIZES)
def test_reference_equals_pillow_path(tmp_path, h, w, names):
    from computervision_codes_amd import cholect, drivers
    n = 12
    data, video, ids = _write_frames(tmp_path, n, h + 11, w - 9)
    want = drivers.load_train_frames_u8(data, video, ids, h, w, random.Random(SEED), names)
    frames = cholect.load_frames_u8(data, video, ids, h, w)
    p = augment.draw_params(random.Random(SEED), names, n, h, w)
    combos = {(bool(c), bool(s)) for c, s in zip(p.table[:, 10].tolist(), p.table[:, 11].tolist())}
    if "contrast" in names:
        assert combos == {(False, False), (False, True), (True, False), (True, True)}       # sharpen x contrast: all four
    else:
        assert combos == {(False, False), (False, True)}
    st = augment.reference_u8(frames, p, stages=True)
    assert np.array_equal(st["out"], want)
    assert st["sharp"].shape == frames.shape
    for i in range(n):
        if not p.table[i, 11]:
            assert np.array_equal(st["sharp"][i], frames[i]), i
        elif p.table[i, 11] == 1:
            assert np.array_equal(st["sharp"][i], _pillow_sharp(frames[i])), i
    assert np.array_equal(augment.reference_u8(frames, p), want)


def test_reference_with_scripted_draws_on_the_constant_and_narrow_frames(tmp_path):
    """frames 1 (constant channel) and 2 (narrow range) with contrast AND sharpening drawn, in both orders"""
    from computervision_codes_amd import cholect, drivers
    h, w = 37, 53
    data, video, ids = _write_frames(tmp_path, 4, h + 11, w - 9)
    frames = cholect.load_frames_u8(data, video, ids, h, w)
    for names in (["contrast", "brightness"], ["brightness", "contrast"], ["contrast", "brightness", "rot90"], ["brightness", "contrast", "rot90"]):
        randoms, angles = [0.1, 0.1] * 4, [33.0, -71.5, 0.0, 90.0]
        want = drivers.load_train_frames_u8(data, video, ids, h, w, Scripted(randoms, angles), names)
        p = augment.draw_params(Scripted(randoms, angles), names, 4, h, w)
        assert p.table[:, 11].tolist() == [2 if names[0] == "contrast" else 1] * 4
        assert np.array_equal(augment.reference_u8(frames, p), want), names


BARE_SIZES = ([(3, 3), (2, 5), (5, 2), (1, 1), (5, 4)]
              + [(augment.SHARP_ROWS + d, 9) for d in (-1, 0, 1)] + [(7, augment.SHARP_COLS + d) for d in (-1, 0, 1)]
              + [(2 * augment.SHARP_ROWS + 1, 2 * augment.SHARP_COLS + 1)])


@pytest.mark.parametrize("h,w", BARE_SIZES)
def test_bare_stage_equals_pillow(h, w):
    g = np.random.default_rng(h * 1000 + w)
    for kind in range(3):
        a = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if kind == 1:
            a[..., 1] = 77
        if kind == 2:
            a = (a // 3 + 40).astype(np.uint8)
        want = _pillow_sharp(a)
        got = augment.sharpen_u8(a)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (h, w, kind)
        if h < 3 or w < 3:
            assert np.array_equal(got, a)
        else:
            assert np.array_equal(got[0], a[0]) and np.array_equal(got[-1], a[-1]) and np.array_equal(got[:, 0], a[:, 0]) \
                and np.array_equal(got[:, -1], a[:, -1])                                  # the border is the source
            if kind == 0:
                assert not np.array_equal(got, a)


def test_both_clamps_occur_in_pillows_result_on_random_frames():
    a = np.random.default_rng(9).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    want = _pillow_sharp(a)
    _assert_both_clamps(want)
    assert np.array_equal(augment.sharpen_u8(a), want)


def test_sharpening_commutes_with_both_flips():
    a = np.random.default_rng(2).integers(0, 256, (11, 14, 3), dtype=np.uint8)
    s = augment.sharpen_u8(a)
    assert np.array_equal(augment.sharpen_u8(a[::-1].copy()), s[::-1]) and np.array_equal(augment.sharpen_u8(a[:, ::-1].copy()), s[:, ::-1])


# ------------------------------------------------------------------------------------------------ 4. supported and the fallback
def test_supported_lists_and_the_fallback_line(capsys, monkeypatch, tmp_path):
    from computervision_codes_amd import cholect, drivers
    assert all(augment.supported(names) for names in LISTS)
    h, w = 16, 20
    data, video, ids = _write_frames(tmp_path, 2, h, w)
    frames = cholect.load_frames_u8(data, video, ids, h, w)
    for names in NO_DEVICE_FORM:
        monkeypatch.setattr(drivers, "_WARNED_TRANSFORM", False)
        capsys.readouterr()
        assert not augment.supported(names)
        with pytest.raises(ValueError, match="brightness"):
            augment.draw_params(random.Random(0), names, 1, 8, 8)
        F = argparse.Namespace(train_transform="device", augmentation_list=names)
        assert not drivers._device_transform(F) and not drivers._device_transform(F)
        out = capsys.readouterr().out
        assert out.count("--train_transform device") == 1 and "brightness" in out              # said once
    # the host path still produces Pillow's bytes for them
    got = drivers.load_train_frames_u8(data, video, ids, h, w, Scripted([0.1, 0.1, 0.9, 0.1], []), ["brightness", "brightness"])
    assert np.array_equal(got[0], _pillow_sharp(_pillow_sharp(frames[0]))) and np.array_equal(got[1], _pillow_sharp(frames[1]))
    from PIL import Image
    got = drivers.load_train_frames_u8(data, video, ids[:1], h, w, Scripted([0.1], [30.0]), ["rot90", "brightness"])
    rot = Image.fromarray(frames[0]).rotate(30.0, resample=Image.NEAREST, expand=True)
    assert np.array_equal(got[0], np.asarray(Image.fromarray(_pillow_sharp(np.asarray(rot))).resize((w, h), Image.BILINEAR)))
    assert drivers._device_transform(argparse.Namespace(train_transform="device", augmentation_list=LISTS[0]))
