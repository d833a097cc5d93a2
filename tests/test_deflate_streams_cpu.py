"""The constructed DEFLATE streams and scanline cases of `deflate_streams.py`, checked without a GPU: zlib inflates every stream to the bytes
its row expects, the census finds in it what the row says it tests, and the table as a whole covers every form it exists for.  The scanline
reference is tied to Pillow.  `test_gpu_png_streams.py` runs the same rows through the kernels."""
import io
import zlib

import numpy as np
import pytest

import deflate_streams as ds

NAMES = [c[0] for c in ds.CASES]


@pytest.fixture(scope="module")
def reports():
    return {name: ds.census(s) for name, (s, _, _) in ds.build_all().items()}


@pytest.mark.parametrize("name", NAMES)
def test_zlib_inflates_the_stream_to_the_expected_bytes(name):
    s, expected, _ = ds.build_all()[name]
    d = zlib.decompressobj(-15)
    assert d.decompress(s[:-4]) == expected
    assert d.eof and d.unused_data == b""                       # the body ends with its final block, nothing behind it but the trailer
    assert int.from_bytes(s[-4:], "big") == zlib.adler32(expected)


@pytest.mark.parametrize("name", NAMES)
def test_census_finds_what_the_row_names(name, reports):
    s, expected, feats = ds.build_all()[name]
    rep = reports[name]
    assert rep["error"] is None and rep["adler_ok"] and rep["out"] == expected
    missing = feats - ds.features(rep)
    assert not missing, (name, sorted(missing))


def test_the_table_covers_every_required_form(reports):
    seen = set().union(*(ds.features(r) for r in reports.values()))
    assert not (ds.REQUIRED - seen), sorted(ds.REQUIRED - seen)
    asked = set().union(*(c[2] for c in ds.CASES))
    assert not (ds.REQUIRED - asked), sorted(ds.REQUIRED - asked)        # and each is some row's stated purpose, not a by-product
    # every (stream length + start alignment) mod 512 around a 512-byte chunk edge, for a short and a long stream
    for tag in ("short", "long"):
        for a in range(4):
            for t in (508, 509, 510, 511, 0, 1, 4):
                assert f"streamlen%512={(t - a) % 512}/{tag}" in seen


def test_names_are_unique_and_streams_stay_small():
    assert len(set(NAMES)) == len(NAMES)
    for name, (s, _, _) in ds.build_all().items():
        assert len(s) <= (150 << 10 if name == "zlib_level0_140000" else 70 << 10), (name, len(s))


@pytest.mark.parametrize("name,build,status", ds.REJECTED)
def test_rejected_streams_fail_on_a_checked_condition(name, build, status):
    s, _ = build()
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(s[:-4])
    rep = ds.census(s)
    assert rep["error"] == "no end-of-block code" and rep["blocks"][0]["hclen"] == 4 and rep["blocks"][0]["hlit"] == 257


def test_census_reads_streams_it_did_not_write():
    data = ds._scanlines(30000)
    for level in (1, 6, 9):
        z = zlib.compress(data, level)
        rep = ds.census(z[2:])                                  # header stripped, Adler-32 kept: as `parse_png` leaves it
        assert rep["error"] is None and rep["adler_ok"] and len(rep["out"]) == len(data) and rep["out"] == data
        assert "dynamic" in ds.features(rep) and "matches" in ds.features(rep)
    rep = ds.census(zlib.compress(data, 6)[2:-9] + b"\0\0\0\0")          # cut short: reported, not raised
    assert rep["error"] is not None


def test_writer_refuses_bad_code_length_sets():
    ok = [8] * 255 + [0, 8]
    ds.body([ds.Dynamic(ok, [0], [1, 2, 3])])
    ds.body([ds.Dynamic(ok, [1], [1, 2, 3])])
    with pytest.raises(ds.OverSubscribed):
        ds.body([ds.Dynamic([8] * 257, [0], [1])])
    with pytest.raises(ds.Incomplete):
        ds.body([ds.Dynamic([8] * 254 + [0, 0, 8], [0], [1])])
    with pytest.raises(ds.OverSubscribed):
        ds.body([ds.Dynamic(ok, [1, 1, 1], [1])])
    with pytest.raises(ds.Incomplete):                          # two distance codes that leave half the code space unused
        ds.body([ds.Dynamic(ok, [2, 2], [1])])
    with pytest.raises(ds.Incomplete):                          # one distance code, but not of length 1
        ds.body([ds.Dynamic(ok, [2], [1])])
    with pytest.raises(ds.BadLengths):                          # no end-of-block code
        ds.body([ds.Dynamic([8] * 256 + [0], [0], [1])])
    with pytest.raises(ds.BadLengths):                          # a sequence that does not say what the lengths say
        ds.body([ds.Dynamic(ok, [0], [1], cl_items=[(8, None)] * 258)])


def test_code_length_sequence_symbol_by_symbol_and_hclen():
    """the same block with its lengths sent one symbol each (no runs) and with runs: both inflate alike; HCLEN as asked"""
    ll = ds.balanced_lengths(260, list(range(97, 123)) + [256])
    toks = list(b"symbol by symbol".replace(b" ", b"q"))
    plain = ds.stream([ds.Dynamic(ll, [0], toks, cl_items=[(l, None) for l in ll + [0]])])
    runs = ds.stream([ds.Dynamic(ll, [0], toks, hclen=19)])
    assert len(plain) > len(runs)
    for s in (plain, runs):
        assert zlib.decompressobj(-15).decompress(s[:-4]) == bytes(toks)
    assert not ds.census(plain)["blocks"][0]["crossing"] and ds.census(runs)["blocks"][0]["crossing"] == [(17, 0)]
    assert ds.census(runs)["blocks"][0]["hclen"] == 19


def test_idat_spans_refuses_width_4097():
    from computervision_codes_amd import pngdec
    raw = ds.filter_rows(np.zeros((1, 4096, 3), np.uint8), [0])
    assert pngdec._idat_spans(ds.png_file(raw, 1, 4096))[:2] == (4096, 1)
    wide = ds.filter_rows(np.zeros((1, 4097, 3), np.uint8), [0])
    with pytest.raises(pngdec.UnsupportedPng):
        pngdec._idat_spans(ds.png_file(wide, 1, 4097))


@pytest.mark.parametrize("h,w", ds.FILTER_SHAPES)
def test_unfilter_ref_equals_pillow(h, w):
    from PIL import Image
    kinds = set()
    for name, raw in ds.filter_cases(h, w):
        assert len(raw) == h * (1 + 3 * w)
        kinds.update(raw[y * (1 + 3 * w)] for y in range(h))
        got = np.asarray(Image.open(io.BytesIO(ds.png_file(raw, h, w))))
        assert got.shape == (h, w, 3) and np.array_equal(got, ds.unfilter_ref(raw, h, w)), (name, h, w)
    assert kinds == {0, 1, 2, 3, 4}


def test_forward_filter_round_trip_and_the_crafted_neighbourhoods():
    """`filter_rows` then `unfilter_ref` is the identity; and the crafted images do hold what they are for: Paeth's three ties, sums that wrap
    mod 256, Average sums that need the ninth bit"""
    h, w = 5, 22
    imgs = ds._filter_images(h, w)
    for img in imgs.values():
        for t in range(5):
            assert np.array_equal(ds.unfilter_ref(ds.filter_rows(img, [t] * h), h, w), img)
    t = imgs["ties"].astype(int)
    a, b, c = t[1:, :-1], t[:-1, 1:], t[:-1, :-1]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    assert ((a == b) & (b == c)).any() and ((a == b) & (b != c)).any() and ((pa == pc) & (pa < pb)).any() and ((pb == pc) & (pb < pa)).any()
    assert (a[0, 0, 0], b[0, 0, 0], c[0, 0, 0]) == (6, 12, 10)
    hi = imgs["high"].astype(int)
    assert (hi[1:, :-1] + hi[:-1, 1:] >= 256).all()
    for ft in (1, 2, 3, 4):                                      # filtered byte + predictor passes 255 somewhere in every predicted type
        raw = np.frombuffer(ds.filter_rows(imgs["high"], [ft] * h), np.uint8).reshape(h, 1 + 3 * w)[:, 1:].astype(int)
        assert ((hi.reshape(h, 3 * w) - raw) % 256 + raw >= 256).any()


def test_png_file_splits_the_idat_payload_as_asked():
    from computervision_codes_amd import pngdec
    h, w = 2, 4096
    raw = ds.filter_cases(h, w)[5][1]
    f = ds.png_file(raw, h, w, idat_sizes=(2, 1, 1, 7, 4096), empty_between=True, ancillary=True)
    assert f.index(b"tEXt") < f.index(b"pHYs") < f.index(b"IDAT")
    assert f.count(b"IDAT") == 11                                # six pieces, an empty chunk between any two
    w2, h2, spans = pngdec._idat_spans(f)
    assert (w2, h2) == (w, h) and [n for _, n in spans][:5] == [2, 1, 1, 7, 4096] and len(spans) == 6
    assert pngdec.parse_png(f)[2] == zlib.compress(raw, 6)[2:]
    assert np.array_equal(np.asarray(__import__("PIL.Image").Image.open(io.BytesIO(f))), ds.unfilter_ref(raw, h, w))
