"""`mt4_png_inflate` and `mt4_png_unfilter_rgb8` called directly on the constructed streams and forced filters of `deflate_streams.py`
(`test_deflate_streams_cpu.py` checks the same rows against zlib and Pillow), then the hand-assembled files through `pngdec`.  Every
comparison is byte equality or an exact status code: a valid stream the decoder rejects is a failure."""
import numpy as np
import pytest
import torch

import deflate_streams as ds

pytestmark = pytest.mark.gpu

MT4_OK, MT4_EUNSUPPORTED = 0, -4
POISON = 0xCD


def _by_raw_len():
    groups = {}
    for name, (s, expected, _) in ds.build_all().items():
        groups.setdefault(len(expected), []).append(name)
    return groups


GROUPS = _by_raw_len()


def _inflate(cuda, placed, raw_len):
    """one launch of `mt4_png_inflate` the way `pngdec._decode_streams` makes it.  placed: [(stream bytes, start alignment 0..3)]; stream i lies
    in the blob at an offset = its alignment mod 4, behind the last one 1 KB of zeros.  -> (status [B], raw rows [B, raw_stride]) on the host"""
    from computervision_codes_amd import ops
    from computervision_codes_amd._lib import lib
    offsets, cursor = [], 0
    for s, a in placed:
        cursor = (cursor + 3) // 4 * 4 + a
        offsets.append(cursor)
        cursor += len(s)
    blob = np.zeros(cursor + 1024, np.uint8)
    for (s, _), o in zip(placed, offsets):
        blob[o:o + len(s)] = np.frombuffer(s, np.uint8)
    n = len(placed)
    raw_stride = (raw_len + 15) // 16 * 16
    streams = torch.from_numpy(blob).to(cuda)
    assert streams.data_ptr() % 4 == 0
    offs = torch.tensor(offsets, dtype=torch.int64, device=cuda)
    lens = torch.tensor([len(s) for s, _ in placed], dtype=torch.int32, device=cuda)
    raw = torch.full((n, raw_stride), POISON, dtype=torch.uint8, device=cuda)
    status = torch.zeros(n, dtype=torch.int32, device=cuda)
    code = lib.mt4_png_inflate(streams.data_ptr(), offs.data_ptr(), lens.data_ptr(), raw.data_ptr(), n, raw_stride, raw_len, status.data_ptr(),
                               ops._stream())
    assert code == MT4_OK
    torch.cuda.synchronize()
    return status.cpu().numpy(), raw.cpu().numpy()


@pytest.mark.parametrize("raw_len", sorted(GROUPS), ids=lambda n: f"len{n}")
def test_every_case_at_every_start_alignment(cuda, raw_len):
    """the rows that share an output length in ONE launch, each at all four start alignments (`mis` of the bit reader) side by side"""
    cases = ds.build_all()
    placed = [(name, a) for name in GROUPS[raw_len] for a in range(4)]
    status, raw = _inflate(cuda, [(cases[name][0], a) for name, a in placed], raw_len)
    for i, (name, a) in enumerate(placed):
        assert status[i] == 0, (name, a, int(status[i]))
    for i, (name, a) in enumerate(placed):
        expected = np.frombuffer(cases[name][1], np.uint8)
        same = raw[i, :raw_len] == expected
        assert same.all(), (name, a, "first wrong byte", int(np.argmin(same)), "of", raw_len)
        assert (raw[i, raw_len:] == POISON).all(), (name, a, "bytes behind the output were written")


def test_shortest_and_longest_stream_of_one_length_mixed_equal_each_alone(cuda):
    """a wave's ring, tables and bit reader are its own: for every output length that several rows share, the row with the shortest and the one
    with the longest stream, interleaved in one batch, give the bytes each gives alone"""
    cases = ds.build_all()
    shared = {n: names for n, names in GROUPS.items() if len(names) >= 2}
    assert len(shared) >= 3
    for raw_len, names in sorted(shared.items()):
        by_size = sorted(names, key=lambda k: len(cases[k][0]))
        short, long_ = by_size[0], by_size[-1]
        alone = {k: _inflate(cuda, [(cases[k][0], 0)], raw_len) for k in (short, long_)}
        order = [short, long_, long_, short, long_, short, short, long_]
        status, raw = _inflate(cuda, [(cases[k][0], i % 4) for i, k in enumerate(order)], raw_len)
        assert not status.any(), (raw_len, status)
        for i, k in enumerate(order):
            assert alone[k][0][0] == 0
            assert np.array_equal(raw[i], alone[k][1][0]), (raw_len, k, i)
            assert raw[i, :raw_len].tobytes() == cases[k][1]


@pytest.mark.parametrize("name,build,expect", ds.REJECTED)
def test_rejected_streams_give_their_status(cuda, name, build, expect):
    s, _ = build()
    status, _ = _inflate(cuda, [(s, a) for a in range(4)], 16)
    assert (status == expect).all(), (name, status)


# ---------------------------------------------------------------------------------------------------------------- scanline filters

def _unfilter(cuda, rows, h, w):
    """one launch of `mt4_png_unfilter_rgb8` on [raw scanline bytes of one frame each] -> (return code, status [B], frames [B, h, w, 3])"""
    from computervision_codes_amd import ops
    from computervision_codes_amd._lib import lib
    raw_len = h * (1 + 3 * w)
    raw_stride = (raw_len + 15) // 16 * 16
    host = np.full((len(rows), raw_stride), POISON, np.uint8)
    for i, r in enumerate(rows):
        assert len(r) == raw_len
        host[i, :raw_len] = np.frombuffer(r, np.uint8)
    raw = torch.from_numpy(host).to(cuda)
    out = torch.full((len(rows), h, w, 3), POISON, dtype=torch.uint8, device=cuda)
    status = torch.zeros(len(rows), dtype=torch.int32, device=cuda)
    code = lib.mt4_png_unfilter_rgb8(raw.data_ptr(), out.data_ptr(), len(rows), h, w, raw_stride, status.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    return code, status.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("h,w", ds.FILTER_SHAPES)
def test_forced_filters_match_the_specification(cuda, h, w):
    """every filter type on every row (the first included: up = 0), the five types cycled from each start; random filtered bytes, Paeth ties,
    wrapping sums, Average's ninth bit -- all cases of one frame size in one launch, against `unfilter_ref` (tied to Pillow on the CPU)"""
    cases = ds.filter_cases(h, w)
    code, status, got = _unfilter(cuda, [raw for _, raw in cases], h, w)
    assert code == MT4_OK and not status.any()
    for i, (name, raw) in enumerate(cases):
        ref = ds.unfilter_ref(raw, h, w)
        same = got[i] == ref
        assert same.all(), (name, h, w, "first wrong byte", int(np.argmin(same)))


def test_width_4097_is_unsupported_and_filter_type_5_is_reported(cuda):
    from computervision_codes_amd import pngdec
    code, status, _ = _unfilter(cuda, [bytes(1 + 3 * 4097)], 1, 4097)
    assert code == MT4_EUNSUPPORTED and not status.any()
    h, w = 5, 22
    good = ds.filter_cases(h, w)[0][1]
    rows = [good]
    for y in range(h):                                           # filter byte 5 in row y: every access stays in bounds, the frame is reported
        bad = bytearray(good)
        bad[y * (1 + 3 * w)] = 5
        rows.append(bytes(bad))
    code, status, got = _unfilter(cuda, rows + [good], h, w)
    assert code == MT4_OK and status.tolist() == [0] + [8] * h + [0]
    assert np.array_equal(got[0], ds.unfilter_ref(good, h, w)) and np.array_equal(got[-1], got[0])
    # and through the front door: a real file whose third row has filter type 5 is a DecodeError
    bad = bytearray(good)
    bad[2 * (1 + 3 * w)] = 5
    with pytest.raises(pngdec.DecodeError, match="code 8"):
        pngdec.decode_batch([ds.png_file(good, h, w), ds.png_file(bytes(bad), h, w)], cuda)


# ---------------------------------------------------------------------------------------------------------------- whole files

SPLIT = (2, 1, 1, 7, 4096)


@pytest.mark.parametrize("h,w", [(2, 4096), (5, 43)])
def test_hand_assembled_files_through_decode_batch_and_decode_files(cuda, tmp_path, h, w):
    """IDAT payload in chunks of 2, 1, 1, 7 and 4096 bytes, empty IDAT chunks between them, tEXt and pHYs in front: both paths give what the
    specification says (at 5 x 43 the stream ends inside the 4096-byte chunk's place: fewer, shorter chunks)"""
    from computervision_codes_amd import pngdec
    cases = ds.filter_cases(h, w)
    files = [ds.png_file(raw, h, w, idat_sizes=SPLIT, empty_between=bool(i % 2), ancillary=bool(i % 3)) for i, (_, raw) in enumerate(cases)]
    files.append(ds.png_file(cases[0][1], h, w))                 # and a plain one among them
    ref = np.stack([ds.unfilter_ref(raw, h, w) for _, raw in cases] + [ds.unfilter_ref(cases[0][1], h, w)])
    if w == 4096:
        assert [n for _, n in pngdec._idat_spans(files[0])[2]][:5] == list(SPLIT)
    got = pngdec.decode_batch(files, cuda).cpu().numpy()
    assert np.array_equal(got, ref)
    paths = []
    for i, f in enumerate(files):
        p = tmp_path / f"{i:04d}.png"
        p.write_bytes(f)
        paths.append(str(p))
    got = pngdec.decode_files(paths, cuda, workers=3).cpu().numpy()
    assert np.array_equal(got, ref)


def test_first_idat_of_one_byte_is_refused_by_both_paths(cuda, tmp_path):
    """the zlib header split over two chunks: legal, written by no encoder, and documented as left to the caller's fallback"""
    from computervision_codes_amd import pngdec
    h, w = 2, 21
    raw = ds.filter_cases(h, w)[3][1]
    f = ds.png_file(raw, h, w, idat_sizes=(1, 1, 5))
    from PIL import Image
    import io
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), ds.unfilter_ref(raw, h, w))       # a valid file all the same
    with pytest.raises(pngdec.UnsupportedPng):
        pngdec.decode_batch([f], cuda)
    p = tmp_path / "split_header.png"
    p.write_bytes(f)
    with pytest.raises(pngdec.UnsupportedPng):
        pngdec.decode_files([str(p)], cuda)
