"""No GPU: the --causal / --online flags and their refusals (before any model is built), the argument contract of `mt4_tcn_stream_conv_f32`
(every refusal precedes a launch) and the host restatement of the ring indexing."""

import pytest

from computervision_codes_amd import drivers


def test_causal_flag_is_declared_in_all_three_parsers_and_defaults_off():
    for p in (drivers._parser("tenco", True), drivers._parser("tenco", False), drivers._predict_parser()):
        assert p.parse_known_args([])[0].causal is False
        assert p.parse_known_args(["--causal"])[0].causal is True
    F = drivers._predict_parser().parse_known_args([])[0]
    assert F.online is False and F.online_chunk == 1
    assert not hasattr(drivers._parser("spatial_cnn", True).parse_known_args([])[0], "causal")


def test_causal_with_hier_is_refused_before_any_model(capsys):
    for run in (lambda: drivers.tenco_eval(["-t", "--causal", "--hier", "True", "--fpn", "--data_dir", "/nonexistent"]),
                lambda: drivers.tenco_eval(["-e", "--causal", "--hier", "True", "--fpn", "--data_dir", "/nonexistent"]),
                lambda: drivers.predict(["--causal", "--hier", "True", "--student_ckpt", "/nonexistent/s.pth", "--frames_dir", "/nonexistent"])):
        with pytest.raises(ValueError) as e:
            run()
        msg = str(e.value)
        assert "--causal" in msg and "--hier" in msg and "AvgPool1d(7, 3)" in msg and "linear" in msg and "nearest" in msg


@pytest.mark.parametrize("argv, words", [
    (["--online", "--temporal_ckpt", "/nonexistent/t.pth"], ("--online", "--causal")),
    (["--online", "--causal"], ("--online", "--temporal_ckpt")),
    (["--online", "--causal", "--temporal_ckpt", "/nonexistent/t.pth", "--online_chunk", "0"], ("--online_chunk", "0")),
    (["--online", "--causal", "--temporal_ckpt", "/nonexistent/t.pth", "--online_chunk", "33"], ("--online_chunk", "33")),
    (["--online", "--causal", "--temporal_ckpt", "/nonexistent/t.pth", "--dtype", "bf16"], ("--online", "bf16")),
])
def test_online_refusals_name_the_flag_before_any_model(argv, words):
    with pytest.raises(ValueError) as e:
        drivers.predict(argv + ["--student_ckpt", "/nonexistent/s.pth", "--frames_dir", "/nonexistent"])
    assert all(w in str(e.value) for w in words), str(e.value)


def test_causal_says_one_line_and_the_default_says_nothing(capsys):
    with pytest.raises(FileNotFoundError):          # the next check after the flags: the checkpoint file
        drivers.predict(["--causal", "--student_ckpt", "/nonexistent/s.pth", "--frames_dir", "/nonexistent"])
    out = capsys.readouterr().out
    assert out.count("--causal") == 1 and len(out.strip().splitlines()) == 1
    with pytest.raises(FileNotFoundError):
        drivers.predict(["--student_ckpt", "/nonexistent/s.pth", "--frames_dir", "/nonexistent"])
    assert capsys.readouterr().out == ""


def test_stream_conv_refuses_bad_arguments_before_any_launch():
    """NULL, n = 0, n = 33, a ring shorter than 2 d + n, a ring length that is no power of two: MT4_EINVAL (-1).  The pointers are never
    dereferenced on the host and no launch is reached, so made-up aligned addresses serve."""
    from computervision_codes_amd._lib import lib
    x, r, y, w, b, t0 = (0x10000 * (i + 1) for i in range(6))

    def call(x=x, lin=64, res=r, lres=64, y=y, lout=64, w=w, bias=b, cin=64, cout=64, taps=3, d=4, relu=1, n=5, t0=t0):
        return lib.mt4_tcn_stream_conv_f32(x, lin, res, lres, y, lout, w, bias, cin, cout, taps, d, relu, n, t0, None)

    assert call(x=None) == -1 and call(y=None) == -1 and call(w=None) == -1 and call(t0=None) == -1
    assert call(n=0) == -1 and call(n=33) == -1 and call(n=-1) == -1
    assert call(lin=32, d=16, n=1) == -1             # 2 d + n = 33 > 32
    assert call(lin=8, d=4, n=1) == -1               # 9 > 8
    assert call(lin=48) == -1 and call(lout=24) == -1 and call(lres=3) == -1      # not powers of two
    assert call(lin=0) == -1                         # three taps need a ring
    assert call(taps=2) == -1 and call(d=0) == -1 and call(lout=4, n=5) == -1
    assert call(cin=40) == -4 and call(cout=66) == -4                                # geometry: MT4_EUNSUPPORTED
    assert call(x=x + 4) == -2 and call(t0=t0 + 4) == -2                             # MT4_EALIGN
    assert lib.mt4_tcn_stream_advance(None, 1, None) == -1 and lib.mt4_tcn_stream_advance(t0, 33, None) == -1


def test_tap_rows_by_hand():
    from computervision_codes_amd.tenco_stream import ring_rows, tap_rows
    assert [ring_rows(d) for d in (1, 4, 16, 32, 1024)] == [64, 64, 64, 128, 4096] and ring_rows(1, taps=1) == 32
    # t0 = 0, d = 2, three frames: taps at f - 4, f - 2, f; every negative frame is padding
    reads, writes = tap_rows(0, 3, 2, 64)
    assert reads == [[-1, -1, 0], [-1, -1, 1], [-1, 0, 2]] and writes == [0, 1, 2]
    # a write that wraps inside the chunk: L = 64, frames 62 .. 65 land in rows 62, 63, 0, 1; d = 4 reads frames f - 8, f - 4, f
    reads, writes = tap_rows(62, 4, 4, 64)
    assert writes == [62, 63, 0, 1]
    assert reads == [[54, 58, 62], [55, 59, 63], [56, 60, 0], [57, 61, 1]]
    # d < n: later rows of the chunk read rows the SAME chunk wrote (frames 10, 11 feed frames 11, 12 at d = 1)
    reads, writes = tap_rows(10, 5, 1, 64)
    assert writes == [10, 11, 12, 13, 14] and reads[2] == [10, 11, 12] and reads[4] == [12, 13, 14] and reads[0] == [8, 9, 10]
    # far beyond the ring length (three wraps and 7): only the low bits count
    assert tap_rows(3 * 64 + 7, 1, 16, 64) == ([[(199 - 32) % 64, (199 - 16) % 64, 199 % 64]], [199 % 64])
    # one tap: the row itself
    assert tap_rows(5, 2, 1, 32, taps=1) == ([[5], [6]], [5, 6])
    with pytest.raises(AssertionError):
        tap_rows(0, 5, 16, 32)                       # 2 d + n = 37 > 32
