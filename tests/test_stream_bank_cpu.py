"""No GPU: the row tables of `tenco_stream.StreamBank` by hand, the argument contract of `mt4_tcn_stream_conv_rows_f32` and
`mt4_tcn_stream_advance_rows` (every refusal precedes a launch) and the --online_streams refusals (before any model is built)."""
import pytest

from computervision_codes_amd import drivers


def test_row_table_by_hand():
    from computervision_codes_amd.tenco_stream import row_table
    assert row_table({2: 1, 0: 5}, 4) == ([0, 0, 0, 0, 0, 2], [0, 1, 2, 3, 4, 0], [0, 2], [5, 1])
    assert row_table({3: 1}, 4) == ([3], [0], [3], [1])
    # exactly one block of 32 rows: 20 + 12
    rs, ri, ps, pc = row_table({1: 12, 0: 20}, 2)
    assert rs == [0] * 20 + [1] * 12 and ri == list(range(20)) + list(range(12)) and (ps, pc) == ([0, 1], [20, 12]) and len(rs) == 32
    # 33 rows: the second block holds one row, the second stream's last frame
    rs, ri, ps, pc = row_table({5: 32, 7: 1}, 8)
    assert rs == [5] * 32 + [7] and ri == list(range(32)) + [0] and (ps, pc) == ([5, 7], [32, 1])
    rs, ri, ps, pc = row_table({0: 1, 1: 32}, 2)
    assert len(rs) == 33 and rs[32] == 1 and ri[32] == 31 and ri[1] == 0
    # a full bank
    rs, ri, ps, pc = row_table({s: 32 for s in range(64)}, 64)
    assert len(rs) == 2048 and rs[::32] == list(range(64)) and ri[-32:] == list(range(32)) and pc == [32] * 64


@pytest.mark.parametrize("counts, capacity, word", [({}, 4, "no stream"), ({4: 1}, 4, "slot 4"), ({-1: 1}, 4, "slot -1"), ({0: 0}, 4, "0 frames"),
                                                    ({0: 33}, 4, "33 frames"), ({1: 2, 0: -1}, 4, "-1 frames"), ({0: 1.0}, 4, "1.0")])
def test_row_table_refusals(counts, capacity, word):
    from computervision_codes_amd.tenco_stream import row_table
    with pytest.raises(ValueError) as e:
        row_table(counts, capacity)
    assert word in str(e.value), str(e.value)


def test_rows_entry_points_refuse_bad_arguments_before_any_launch():
    """The pointers are never dereferenced on the host and no launch is reached, so made-up aligned addresses serve (as in test_causal_cpu.py)."""
    from computervision_codes_amd._lib import lib
    x, r, y, w, b, rs, ri, nr, ct = (0x10000 * (i + 1) for i in range(9))

    def call(x=x, lin=64, res=r, lres=64, y=y, lout=64, w=w, bias=b, cin=64, cout=64, taps=3, d=4, relu=1, n_slots=4, max_rows=40, rs=rs, ri=ri,
             nr=nr, ct=ct):
        return lib.mt4_tcn_stream_conv_rows_f32(x, lin, res, lres, y, lout, w, bias, cin, cout, taps, d, relu, n_slots, max_rows, rs, ri, nr, ct, None)

    for name in ("x", "y", "w", "rs", "ri", "nr", "ct"):
        assert call(**{name: None}) == -1, name
    assert call(n_slots=0) == -1 and call(n_slots=65, max_rows=1) == -1
    assert call(max_rows=0) == -1 and call(max_rows=32 * 4 + 1) == -1 and call(n_slots=1, max_rows=33) == -1
    assert call(taps=2) == -1 and call(d=0) == -1 and call(relu=2) == -1
    assert call(lin=48) == -1 and call(lout=48) == -1 and call(lres=48) == -1          # not powers of two
    assert call(lin=32, d=1) == -1                                                     # 2 d + 32 = 34 > 32
    assert call(lin=64, d=17) == -1 and call(lin=128, d=64) == -1                      # a full chunk per stream: 2 d + 32 rows, whatever max_rows
    assert call(lin=0) == -1                                                           # three taps need a ring
    assert call(lout=16) == -1 and call(lres=16) == -1                                 # a ring shorter than one stream's chunk
    assert call(cin=48) == -4 and call(cout=66) == -4                                  # geometry: MT4_EUNSUPPORTED
    assert call(x=x + 4) == -2 and call(y=y + 8) == -2 and call(bias=b + 4) == -2 and call(ct=ct + 4) == -2 and call(rs=rs + 2) == -2   # MT4_EALIGN

    def adv(ct=ct, n_slots=4, ps=rs, pc=ri, np_=nr):
        return lib.mt4_tcn_stream_advance_rows(ct, n_slots, ps, pc, np_, None)

    for name in ("ct", "ps", "pc", "np_"):
        assert adv(**{name: None}) == -1, name
    assert adv(n_slots=0) == -1 and adv(n_slots=65) == -1
    assert adv(ct=ct + 4) == -2 and adv(ps=rs + 2) == -2 and adv(np_=nr + 1) == -2
    assert lib.mt4_abi_version() == 10                                                 # additions only


@pytest.mark.parametrize("argv, words", [
    (["--online", "--causal", "--temporal_ckpt", "/nonexistent/t.pth", "--online_streams", "0"], ("--online_streams", "0")),
    (["--online", "--causal", "--temporal_ckpt", "/nonexistent/t.pth", "--online_streams", "65"], ("--online_streams", "65")),
    (["--causal", "--temporal_ckpt", "/nonexistent/t.pth", "--online_streams", "2"], ("--online_streams", "--online")),
    (["--online_streams", "2"], ("--online_streams", "--online")),
])
def test_online_streams_refusals_name_the_flag_before_any_model(argv, words):
    with pytest.raises(ValueError) as e:
        drivers.predict(argv + ["--student_ckpt", "/nonexistent/s.pth", "--frames_dir", "/nonexistent"])
    assert all(w in str(e.value) for w in words), str(e.value)


def test_online_streams_default_and_in_range_values_pass_the_flag_checks():
    assert drivers._predict_parser().parse_known_args([])[0].online_streams == 1
    for extra in ([], ["--online_streams", "1"], ["--online", "--causal", "--temporal_ckpt", "/nonexistent/t.pth", "--online_streams", "64"]):
        with pytest.raises(FileNotFoundError):          # the next check after the flags: the checkpoint file
            drivers.predict(extra + ["--student_ckpt", "/nonexistent/s.pth", "--frames_dir", "/nonexistent"])
