"""GPU: `tenco_stream.StreamBank`: four videos through a 4-slot bank on a fixed irregular schedule (videos opening at different ticks, per-tick
counts from 1 to 32 that differ between the streams, one video pausing, a slot closed and reused with NaN left in its rings) give, for every
video, the logits of a solo `TencoStream` pushed frame by frame -- to the bit, eager and replayed.  The small head of test_gpu_tcn_stream.py
(C = 64, D = 32, layers 3 / 2 / 3: every ring 64 rows, so the 150-frame video wraps each ring twice)."""
import types

import pytest
import torch

import bf16_bounds as bb
from computervision_codes_amd import shapes, synth

pytestmark = pytest.mark.gpu
CFG = dict(num_layers_PG=3, num_layers_R=2, num_R=3)
C, D = 64, 32
HEADS = ("ivt", "i", "v", "t")
LENGTHS = {"a": 150, "b": 97, "c": 40, "d": 61}
# (video, first tick, per-tick counts in turn; 0: the video pauses that tick).  "d" opens when "c" has closed, into c's slot.
PLAN = {"a": (0, [32, 1, 7, 32, 5, 16, 3]), "b": (2, [1, 9, 0, 0, 32, 4]), "c": (1, [3, 17, 1, 19]), "d": (None, [2, 32, 11])}


def _model(causal=True, hier=False, dtype=torch.float32, sd=None):
    from computervision_codes_amd.temporal_tenco import VideoNas
    args = types.SimpleNamespace(fpn=True, output=False, hier=hier)
    m = VideoNas(args, CFG["num_layers_PG"], CFG["num_layers_R"], CFG["num_R"], C, D, 100, causal=causal, dtype=dtype).eval()
    return m.load_state_dict(sd) if sd is not None else m


@pytest.fixture(scope="module")
def head(cuda):
    """the small causal head, the four feature videos and ONE solo reference run of each (one frame per push, eager)"""
    from computervision_codes_amd.tenco_stream import TencoStream
    sd = synth.fill_from_shapes(shapes.tenco_shapes(CFG["num_layers_PG"], CFG["num_layers_R"], CFG["num_R"], C, D, 100, fpn=True), seed=31)
    model = _model(sd=sd)
    feats = {v: synth.synthetic_features(n, D, seed=40 + i)[0].to(cuda).contiguous() for i, (v, n) in enumerate(LENGTHS.items())}
    solo, ref = TencoStream(model, use_graph=False), {}
    for v, x in feats.items():
        solo.reset()
        outs = [solo.push(x[t:t + 1]) for t in range(x.shape[0])]
        ref[v] = {h: torch.cat([o[h] for o in outs]).cpu() for h in HEADS}
    return dict(model=model, sd=sd, feats=feats, ref=ref)


def _run_schedule(bank, feats):
    """-> ({video: {head: logits [T, K]}}, {video: slot}); asserts the bookkeeping on the way"""
    slot, at, turn, outs = {}, {v: 0 for v in PLAN}, {v: 0 for v in PLAN}, {v: [] for v in PLAN}
    done, tick = set(), 0
    while len(done) < len(PLAN):
        assert tick < 200
        for v, (first, _) in PLAN.items():
            if v not in slot and v not in done and (first == tick or (first is None and "c" in done)):
                if v == "d":
                    for stage in bank.rings:
                        for r in stage:
                            r[slot["c"]].fill_(float("nan"))           # what the closed video left must never be read
                slot[v] = bank.open()
                assert bank.frames_seen(slot[v]) == 0
        push = {}
        for v in slot:
            if v in done:
                continue
            seq = PLAN[v][1]
            n = min(seq[turn[v] % len(seq)], LENGTHS[v] - at[v])
            turn[v] += 1
            if n:
                push[slot[v]] = (v, n)
        before = bank.counters.cpu().tolist()
        if push:
            res = bank.push({s: feats[v][at[v]:at[v] + n] for s, (v, n) in push.items()})
            assert sorted(res) == sorted(push)
        after = bank.counters.cpu().tolist()
        for s in range(bank.capacity):
            assert after[s] - before[s] == (push[s][1] if s in push else 0), (tick, s)     # a slot that is open but absent is untouched
        for s, (v, n) in push.items():
            assert res[s]["ivt"].shape == (n, 100) and res[s]["t"].shape == (n, 15)
            outs[v].append(res[s])
            at[v] += n
            assert bank.frames_seen(s) == at[v]
            if at[v] == LENGTHS[v]:
                bank.close(s)
                done.add(v)
        tick += 1
    assert slot["d"] == slot["c"] and len(set(slot[v] for v in "abc")) == 3
    return {v: {h: torch.cat([o[h] for o in outs[v]]).cpu() for h in HEADS} for v in PLAN}, slot


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_every_video_equals_its_solo_stream_to_the_bit(head, use_graph):
    from computervision_codes_amd.tenco_stream import StreamBank, TencoStream
    bank = StreamBank(head["model"], 4, use_graph=use_graph)
    assert all(r.shape == (4, 64, C) for stage in bank.rings for r in stage)
    assert bank.ring_bytes() == 4 * TencoStream(head["model"]).ring_bytes()
    got, _ = _run_schedule(bank, head["feats"])
    for v in PLAN:
        for h in HEADS:
            bb.check_exact(got[v][h], head["ref"][v][h], what=f"bank graph {use_graph}: video {v} head {h}")
    if use_graph:
        assert sorted(bank._graphs) == [32, 64, 96]          # one graph per number of 32-row blocks, whatever the per-stream counts


def test_absent_slots_keep_their_rings(head):
    from computervision_codes_amd.tenco_stream import StreamBank
    bank = StreamBank(head["model"], 4)
    a, b = bank.open(), bank.open()
    x = head["feats"]["a"]
    bank.push({a: x[:9], b: x[9:12]})
    keep = [[r[b].clone() for r in stage] for stage in bank.rings]
    bank.push({a: x[9:41]})
    bank.push({a: x[41:42]})
    for stage, kstage in zip(bank.rings, keep):
        for r, k in zip(stage, kstage):
            assert torch.equal(r[b], k) and not bool(r[2:].any())            # nor was a slot that was never opened written
    assert bank.frames_seen(a) == 42 and bank.frames_seen(b) == 3 and bank.counters.tolist() == [42, 3, 0, 0]


def test_bank_refusals_say_why(head):
    from computervision_codes_amd.tenco_stream import StreamBank
    bank = StreamBank(head["model"], 2)
    x = head["feats"]["a"]
    with pytest.raises(ValueError, match="not open"):
        bank.push({0: x[:1]})
    s0, s1 = bank.open(), bank.open()
    assert (s0, s1) == (0, 1)
    with pytest.raises(RuntimeError, match="all 2 slots"):
        bank.open()
    with pytest.raises(ValueError, match="1..32"):
        bank.push({0: x[:33]})
    with pytest.raises(ValueError, match="no stream"):
        bank.push({})
    bank.close(0)
    with pytest.raises(ValueError, match="not open"):
        bank.push({0: x[:1], 1: x[:1]})
    with pytest.raises(ValueError, match="not open"):
        bank.frames_seen(0)
    assert bank.frames_seen(1) == 0 and bank.counters.tolist() == [0, 0]     # a refused push moves nothing
    assert bank.open() == 0
    for cap in (0, 65):
        with pytest.raises(ValueError, match="capacity"):
            StreamBank(head["model"], cap)
    with pytest.raises(ValueError, match="causal"):
        StreamBank(_model(causal=False, sd=head["sd"]), 2)
    with pytest.raises(ValueError, match="fp32"):
        StreamBank(_model(dtype=torch.bfloat16, sd=head["sd"]), 2)
    with pytest.raises(ValueError, match="--hier"):
        hier = types.SimpleNamespace(causal=True, hier=True, dtype=torch.float32, use_fpn=True)      # (VideoNas itself refuses causal with --hier)
        StreamBank(hier, 2)
