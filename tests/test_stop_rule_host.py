"""Host: the model of per-request stop conditions (tests/stop_rule.py) pinned before tests/test_stop_gpu.py holds
teal_batched_retire_stops to it, and the host side of the feature.

  1. the model on hand-written cases: ids, sequences, precedence, min_new_tokens, untouched slots;
  2. check_stops' refusals and pack_row's layout (against the model's own hand-written row);
  3. parse_requests reads and validates "stop_token_ids", "stop_sequences", "min_new_tokens" and "stop", each malformed shape
     refused with its line number;
  4. the batcher on a fake engine that retires by the model: the feature is switched on exactly when asked for, the keywords are
     passed only then, "finish_reason" / "stop_match" appear only then and are the model's, whatever sync_every;
  5. generate.py's refusals, before anything is loaded;
  6. the header's TEAL_STOP_* / TEAL_FINISH_* values are stopping.py's, the unit and the symbol are registered and built without
     scratch, and the entry point's argument checks need no device.
"""
import ctypes
import os
import re

import pytest

import stop_rule as R
from teal_amd import _lib
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast import stopping as S
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request, parse_requests
from test_continuous_host import FakeEngine, _args, _draw, _resources


# ---- 1. the model ------------------------------------------------------------------------------------------------------------------
def _one(n, t, hist, budget=5, eos=-1, p=10, max_seq=32, **kw):
    """one active slot with n tokens produced draws t: (active afterwards, reason, match, state, pos)"""
    st = [0] * R.SLOT_WORDS
    st[R.ACTIVE], st[R.STEP], st[R.BUDGET], st[R.PRODUCED], st[R.EOS], st[R.FINISH] = 1, 7, budget, n, eos, -1
    stops = [R.row(**kw)] + [R.row() for _ in range(7)]
    pos = [p]
    R.retire(st, [t], pos, [list(hist) + [t]], stops, 1, 1, max_seq, True)
    assert st[R.PRODUCED] == n + 1 and st[R.BUDGET] == budget - 1 and st[R.STEP] == 8
    assert (st[R.FINISH] == 7) == (st[R.ACTIVE] == 0)
    return st[R.ACTIVE], stops[0][R.REASON], stops[0][R.MATCH], st, pos


def test_model_stop_ids_and_eos():
    assert _one(3, 9, [1, 2, 3], stop_token_ids=[4, 9])[:3] == (0, R.STOP_TOKEN, 9)
    assert _one(3, 9, [1, 2, 3], stop_token_ids=[4, 8])[:3] == (1, R.RUNNING, -1)
    assert _one(3, 9, [1, 2, 3], eos=9)[:3] == (0, R.STOP_TOKEN, 9)
    row = R.row(stop_token_ids=[4, 9])
    row[R.NIDS] = 1  # the 9 sits one past the end
    st = [0] * R.SLOT_WORDS
    st[R.ACTIVE], st[R.BUDGET], st[R.EOS] = 1, 5, -1
    R.retire(st, [9], [3], [[9]], [row] + [R.row()] * 7, 1, 1, 32, False)
    assert st[R.ACTIVE] == 1 and st[R.STEP] == 0


def test_model_sequences_match_generated_tokens_only():
    assert _one(3, 7, [5, 6, 9], stop_sequences=[[6, 9, 7]])[:3] == (0, R.STOP_SEQUENCE, 0)
    assert _one(3, 7, [5, 6, 9], stop_sequences=[[6, 8, 7]])[:3] == (1, R.RUNNING, -1)
    assert _one(2, 7, [6, 9], stop_sequences=[[6, 9, 7]])[:3] == (0, R.STOP_SEQUENCE, 0)      # len == n + 1
    assert _one(1, 7, [9], stop_sequences=[[6, 9, 7]])[:3] == (1, R.RUNNING, -1)              # len == n + 2: would need the prompt
    assert _one(3, 7, [5, 6, 9], stop_sequences=[[1], [9, 7], [6, 9, 7]])[:3] == (0, R.STOP_SEQUENCE, 1)  # the lowest index
    assert _one(0, 7, [], stop_sequences=[[7]])[:3] == (0, R.STOP_SEQUENCE, 0)                # a one-token sequence stays a sequence
    for bad in (0, 9, -1):
        row = R.row(stop_sequences=[[7]])
        row[R.SEQLEN] = bad
        row[R.SEQ:R.SEQ + 8] = [7] * 8
        st = [0] * R.SLOT_WORDS
        st[R.ACTIVE], st[R.BUDGET], st[R.EOS], st[R.PRODUCED] = 1, 5, -1, 12
        R.retire(st, [7], [3], [[7] * 13], [row] + [R.row()] * 7, 1, 1, 32, False)
        assert st[R.ACTIVE] == 1, bad


def test_model_precedence_and_min_new_tokens():
    assert _one(3, 7, [5, 6, 9], stop_token_ids=[7], stop_sequences=[[9, 7]])[:3] == (0, R.STOP_TOKEN, 7)
    assert _one(3, 7, [5, 6, 9], budget=1, stop_token_ids=[7])[:3] == (0, R.STOP_TOKEN, 7)
    assert _one(3, 7, [5, 6, 9], budget=1, stop_sequences=[[7]])[:3] == (0, R.STOP_SEQUENCE, 0)
    assert _one(3, 7, [5, 6, 9], budget=1)[:3] == (0, R.LENGTH, -1)
    a, why, match, st, pos = _one(3, 7, [5, 6, 9], p=32)
    assert (a, why, match, pos) == (0, R.CACHE, -1, [31])
    assert _one(3, 7, [5, 6, 9], budget=1, p=32)[:3] == (0, R.LENGTH, -1)
    for kw in (dict(stop_token_ids=[7]), dict(stop_sequences=[[9, 7]]), dict(eos=7)):
        assert _one(3, 7, [5, 6, 9], min_new_tokens=4, **kw)[0] == 0      # n + 1 == MIN: armed
        assert _one(3, 7, [5, 6, 9], min_new_tokens=5, **kw)[:3] == (1, R.RUNNING, -1)
    assert _one(3, 7, [5, 6, 9], budget=1, min_new_tokens=9, stop_token_ids=[7])[:3] == (0, R.LENGTH, -1)  # the budget is not held back


def test_model_leaves_other_slots_alone_and_fire_cuts_a_stream():
    st = [0] * R.SLOT_WORDS
    st[R.ACTIVE] = 0b101
    for b in range(8):
        st[R.BUDGET + b], st[R.EOS + b], st[R.FINISH + b] = 3, 7, -1
    stops = [R.row(stop_token_ids=[7]) for _ in range(8)]
    before = [list(r) for r in stops]
    pos = [40] * 8
    R.retire(st, [7] * 8, pos, [[7]] * 8, stops, 4, 0b1011, 32, True)
    assert st[R.ACTIVE] == 0b100 and st[R.PRODUCED:R.PRODUCED + 8] == [1, 0, 0, 0, 0, 0, 0, 0] and pos == [31] + [40] * 7
    assert stops[1:] == before[1:] and stops[0][R.REASON] == R.STOP_TOKEN
    stream = [3, 8, 5, 8, 5, 6, 1, 2]
    assert R.fire(stream, 8) == (stream, "length", -1)
    assert R.fire(stream, 8, stop_token_ids=[5]) == (stream[:3], "stop_token", 5)
    assert R.fire(stream, 8, stop_token_ids=[8], min_new_tokens=3) == (stream[:4], "stop_token", 8)
    assert R.fire(stream, 8, stop_sequences=[[9], [8, 5, 6]]) == (stream[:6], "stop_sequence", 1)
    assert R.fire(stream, 8, eos=3) == (stream[:1], "stop_token", 3)
    assert R.fire(stream, 8, first_pos=5, max_seq=8) == (stream[:4], "cache", -1)


# ---- 2. check_stops and pack_row ---------------------------------------------------------------------------------------------------
def test_check_stops_validates_with_the_reason():
    assert S.check_stops(100) == {"stop_token_ids": [], "stop_sequences": [], "min_new_tokens": 0}
    c = S.check_stops(100, [5, 9, 5], [[7], (1, 2, 3)], 4)
    assert c == {"stop_token_ids": [5, 9], "stop_sequences": [[7], [1, 2, 3]], "min_new_tokens": 4}
    assert S.is_default(S.check_stops(100)) and not S.is_default(c) and not S.is_default(S.check_stops(100, min_new_tokens=1))
    assert len(S.check_stops(100, list(range(16)) * 2)["stop_token_ids"]) == 16  # 16 after de-duplication
    for kw, msg in [(dict(stop_token_ids=[100]), "outside the vocabulary 0..99"), (dict(stop_token_ids=[-1]), "outside the vocabulary"),
                    (dict(stop_token_ids=[1.5]), "outside the vocabulary"), (dict(stop_token_ids=[True]), "outside the vocabulary"),
                    (dict(stop_token_ids=list(range(17))), "17 stop token ids: at most 16"), (dict(stop_token_ids="5"), "list of token ids"),
                    (dict(stop_sequences=[[1]] * 9), "9 stop sequences: at most 8"), (dict(stop_sequences=[[1], []]), "stop sequence 1 is empty"),
                    (dict(stop_sequences=[list(range(9))]), "9 tokens: at most 8"), (dict(stop_sequences=[[1, 100]]), "stop sequence 0: token id 100"),
                    (dict(stop_sequences=[5]), "must be a list of token ids"), (dict(min_new_tokens=-1), "non-negative integer"),
                    (dict(min_new_tokens=1.5), "non-negative integer"), (dict(min_new_tokens=True), "non-negative integer")]:
        with pytest.raises(ValueError, match=msg):
            S.check_stops(100, **kw)


def test_pack_row_is_the_headers_layout():
    kw = dict(stop_token_ids=[5, 9, 11], stop_sequences=[[7], [1, 2, 3], list(range(20, 28))], min_new_tokens=4)
    got = S.pack_row(S.check_stops(100, **kw))
    assert got == R.row(**kw) and len(got) == 96
    assert got[:8] == [4, 3, 3, 0, -1, 0, 0, 0] and got[8:11] == [5, 9, 11] and got[24:27] == [1, 3, 8]
    assert got[32] == 7 and got[40:43] == [1, 2, 3] and got[48:56] == list(range(20, 28))
    assert S.pack_row(S.check_stops(100)) == R.row()
    assert S.REASONS == {0: None, **R.NAMES}


# ---- 3. requests -------------------------------------------------------------------------------------------------------------------
class _Tok:
    def bos_id(self):
        return 1

    def encode(self, s):
        return [ord(c) for c in s]


def test_parse_requests_reads_and_validates_the_stop_fields():
    lines = ['{"tokens": [1, 2, 3]}',
             '{"tokens": [4], "stop_token_ids": [7, 8], "stop_sequences": [[1, 2], [3]], "min_new_tokens": 2}',
             '{"tokens": [5], "stop_token_ids": [], "min_new_tokens": 0}']
    rs = parse_requests(lines, 20)
    assert (rs[0].stop_token_ids, rs[0].stop_sequences, rs[0].min_new_tokens) == (None, None, None)
    assert (rs[1].stop_token_ids, rs[1].stop_sequences, rs[1].min_new_tokens) == ([7, 8], [[1, 2], [3]], 2)
    d = {"stop_token_ids": [9], "min_new_tokens": 3}
    assert rs[0].stops() == {} and rs[0].stops(d) == d
    assert rs[1].stops(d) == {"stop_token_ids": [7, 8], "stop_sequences": [[1, 2], [3]], "min_new_tokens": 2}
    assert rs[2].stops(d) == {}  # a request's own "none" wins
    r = parse_requests(['{"prompt": "hi", "stop": ["ab", "c"], "stop_sequences": [[9]]}'], 5, _Tok())[0]
    assert r.stop_sequences == [[9], [97, 98], [99]] and r.tokens == [1, 104, 105]  # no BOS in a stop string
    for bad, msg in [('{"tokens": [1], "stop_token_ids": 5}', '"stop_token_ids" must be a list'), ('{"tokens": [1], "stop_token_ids": [-1]}', "stop_token_ids"),
                     ('{"tokens": [1], "stop_token_ids": [1.5]}', "stop_token_ids"), ('{"tokens": [1], "stop_token_ids": [true]}', "stop_token_ids"),
                     ('{"tokens": [1], "stop_token_ids": [0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16]}', "at most 16"),
                     ('{"tokens": [1], "stop_sequences": [1, 2]}', '"stop_sequences" must be a list of lists'),
                     ('{"tokens": [1], "stop_sequences": [[]]}', "stop_sequences"), ('{"tokens": [1], "stop_sequences": [[1,2,3,4,5,6,7,8,9]]}', "1..8"),
                     ('{"tokens": [1], "stop_sequences": [["a"]]}', "stop_sequences"), ('{"tokens": [1], "stop_sequences": "ab"}', "stop_sequences"),
                     ('{"tokens": [1], "stop_sequences": [[1],[1],[1],[1],[1],[1],[1],[1],[1]]}', "9 stop sequences"),
                     ('{"tokens": [1], "min_new_tokens": -1}', '"min_new_tokens" must be a non-negative integer'),
                     ('{"tokens": [1], "min_new_tokens": 1.5}', "min_new_tokens"), ('{"tokens": [1], "min_new_tokens": false}', "min_new_tokens"),
                     ('{"tokens": [1], "stop": ["x"]}', '"stop" strings need a tokenizer'), ('{"tokens": [1], "stop": "x"}', '"stop" must be a list')]:
        with pytest.raises(ValueError, match="line 2: .*" + msg):
            parse_requests(['{"tokens": [1]}', bad], 5)
    for bad, msg in [('{"tokens": [1], "stop": [""]}', "non-empty strings"), ('{"tokens": [1], "stop": ["abcdefghi"]}', "encodes to 9 tokens"),
                     ('{"tokens": [1], "stop": ["a","b","c","d","e"], "stop_sequences": [[1],[2],[3],[4]]}', "at most 8")]:
        with pytest.raises(ValueError, match="line 1: .*" + msg):
            parse_requests([bad], 5, _Tok())


# ---- 4. the batcher ----------------------------------------------------------------------------------------------------------------
class _StopEngine(FakeEngine):
    """FakeEngine that retires by the model once the feature is on, and records what the batcher tells it"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.switched, self.admitted, self.stops = [], [], None

    def set_stop_conditions(self, on):
        assert self.state[R.ACTIVE] == 0
        self.switched.append(on)
        self.stops = [R.row() for _ in range(8)] if on else None

    def _retire(self, mask, count_step):
        if self.stops is None:
            return super()._retire(mask, count_step)
        R.retire(self.state, [h[-1] if h else 0 for h in self.hist] + [0] * 8, self.pos + [0] * 8, self.hist, self.stops, self.B, mask,
                 self.max_seq, count_step)

    def admit(self, slot, tokens, budget, eos_id, seed, temperature, top_k, **kw):
        self.admitted.append((seed, kw))
        if self.stops is not None:  # every admission: the last occupant left its row
            self.stops[slot] = R.row(**kw)
        else:
            assert not kw
        super().admit(slot, tokens, budget, eos_id, seed, temperature, top_k)

    def read_finish(self, slot):
        return R.NAMES.get(self.stops[slot][R.REASON]), self.stops[slot][R.MATCH]


def _stream(r, n, seed=1234):
    return [_draw(seed + r, i) for i in range(n)]


def test_the_batcher_switches_the_feature_on_exactly_when_asked():
    plain = [Request([1, 2], 6), Request([3], 9, eos_id=_stream(1, 9)[4]), Request([4], 2, stop_token_ids=[], min_new_tokens=0)]
    eng = _StopEngine(B=2)
    res = ContinuousBatcher(eng, use_graph=False).run(plain)
    assert eng.switched == [] and all(kw == {} for _, kw in eng.admitted)  # today's calls, keyword for keyword
    assert "finish_reason" not in res and "stop_match" not in res
    res0 = ContinuousBatcher(FakeEngine(B=2), use_graph=False).run(plain)  # the engine of the existing tests, unchanged
    assert res0["tokens"] == res["tokens"] and set(res0) == set(res)
    s0 = _stream(0, 6)
    for reqs, kw in [([Request([1], 6, stop_token_ids=[s0[2]])] + plain, {}), ([Request([1], 6, stop_sequences=[s0[1:3]])] + plain, {}),
                     ([Request([1], 6, min_new_tokens=2)] + plain, {}), (plain, dict(stop_token_ids=[s0[2]])),
                     (plain, dict(min_new_tokens=3)), (plain, dict(finish_reason=True))]:
        eng = _StopEngine(B=2)
        b = ContinuousBatcher(eng, use_graph=False, **kw)
        res = b.run(reqs)
        assert eng.switched == [True]
        d = {k: v for k, v in kw.items() if k != "finish_reason"}
        assert [a[1] for a in eng.admitted] == [r.stops(d) for r in reqs]  # only the requests that ask get keywords
        assert len(res["finish_reason"]) == len(reqs) == len(res["stop_match"]) and all(res["finish_reason"])
        b.run(plain)
        assert eng.switched == [True]  # once
    for kw, msg in [(dict(stop_token_ids=[-1]), "stop_token_ids"), (dict(min_new_tokens=-2), "min_new_tokens")]:
        with pytest.raises(ValueError, match=msg):
            ContinuousBatcher(FakeEngine(), **kw)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_finish_reasons_and_tokens_are_the_models_whatever_sync_every(K):
    full = [_stream(r, 12) for r in range(7)]
    specs = [dict(stop_token_ids=[full[0][3]]), dict(stop_sequences=[[1000], full[1][4:7]]), dict(), dict(stop_token_ids=[full[3][0]]),
             dict(stop_token_ids=[full[4][1]], min_new_tokens=4), dict(stop_sequences=[full[5][0:1]]), dict()]
    reqs = [Request([1, 2, 3], 12 if r != 2 else 5, eos_id=full[6][7] if r == 6 else None, **kw) for r, kw in enumerate(specs)]
    res = ContinuousBatcher(_StopEngine(B=3), sync_every=K, use_graph=False).run(reqs)
    for r, q in enumerate(reqs):
        want = R.fire(full[r], q.max_new_tokens, eos=-1 if q.eos_id is None else q.eos_id, **specs[r])
        assert (res["tokens"][r], res["finish_reason"][r], res["stop_match"][r]) == want, r
    assert res["finish_reason"][:4] == ["stop_token", "stop_sequence", "length", "stop_token"] and res["stop_match"][1] == 1
    assert len(res["tokens"][3]) == 1 and len(res["tokens"][5]) == 1 and res["finish_reason"][6] == "stop_token"


# ---- 5. generate.py ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,msg", [
    (("--synthetic", "tiny-test", "--compile", "--stop_token_ids", "5"), "need --requests"),
    (("--synthetic", "tiny-test", "--batch_size", "4", "--compile", "--min_new_tokens", "3"), "need --requests"),
    (("--synthetic", "tiny-test", "--finish_reason"), "need --requests"),
    (("--synthetic", "tiny-test", "--requests", "r.jsonl", "--stop_token_ids", "5,x"), "--stop_token_ids must be 1..16 token ids"),
    (("--synthetic", "tiny-test", "--requests", "r.jsonl", "--stop_token_ids", "-3"), "--stop_token_ids must be"),
    (("--synthetic", "tiny-test", "--requests", "r.jsonl", "--stop_token_ids", ",".join(str(i) for i in range(17))), "--stop_token_ids must be"),
    (("--synthetic", "tiny-test", "--requests", "r.jsonl", "--min_new_tokens", "-1"), "--min_new_tokens must be >= 0"),
])
def test_check_stop_args_refusals(extra, msg):
    with pytest.raises(SystemExit, match=msg):
        G.check_stop_args(_args(*extra))
    with pytest.raises(SystemExit, match=msg):  # ... and main() raises it before anything is loaded
        G.main(_args(*extra))


def test_check_stop_args_with_requests():
    assert G.check_stop_args(_args("--synthetic", "tiny-test")) == {}
    assert G.check_stop_args(_args("--synthetic", "tiny-test", "--min_new_tokens", "0")) == {}  # spelled-out "off" needs nothing
    got = G.check_stop_args(_args("--synthetic", "tiny-test", "--requests", "r.jsonl", "--stop_token_ids", "5, 9,5", "--min_new_tokens", "2",
                                  "--finish_reason"))
    assert got == {"stop_token_ids": [5, 9, 5], "min_new_tokens": 2, "finish_reason": True}
    a = _args()
    assert a.stop_token_ids is None and a.min_new_tokens is None and a.finish_reason is False and a.eos_id is None


# ---- 6. the header, the build, the entry point's argument checks -----------------------------------------------------------------
def test_header_constants_are_the_host_modules():
    hdr = open(os.path.join(_lib.INCLUDE, "teal_hip.h")).read()
    offs = {m: int(v) for m, v in re.findall(r"#define TEAL_STOP_(\w+) (\d+)", hdr)}
    assert offs == {"MIN": S.STOP_MIN, "NIDS": S.STOP_NIDS, "NSEQ": S.STOP_NSEQ, "REASON": S.STOP_REASON, "MATCH": S.STOP_MATCH,
                    "IDS": S.STOP_IDS, "SEQLEN": S.STOP_SEQLEN, "SEQ": S.STOP_SEQ, "WORDS": S.STOP_WORDS, "MAX_IDS": S.MAX_IDS,
                    "MAX_SEQS": S.MAX_SEQS, "MAX_SEQ_LEN": S.MAX_SEQ_LEN}
    assert (S.STOP_WORDS, S.STOP_IDS, S.STOP_SEQLEN, S.STOP_SEQ) == (96, 8, 24, 32) == (R.WORDS, R.IDS, R.SEQLEN, R.SEQ)
    fin = {m: int(v) for m, v in re.findall(r"#define TEAL_FINISH_(\w+) (\d+)", hdr)}
    assert fin == {"RUNNING": S.RUNNING, "STOP_TOKEN": S.STOP_TOKEN, "STOP_SEQUENCE": S.STOP_SEQUENCE, "LENGTH": S.LENGTH, "CACHE": S.CACHE}
    assert [fin[k] for k in ("RUNNING", "STOP_TOKEN", "STOP_SEQUENCE", "LENGTH", "CACHE")] == [0, 1, 2, 3, 4]
    assert int(re.search(r"#define TEAL_SLOT_WORDS (\d+)", hdr).group(1)) == 40  # the slot state did not move
    assert re.search(r"\bteal_batched_retire_stops\(", hdr)


def test_the_unit_is_registered_and_built_without_scratch(tmp_path):
    assert "teal_stop.hip" in _lib.SOURCES and "teal_stop.hip" not in _lib.PRELOAD
    assert "teal_batched_retire_stops" in _lib.EXPORTS and "teal_batched_retire_stops" in _lib.OPTIONAL_WITH_OVERRIDE
    assert hasattr(_lib.load(), "teal_batched_retire_stops") and hasattr(_lib.load_diag(), "teal_batched_retire_stops")
    res = _resources(tmp_path, "teal_stop.hip")
    assert len(res) == 1 and all("retire_stops" in n and v == (0, 0) for n, v in res.items()), res


def _stop_args(**kw):
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    a = dict(slot_state=p, tokens=p + 256, pos=p + 320, history=p + 1024, history_stride=40, stops=p + 4096, B=3, mask=7, max_seq=32,
             count_step=1, stream=None)
    a.update(kw)
    return buf, tuple(a.values())


@pytest.mark.parametrize("kw", [dict(slot_state=None), dict(tokens=None), dict(pos=None), dict(history=None), dict(stops=None), dict(B=0),
                                dict(B=9), dict(B=-1), dict(max_seq=0), dict(history_stride=7), dict(history_stride=0)])
def test_retire_stops_error_codes_without_a_device(kw):
    keep, args = _stop_args(**kw)
    assert _lib.load().teal_batched_retire_stops(*args) == -1  # TEAL_ERR_ARG, before any HIP call
    assert keep.raw == bytes(len(keep.raw))
