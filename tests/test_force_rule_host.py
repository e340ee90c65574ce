"""Host-side checks of teacher-forced requests: the request fields and every refusal that comes before anything is loaded, the
batcher's Forced feature against the recording engine of tests/batcher_trace.py (taught the device rule of tests/force_rule.py),
the sampler mixin's launch order against the host harness of tests/test_engine_features_host.py, and the engines without an
admission, which refuse the setter."""
import json

import numpy as np
import pytest
import torch

import force_rule as R
from batcher_trace import VOCAB, RecordingEngine, _draw
from teal_amd.gpt_fast import continuous as C
from teal_amd.gpt_fast import forcing as FT
from teal_amd.gpt_fast.batched import BatchedDecodeEngine, SlotDecodeEngine
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
from teal_amd.gpt_fast.engine import DecodeEngine
from test_engine_features_host import ADDR, DRAW_SHAPES, ST, _DrawHost, _Rec, no_library  # noqa: F401  (no_library: a fixture)


# ---- the host rule itself ------------------------------------------------------------------------------------------------------
def test_the_rule_in_numpy():
    forced = [[10, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33]]
    rng = np.array([[7, 1], [7, 3], [7, 5]], dtype=np.uint64)
    tok, hist = R.force_tokens(forced, [4, 2, 9], rng, [1, 2, 3], [[0] * 3] * 3)
    # row 0: i = 0 < 4; row 1: i = 2 is not below its length 2; row 2: length 9 is clamped to the stride 4 and i = 4 is not below it
    assert tok.tolist() == [10, 2, 3] and hist.tolist() == [[10, 0, 0], [0, 0, 0], [0, 0, 0]]
    tok, hist = R.force_tokens(forced, [4, 4, 4], np.array([[7, 4], [7, 0], [7, 2]], dtype=np.uint64), [1, 2, 3], [[0] * 3] * 3,
                               active=0b101 << 5, slot0=5)
    assert tok.tolist() == [13, 2, 31] and hist.tolist() == [[0, 0, 0], [0, 0, 0], [0, 31, 0]]  # i = 3 is past the history; c = 0
    tok, hist = R.force_tokens(forced, [4, 4, 4], rng, [1, 2, 3], None, active=0b010)
    assert tok.tolist() == [1, 22, 3] and hist is None
    assert R.expected_result(None, [1, 2], [-1.0, -2.0], [1, 2]) == (None, None, None)
    assert R.expected_result([5, 6, 7], [5, 6], [-0.5, -0.25], [5, 9]) == (2, -0.75, False)
    assert R.expected_result([5, 6], [5, 6, 8], [-0.5, -0.25, -4.0], [5, 6, 1]) == (2, -0.75, True)


# ---- the fields and their refusals ----------------------------------------------------------------------------------------------
class _Tok:
    def bos_id(self):
        return 1

    def encode(self, s):
        return [3 + ord(ch) % 40 for ch in s]


def test_request_lines_carry_forced_tokens_and_get_their_budget():
    lines = ['{"tokens": [1, 2], "forced_tokens": [7, 8, 9]}', '{"tokens": [1], "forced_tokens": [4], "max_new_tokens": 6}',
             '{"tokens": [3]}', '{"prompt": "ab", "forced_text": "xyz"}', '{"tokens": [3], "forced_tokens": [5, 5], "max_new_tokens": 2}']
    reqs = C.parse_requests(lines, 11, _Tok())
    assert [r.forced_tokens for r in reqs] == [[7, 8, 9], [4], None, _Tok().encode("xyz"), [5, 5]]
    assert [r.max_new_tokens for r in reqs] == [3, 6, 11, 3, 2]  # a pure scoring request: as many draws as forced tokens
    assert reqs[3].tokens == [1] + _Tok().encode("ab")            # the prompt gets its BOS, the forced text none
    assert C.check_forced_fields(lines) is True and C.check_forced_fields(['{"tokens": [1]}', "", "not json"]) is False
    assert Request([1], 4).forced_tokens is None and Request([1], 4, forced_tokens=[2, 3]).forced_tokens == [2, 3]


REFUSED = [
    ('{"tokens": [1], "forced_tokens": []}', "\"forced_tokens\" must be a non-empty list of token ids"),
    ('{"tokens": [1], "forced_tokens": [1.5]}', "\"forced_tokens\" must be a non-empty list of token ids"),
    ('{"tokens": [1], "forced_tokens": [true]}', "\"forced_tokens\" must be a non-empty list of token ids"),
    ('{"tokens": [1], "forced_tokens": [-1]}', "\"forced_tokens\" must be a non-empty list of token ids"),
    ('{"tokens": [1], "forced_tokens": "7"}', "\"forced_tokens\" must be a non-empty list of token ids"),
    ('{"tokens": [1], "forced_text": ""}', "\"forced_text\" must be a non-empty string"),
    ('{"tokens": [1], "forced_text": 5}', "\"forced_text\" must be a non-empty string"),
    ('{"tokens": [1], "forced_tokens": [1], "forced_text": "a"}', "at most one of \"forced_tokens\" and \"forced_text\""),
    ('{"tokens": [1], "forced_tokens": [1], "constraint": "yn"}', "\"forced_tokens\" does not combine with \"constraint\""),
    ('{"tokens": [1], "forced_tokens": [1], "choices": [[1]]}', "\"forced_tokens\" does not combine with \"choices\""),
    ('{"tokens": [1], "forced_text": "a", "allowed_token_ids": [1]}', "\"forced_text\" does not combine with \"allowed_token_ids\""),
    ('{"tokens": [1], "forced_tokens": [1, 2, 3], "max_new_tokens": 2}', "\"max_new_tokens\" 2 is below the 3 forced tokens"),
]


@pytest.mark.parametrize("line,why", REFUSED)
def test_a_malformed_field_is_refused_before_anything_is_loaded(line, why):
    with pytest.raises(ValueError) as e:
        C.check_forced_fields(['{"tokens": [9]}', line])  # needs neither a model nor a tokenizer
    assert str(e.value).startswith("request line 2: ") and why in str(e.value)
    with pytest.raises(ValueError) as e:
        C.parse_requests([line], 8, _Tok(), eos_id=2, constraints={"yn": C.Automaton.from_allowed([1])})
    assert why in str(e.value)


def test_the_other_refusals():
    with pytest.raises(ValueError, match="request line 1: \"forced_text\" needs a tokenizer"):
        C.check_forced_fields(['{"tokens": [1], "forced_text": "a"}'], tokenizer_expected=False)
    with pytest.raises(ValueError, match="request line 1: \"forced_text\" needs a tokenizer"):
        C.parse_requests(['{"tokens": [1], "forced_text": "a"}'], 8)
    with pytest.raises(ValueError, match="\"max_new_tokens\" 2 is below the 3 forced tokens"):
        C.parse_requests(['{"tokens": [1], "forced_text": "abc", "max_new_tokens": 2}'], 8, _Tok())  # known once it is encoded
    for field, v in (("forced_tokens", [1]), ("forced_text", "a")):
        line = json.dumps({"id": "sys", "tokens": [1, 2], field: v})
        with pytest.raises(ValueError, match=f"prefix line 1: \"{field}\" belongs to a request line"):
            C.check_forced_fields(['{"tokens": [1]}'], [line])
        with pytest.raises(ValueError, match=f"prefix line 1: \"{field}\" belongs to a request line"):
            C.parse_prefixes([line], _Tok())
    with pytest.raises(ValueError, match="non-empty list of token ids"):
        Request([1], 4, forced_tokens=[])
    with pytest.raises(ValueError, match="non-empty list of token ids"):
        Request([1], 4, forced_tokens=[1, "2"])
    with pytest.raises(ValueError, match="3 forced_tokens exceed max_new_tokens 2"):
        Request([1], 2, forced_tokens=[1, 2, 3])
    for kw in (dict(constraint="yn"), dict(choices=[[1]]), dict(allowed_token_ids=[1])):
        with pytest.raises(ValueError, match="forced_tokens do not combine with constraint, choices or allowed_token_ids"):
            Request([1], 4, 2, forced_tokens=[1], **kw)
    assert FT.check_forced(50, None) == [] and FT.check_forced(50, (3, 49)) == [3, 49]
    for bad in ([50], [-1], [True], [1.0], "12"):
        with pytest.raises(ValueError):
            FT.check_forced(50, bad)


def test_generate_refuses_the_fields_before_it_loads_anything(tmp_path, monkeypatch):
    import types
    from teal_amd.gpt_fast import generate as G
    monkeypatch.setattr(G, "build_synthetic_model", lambda *a, **k: pytest.fail("a model was built"))
    f, p = tmp_path / "r.jsonl", tmp_path / "p.jsonl"
    args = types.SimpleNamespace(requests=f, prefixes=None, constraints=None, synthetic="tiny-test", greedy_lookup=None)
    f.write_text('{"tokens": [1]}\n{"tokens": [1], "forced_tokens": []}\n')
    with pytest.raises(SystemExit, match="--requests: request line 2: \"forced_tokens\" must be a non-empty list"):
        G.check_request_files(args)
    f.write_text('{"tokens": [1], "forced_text": "yes"}\n')
    with pytest.raises(SystemExit, match="--requests: request line 1: \"forced_text\" needs a tokenizer"):
        G.check_request_files(args)
    f.write_text('{"tokens": [1], "forced_tokens": [3], "prefix": "sys"}\n')
    p.write_text('{"id": "sys", "tokens": [1, 2], "forced_tokens": [3]}\n')
    args.prefixes = p
    with pytest.raises(SystemExit, match="--requests: prefix line 1: \"forced_tokens\" belongs to a request line"):
        G.check_request_files(args)
    p.write_text('{"id": "sys", "tokens": [1, 2]}\n')
    assert G.check_request_files(args)[0] == ['{"tokens": [1], "forced_tokens": [3], "prefix": "sys"}']


# ---- the Forced feature against the recording engine ---------------------------------------------------------------------------------
class ForcingEngine(RecordingEngine):
    """the recording engine taught the device rule: draw i of a request admitted with n forced tokens yields forced[i] for i < n"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.forced = [[] for _ in range(self.B)]
        self.feature = False

    def set_forced_tokens(self, on, capacity=None):
        self._call("set_forced_tokens", on)
        self.feature = on

    def _force(self, slot):
        i = len(self.hist[slot]) - 1
        if i < len(self.forced[slot]):
            self.hist[slot][i] = self.forced[slot][i]

    def admit(self, slot, tokens, budget, eos_id, seed, temperature, top_k, **kw):
        assert self.feature or "forced_tokens" not in kw
        self.forced[slot] = list(kw.get("forced_tokens", ()))
        self._retire = lambda *a: None  # (the first draw is forced before it is retired)
        try:
            super().admit(slot, tokens, budget, eos_id, seed, temperature, top_k, **kw)
        finally:
            del self._retire
        self._force(slot)
        self._retire(1 << slot, False)

    def run_steps(self, k, temperature, top_k, use_graph):
        self._call("run_steps", k, temperature, top_k, use_graph)
        for _ in range(k):
            self.ran = [(self.state[0] >> b) & 1 for b in range(self.B)]
            for b in range(self.B):
                if self.ran[b]:
                    self.hist[b].append(_draw(self.seed[b], len(self.hist[b])))
                    self.pos[b] += 1
                    self._force(b)
            self._retire((1 << self.B) - 1, True)

    def read_logprobs(self, slot, n):
        """the parent's, but a token is its row's top-1 only where its logprob is 0"""
        lp, ids, tlp = super().read_logprobs(slot, n)
        return lp, [[(i + (v != 0)) % VOCAB for i in row] for row, v in zip(ids, lp)], tlp


def _lp(t):  # the forcing engine's logprob and top-1 id of a token
    return -(t % 7) / 8, (t + (t % 7 != 0)) % VOCAB


def test_the_forced_feature_is_off_until_a_request_carries_tokens():
    eng = ForcingEngine(2)
    b = ContinuousBatcher(eng, sync_every=2, logprobs=0)
    res = b.run([Request([1, 2], 5), Request([3], 3)])
    assert not {"forced", "loglikelihood", "is_greedy", "top_logprobs"} & set(res) and "logprobs" in res
    calls = [c[0] for c in eng.log]
    assert "set_forced_tokens" not in calls and calls.count("set_logprobs") == 1
    assert all("forced_tokens" not in c[2] for c in eng.log if c[0] == "admit")
    assert isinstance(b.features[-1], C.Forced) and not b.features[-1].on


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("logprobs", [None, 0, 2])
def test_the_forced_feature_against_the_recording_engine(logprobs, K):
    eng = ForcingEngine(2)
    eos = 33
    given = [[4, 11, 18], None, [7, 8, eos, 9], [5], [6, 7], None]   # request 2 meets its EOS id at its third forced draw
    budgets = [3, 6, 4, 5, 2, 1]
    # tokens t with t % 7 == 0 have lp 0 and are their row's top-1 in the forcing engine: [7, 14] is greedy, [4, 11, 18] is not
    given[4] = [7, 14]
    reqs = [Request([1, 2, 3 + r], n, eos if r == 2 else None, forced_tokens=g) for r, (n, g) in enumerate(zip(budgets, given))]
    b = ContinuousBatcher(eng, sync_every=K, logprobs=logprobs)
    res = b.run(reqs)
    calls = [c for c in eng.log if c[0] in ("set_logprobs", "set_forced_tokens")]
    level = max(1, logprobs or 0)
    assert [c[:2] for c in calls] == [["set_logprobs", [logprobs]]] * (logprobs is not None) + \
        [["set_logprobs", [level]]] * (logprobs is None or logprobs < 1) + [["set_forced_tokens", [True]]]
    admits = [c for c in eng.log if c[0] == "admit"]
    assert [c[2].get("forced_tokens") for c in sorted(admits, key=lambda c: c[1][4])] == given  # only the requests that carry them
    for r, g in enumerate(given):
        toks = res["tokens"][r]
        if g is None:
            assert toks == [_draw(1234 + r, i) for i in range(budgets[r])]
            assert (res["forced"][r], res["loglikelihood"][r], res["is_greedy"][r]) == (None, None, None)
            continue
        lps, tops = zip(*[_lp(t) for t in toks])
        want = R.expected_result(g, toks, lps, tops)
        assert (res["forced"][r], res["loglikelihood"][r], res["is_greedy"][r]) == want, r
        assert toks[want[0]:] == [_draw(1234 + r, i) for i in range(want[0], len(toks))]  # behind them the stream goes on
        assert res["logprobs"][r] == list(lps) and [t[0][0] for t in res["top_logprobs"][r]] == list(tops)
    assert res["forced"] == [3, None, 3, 1, 2, None] and len(res["tokens"][2]) == 3 and len(res["tokens"][3]) == 5
    assert res["is_greedy"] == [False, None, False, False, True, None]
    again = b.run(reqs)  # what was switched on stays on: no second switch
    assert [c[0] for c in eng.log].count("set_forced_tokens") == 1 and again["loglikelihood"] == res["loglikelihood"]


def test_the_batcher_refuses_what_the_engine_would():
    eng = ForcingEngine(2)
    r = Request([1], 4, forced_tokens=[1, 2])
    r.max_new_tokens = 1  # (a dataclass: changed behind the constructor's back)
    with pytest.raises(ValueError, match="request 0: 2 forced tokens exceed its budget of 1"):
        ContinuousBatcher(eng).run([r])
    with pytest.raises(ValueError, match=f"request 1: a forced token id is outside the vocabulary 0..{VOCAB - 1}"):
        ContinuousBatcher(eng).run([Request([1], 2), Request([1], 2, forced_tokens=[VOCAB])])
    assert not [c for c in eng.log if c[0] in ("admit", "set_forced_tokens")]


# ---- the mixin: key and launch order -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(DRAW_SHAPES))
@pytest.mark.parametrize("sampling", [False, True])
@pytest.mark.parametrize("logprobs", [False, True])
def test_the_forcing_launch_sits_between_the_samplers_and_the_logprob_launch(no_library, logprobs, sampling, shape):  # noqa: F811
    rows, row0, active = DRAW_SHAPES[shape]

    def run(forced):
        log = []
        h = _DrawHost(log)
        if active is not None:
            h._active = active
        if logprobs:
            h.set_logprobs(2)
            h._lp.L = _Rec(log)
        if sampling:
            h.set_sampling_params(True)
            h._samp.L = _Rec(log)
        if forced:
            h._frc = FT.ForcedTokens(4, 6, 16, "cpu")
            h._frc.L = _Rec(log)
        if rows > 1:
            args = (h.logits, 16, rows, 0.7, 40, h.rng_state, h.tok_buf, h.pos_buf, h.history, True)
        else:
            args = (torch.zeros(16, dtype=torch.float16), 0, 1, 0.7, 40, h.rng_state[row0], h.tok_buf[row0:], h.pos_buf[row0:],
                    h.history[row0], False)
        h._draw(*args, row0=row0, st=ST)
        return h, log, args

    h0, off, _ = run(False)
    assert h0._feature_key() == ((2 if logprobs else None), False) + (("sampling",) if sampling else ())
    assert "teal_force_tokens" not in [n for n, _ in off]
    h, on, args = run(True)
    assert h._feature_key() == h0._feature_key() + ("forced",) and len(h._feature_loop_state()) == len(h0._feature_loop_state())
    names = [n for n, _ in on]
    at = names.index("teal_force_tokens")
    assert names[:at] + names[at + 1:] == [n for n, _ in off] and names.count("teal_force_tokens") == 1
    assert at == (1 if sampling else rows) and (names[at + 1:] == ["teal_token_logprobs"]) == logprobs
    f = h._frc
    _, _, _, _, _, rng, tok, _, hist, _ = args
    assert on[at][1] == (f.table[row0].data_ptr(), 6, f.lengths[row0:].data_ptr(), rng.data_ptr(), tok.data_ptr(), hist.data_ptr(), 5, rows,
                         active, row0, ST)
    assert f.table.shape == (8, 6) and f.lengths.tolist() == [0] * 8 and f.table.dtype == f.lengths.dtype == torch.int32


def test_forced_rows_and_their_guards(no_library):  # noqa: F811
    f = FT.ForcedTokens(3, 4, 16, "cpu")
    f.set_row(1, [5, 6, 7])
    assert f.lengths.tolist() == [0, 3, 0, 0, 0, 0, 0, 0] and f.table[1].tolist() == [5, 6, 7, 0] and f.read(1) == 3
    f.set_row(1, ())  # the next occupant: the length word alone says "none"
    assert f.read(1) == 0 and f.table[1].tolist() == [5, 6, 7, 0]
    for bad, why in (([1] * 5, "the table holds 4"), ([16], "outside the vocabulary"), ([True], "outside the vocabulary")):
        with pytest.raises(ValueError, match=why):
            f.set_row(0, bad)
    with pytest.raises(ValueError, match="slot 3 outside 0..2"):
        f.set_row(3, [1])
    assert f.lengths.tolist() == [0] * 8
    for cap in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="capacity"):
            FT.ForcedTokens(3, cap, 16, "cpu")
    h = _DrawHost([])
    with pytest.raises(RuntimeError) as e:
        h._forced()
    assert str(e.value) == "forced tokens are off (set_forced_tokens)"


@pytest.mark.parametrize("cls", [DecodeEngine, BatchedDecodeEngine])
def test_the_engines_without_an_admission_refuse_the_setter(cls):
    eng = object.__new__(cls)
    with pytest.raises(NotImplementedError, match=f"{cls.__name__} has no forced tokens: .* no admission"):
        eng.set_forced_tokens(True)
    eng.set_forced_tokens(False)  # off is what it is
    assert eng._frc is None
    assert SlotDecodeEngine.set_forced_tokens is not BatchedDecodeEngine.set_forced_tokens
