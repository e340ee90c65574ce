"""CPU: token log-probabilities (teal_amd/csrc/teal_logprob.hip and what the engines, the batcher, generate.py and score.py build on
it) — what needs no GPU.

  * the new unit is built, its two entry points are declared and exported, and its kernels neither spill nor use scratch;
  * every argument check of the two entry points answers before any HIP call, so the error codes come back without a device;
  * ContinuousBatcher against a fake engine that offers set_logprobs / read_logprobs: "logprobs" / "top_logprobs" aligned with
    "tokens" per request across refills; with logprobs=None an engine without those methods runs unchanged;
  * generate.py --logprobs' refusals; score.py's parsing, windowing and perplexity arithmetic; the fp64 rule itself.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import logprob_rule as R
from teal_amd import _lib
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast import score as S
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
from test_continuous_host import REQS, FakeEngine, _args, _draw, _expected, _resources

NEW = ("teal_token_logprobs", "teal_score_step")
OK, ARG, DTYPE, SHAPE, ALIGN = 0, -1, -2, -3, -4


def test_logprob_unit_is_built_declared_and_exported():
    assert "teal_logprob.hip" in _lib.SOURCES
    hdr = open(os.path.join(_lib.INCLUDE, "teal_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\(", hdr), name
    assert "temperature 1" in hdr[hdr.index("teal_amd/csrc/teal_logprob.hip"):hdr.index("int teal_token_logprobs(")]
    src = open(os.path.join(_lib.CSRC, "teal_logprob.hip")).read()
    assert "temperature 1" in src[:src.index("#include")] and "__expf" not in src and "__logf" not in src and "asm" not in src


def test_logprob_kernels_do_not_spill_to_scratch(tmp_path):
    res = _resources(tmp_path, "teal_logprob.hip")
    assert len(res) == 4, sorted(res)  # {token_logprobs, score_step} x {fp16, bf16}
    assert all(v == (0, 0) for v in res.values()), res


# ---- error codes, no device ------------------------------------------------------------------------------------------------
class _Mem:
    """host memory at a 16-byte aligned address (never dereferenced: every call below is refused before any HIP call)"""

    def __init__(self, nbytes=4096):
        self.buf = ctypes.create_string_buffer(nbytes + 16)
        self.ptr = (ctypes.addressof(self.buf) + 15) & ~15


def _token_args(**kw):
    m = _Mem()
    a = dict(logits=m.ptr, stride=40, vocab=32, dtype=0, B=2, tokens=m.ptr + 1024, rng=m.ptr + 1040, lp=m.ptr + 1104, lp_len=4,
             top_n=2, top_ids=m.ptr + 1200, top_lp=m.ptr + 1300, active=None, slot0=0, stream=None)
    a.update(kw)
    return m, tuple(a.values())


def _score_args(**kw):
    m = _Mem()
    a = dict(logits=m.ptr, vocab=32, dtype=0, targets=m.ptr + 1024, n=5, token_out=m.ptr + 1100, pos=m.ptr + 1104, lp=m.ptr + 1200,
             stream=None)
    a.update(kw)
    return m, tuple(a.values())


@pytest.mark.parametrize("kw,want", [
    (dict(vocab=12), SHAPE), (dict(vocab=0), SHAPE), (dict(vocab=131072 + 8), SHAPE), (dict(top_n=9), ARG), (dict(top_n=-1), ARG),
    (dict(logits=None), ARG), (dict(tokens=None), ARG), (dict(rng=None), ARG), (dict(lp=None), ARG), (dict(top_ids=None), ARG),
    (dict(top_lp=None), ARG), (dict(B=0), ARG), (dict(B=9), ARG), (dict(slot0=31), ARG), (dict(slot0=-1), ARG), (dict(lp_len=0), ARG),
    (dict(dtype=2), DTYPE), (dict(stride=36), ALIGN),
])
def test_token_logprobs_error_codes_without_a_device(kw, want):
    L = _lib.load()
    keep, args = _token_args(**kw)
    assert L.teal_token_logprobs(*args) == want
    del keep


def test_odd_row_addresses_are_refused():
    L = _lib.load()
    keep, args = _token_args()
    assert L.teal_token_logprobs(args[0] + 2, *args[1:]) == ALIGN
    keep2, sargs = _score_args()
    assert L.teal_score_step(sargs[0] + 2, *sargs[1:]) == ALIGN
    del keep, keep2


@pytest.mark.parametrize("kw,want", [
    (dict(vocab=12), SHAPE), (dict(vocab=4), SHAPE), (dict(logits=None), ARG), (dict(targets=None), ARG), (dict(token_out=None), ARG),
    (dict(pos=None), ARG), (dict(lp=None), ARG), (dict(n=0), ARG), (dict(dtype=7), DTYPE),
])
def test_score_step_error_codes_without_a_device(kw, want):
    L = _lib.load()
    keep, args = _score_args(**kw)
    assert L.teal_score_step(*args) == want
    del keep


# ---- the batcher against a fake engine -----------------------------------------------------------------------------------------
def _lp_of(seed, i):
    return -(_draw(seed, i) + 1) / 64.0


class FakeLogprobEngine(FakeEngine):
    """FakeEngine whose slots also keep, per produced token, a logprob and `top_n` alternates that are functions of (stream, draw)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.top_n, self.set_calls = None, 0

    def set_logprobs(self, n):
        self.top_n, self.set_calls = n, self.set_calls + 1

    def read_logprobs(self, slot, n):
        assert self.top_n is not None, "read_logprobs before set_logprobs"
        seed = self.seed[slot]
        lp = [_lp_of(seed, i) for i in range(n)]
        ids = [[(_draw(seed, i) + j) % 50 for j in range(self.top_n)] for i in range(n)]
        tlp = [[_lp_of(seed, i) - j for j in range(self.top_n)] for i in range(n)]
        return lp, ids, tlp


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("n", [0, 3])
def test_batcher_logprobs_align_with_tokens_across_refills(K, n):
    eng = FakeLogprobEngine()
    b = ContinuousBatcher(eng, sync_every=K, logprobs=n)
    res = b.run(REQS)
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(REQS)]
    assert len(set(s for s, _, _ in eng.log)) == 4 and len(eng.log) == len(REQS)  # 10 requests through 4 slots: refills
    for r, toks in enumerate(res["tokens"]):
        assert res["logprobs"][r] == [_lp_of(1234 + r, i) for i in range(len(toks))]
        assert all(isinstance(v, float) for v in res["logprobs"][r])
    if n:
        for r, toks in enumerate(res["tokens"]):
            assert len(res["top_logprobs"][r]) == len(toks)
            for i, alts in enumerate(res["top_logprobs"][r]):
                assert alts == [((toks[i] + j) % 50, _lp_of(1234 + r, i) - j) for j in range(n)]
    else:
        assert "top_logprobs" not in res
    b.run(REQS)
    assert eng.set_calls == 1  # once per batcher: the call drops the engine's captured step


def test_batcher_without_logprobs_touches_neither_method():
    eng = FakeEngine()  # offers neither set_logprobs nor read_logprobs
    assert not hasattr(eng, "set_logprobs") and not hasattr(eng, "read_logprobs")
    res = ContinuousBatcher(eng, sync_every=3).run(REQS)
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(REQS)]
    assert "logprobs" not in res and "top_logprobs" not in res
    for bad in (9, -1, 1.5, True):
        with pytest.raises(ValueError, match="0..8"):
            ContinuousBatcher(FakeLogprobEngine(), logprobs=bad)


# ---- generate.py --logprobs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,msg", [
    (("--synthetic", "tiny-test", "--compile", "--logprobs", "9"), "0..8"),
    (("--synthetic", "tiny-test", "--compile", "--logprobs", "-1"), "0..8"),
    (("--synthetic", "tiny-test", "--logprobs", "0"), "fused engine"),                            # the module path
    (("--synthetic", "tiny-test", "--compile", "--no_engine", "--logprobs", "0"), "fused engine"),
    (("--synthetic", "tiny-test", "--compile", "--dense", "--logprobs", "0"), "thresholds"),
    (("--synthetic", "tiny-test", "--compile", "--self_speculate", "--logprobs", "2"), "speculative"),
    (("--checkpoint_path", "ck/Llama-2-7b/model.pth", "--compile", "--logprobs", "2"), "thresholds"),
])
def test_check_logprobs_args_refusals(extra, msg):
    with pytest.raises(SystemExit, match=msg):
        G.check_logprobs_args(_args(*extra))


def test_check_logprobs_args_refuses_tensor_parallel(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="tensor parallelism"):
        G.check_logprobs_args(_args("--synthetic", "tiny-test", "--compile", "--logprobs", "0"))


def test_check_logprobs_args_accepts_the_engine_paths(tmp_path):
    assert _args().logprobs is None and G.check_logprobs_args(_args("--synthetic", "tiny-test")) is None
    assert G.check_logprobs_args(_args("--synthetic", "tiny-test", "--compile", "--logprobs", "0")) == 0
    assert G.check_logprobs_args(_args("--synthetic", "tiny-test", "--engine", "--logprobs", "8")) == 8
    assert G.check_logprobs_args(_args("--synthetic", "tiny-test", "--compile", "--batch_size", "4", "--logprobs", "5")) == 5
    assert G.check_logprobs_args(_args("--synthetic", "tiny-test", "--requests", str(tmp_path / "r.jsonl"), "--logprobs", "1")) == 1


def test_engines_refuse_bad_settings_before_touching_a_device():
    from teal_amd.gpt_fast.logprobs import check_setting
    assert check_setting(None) is None and check_setting(0) == 0 and check_setting(8) == 8
    for bad in (9, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="0..8"):
            check_setting(bad)


# ---- score.py ------------------------------------------------------------------------------------------------------------------
def test_score_windowing():
    seqs = [list(range(10)), [7], [1, 2], list(range(5))]
    assert S.cut_windows(seqs, 4) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9], [1, 2], [0, 1, 2, 3]]  # [7] and the tail [4] score nothing
    assert S.cut_windows(seqs, 100) == [list(range(10)), [1, 2], list(range(5))]
    assert S.cut_windows([list(range(9))], 3) == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    with pytest.raises(ValueError, match="at least 2"):
        S.cut_windows(seqs, 1)


def test_score_perplexity_arithmetic():
    lps = [[math.log(0.5), math.log(0.25)], [math.log(0.125)]]
    assert S.perplexity(lps) == pytest.approx(math.exp(-(math.log(0.5) + math.log(0.25) + math.log(0.125)) / 3), rel=1e-12)
    assert S.perplexity(lps) == pytest.approx(4.0, rel=1e-12)  # (2 * 4 * 8)^(1/3)
    assert S.perplexity([[-math.log(512.0)] * 7]) == pytest.approx(512.0, rel=1e-12)  # the uniform model
    assert S.perplexity([[0.0, 0.0]]) == 1.0
    with pytest.raises(ValueError, match="nothing was scored"):
        S.perplexity([[], []])
    assert S.dense_thresholds([{"q": 0.3, "down": 0.1}]) == [{"q": -1.0, "down": -1.0}]


def test_score_parse_sequences():
    assert S.parse_sequences(['{"tokens": [1, 2, 3]}', "", '{"tokens": [4]}']) == [[1, 2, 3], [4]]

    class Tok:
        def bos_id(self):
            return 1

        def encode(self, s):
            return [ord(c) for c in s]
    assert S.parse_sequences(['{"text": "hi"}'], Tok()) == [[1, ord("h"), ord("i")]]
    for bad, msg in [('{"text": "hi"}', "tokenizer"), ('{"tokens": []}', "non-empty"), ('{"tokens": [1], "text": "x"}', "exactly one"),
                     ("not json", "not JSON"), ('{"tokens": [-1]}', "token ids"), ('{"tokens": [true]}', "token ids")]:
        with pytest.raises(ValueError, match=msg):
            S.parse_sequences([bad])
    with pytest.raises(ValueError, match="no sequences"):
        S.parse_sequences(["", " "])


def test_score_tool_refusals(tmp_path):
    f = tmp_path / "t.jsonl"
    f.write_text('{"tokens": [1, 2]}\n')
    p = S.build_parser()
    for extra, msg in [((), "exactly one"), (("--synthetic", "tiny-test", "--checkpoint_path", "x"), "exactly one"),
                       (("--checkpoint_path", "ck/Llama-2-7b/model.pth"), "hist_path"),
                       (("--synthetic", "tiny-test", "--sparsity", "1.0"), "sparsity"), (("--synthetic", "tiny-test", "--window", "1"), "window")]:
        with pytest.raises(SystemExit, match=msg):
            S.main(p.parse_args(["--tokens", str(f), *extra]))


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def test_rule_restates_the_definition():
    g = np.random.default_rng(5)
    row = (g.standard_normal(1000) * 4).astype(np.float16)
    lp = R.logprobs64(row)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-12
    assert np.allclose(lp, np.log(np.exp(row.astype(np.float64)) / np.exp(row.astype(np.float64)).sum()), atol=1e-12)
    assert np.allclose(R.logprobs64(np.zeros(64, np.float16)), -math.log(64))
    peaked = np.full(32, -60000.0, np.float16)
    peaked[7] = 60000.0
    lp = R.logprobs64(peaked)
    assert lp[7] == 0.0 and lp[0] == -120000.0
    ninf = np.array([0.0, -np.inf, 0.0, -np.inf] * 2, np.float16)
    assert np.allclose(R.logprobs64(ninf)[[0, 2]], -math.log(4)) and R.logprobs64(ninf)[1] == -np.inf
    assert R.top_n(np.array([1, 5, 5, 0, 5, 7, -1, 7], np.float16), 5).tolist() == [5, 7, 1, 2, 4]  # equal logits: the lower id first
    assert R.top_n(np.zeros(16, np.float16), 3).tolist() == [0, 1, 2]
    assert R.tol(np.array([0.0, -0.5, 1.0]))[0] == 4 * 2.0 ** -23 and R.tol(-33.0) == 4 * 2.0 ** -18
    assert R.close(np.float32(-33.0) + np.float32(1e-5), -33.0) and not R.close(-33.0 + 2e-5, -33.0)
