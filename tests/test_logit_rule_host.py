"""CPU: per-request logit processors (teal_amd/csrc/teal_logit_adjust.hip and what the engines, the batcher and generate.py build
on it) — what needs no GPU.

  * the rule (tests/logit_rule.py) on hand-computed rows, against a scalar restatement in Python floats, and on a case where a
    contracted fused multiply-add gives other bits than the two roundings the rule asks for;
  * the new unit is built, its entry point is declared and exported, and its kernels neither spill nor use scratch;
  * every argument check of the entry point answers before any HIP call, so the error codes come back without a device;
  * parse_requests accepts and refuses the new fields; ContinuousBatcher against a fake engine: the controls reach admit for
    exactly the requests that carry them, across refills, and an engine without the keywords runs plain requests unchanged;
  * generate.py's refusals.
"""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import logit_rule as R
from teal_amd import _lib
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request, parse_requests
from teal_amd.gpt_fast.logit_processors import check_controls, is_identity
from test_continuous_host import REQS, FakeEngine, _args, _expected, _resources

OK, ARG, DTYPE, SHAPE, ALIGN = 0, -1, -2, -3, -4
PB = -2 ** 31  # bit 31 alone: a prompt token that was never generated


def _h(vals):
    return np.asarray(vals, dtype=np.float16).view(np.uint16)


def _b(vals):
    """bf16 patterns of values that bf16 holds exactly"""
    u = np.asarray(vals, dtype=np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def _out(bits, bf16):
    return R.decode(bits, bf16).tolist()


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def test_repetition_rule_on_hand_computed_rows():
    w = np.array([1, 1, PB, PB, 0, 0, PB | 2, 0], dtype=np.int32)  # generated, generated, prompt only, prompt only, untouched
    row = _h([3.0, -3.0, 3.0, -3.0, 3.0, -3.0, 0.0, -0.0])
    # theta 0.5 is exact: positive / 0.5, others * 0.5; the untouched ones pass; a zero stays a zero of its sign
    assert _out(R.adjust(row, False, w, theta=0.5), False) == [6.0, -1.5, 6.0, -1.5, 3.0, -3.0, 0.0, -0.0]
    assert R.adjust(row, False, w, theta=0.5)[7] == 0x8000
    # theta 1.3: fp16(2.6) = 2.599609375; / fl32(1.3) = 1.99970..., which rounds to 2.0 in fp16 (spacing 2^-10 below 2);
    #            -2.599609375 * fl32(1.3) = -3.379492..., between -3.37890625 and -3.380859375 (spacing 2^-9): the former is nearer
    got = R.adjust(_h([2.6, -2.6, 2.6, -2.6]), False, np.array([1, 1, PB, 0], dtype=np.int32), theta=1.3)
    assert _out(got, False) == [2.0, -3.37890625, 2.0, -2.599609375]
    # bf16, exact values: 3 / 1.5 and -3 * 1.5
    assert _out(R.adjust(_b([3.0, -3.0, 3.0]), True, np.array([PB, 5, 0], dtype=np.int32), theta=1.5), True) == [2.0, -4.5, 3.0]


def test_prompt_only_tokens_take_no_count_penalty_and_counts_scale_the_frequency_penalty():
    #                 n = 0   prompt only  n = 1   n = 3   prompt + 3
    w = np.array([0, PB, 1, 3, PB | 3, 0, 0, 0], dtype=np.int32)
    row = _h([4.0] * 8)
    got = R.adjust(row, False, w, theta=1.0, alpha_p=0.5, alpha_f=0.25)
    assert _out(got, False) == [4.0, 4.0, 4.0 - 0.25 - 0.5, 4.0 - 0.75 - 0.5, 4.0 - 0.75 - 0.5, 4.0, 4.0, 4.0]
    # all three, in order: 4 / 0.5 = 8, - 3 * 0.25, - 0.5; the prompt-only token is only divided
    got = R.adjust(row, False, w, theta=0.5, alpha_p=0.5, alpha_f=0.25)
    assert _out(got, False) == [4.0, 8.0, 8.0 - 0.25 - 0.5, 8.0 - 0.75 - 0.5, 8.0 - 0.75 - 0.5, 4.0, 4.0, 4.0]
    # negative penalties reward: the sign is the caller's
    assert _out(R.adjust(row, False, w, alpha_p=-1.0), False)[2:5] == [5.0, 5.0, 5.0]


def test_bias_comes_last_and_identity_passes_the_row():
    w = np.array([0, 2, 0, 0, 0, 0, 0, 0], dtype=np.int32)
    row, bias = _h([1.0, 1.0, -0.0, 0.0, -1.0, 2.0, 3.0, 4.0]), _h([1.5, 1.5, 0.0, 0.0, 0.0, -100.0, 0.0, 0.0])
    got = R.adjust(row, False, w, theta=2.0, alpha_f=0.125, bias_bits=bias)
    assert _out(got, False) == [2.5, 0.5 - 0.25 + 1.5, 0.0, 0.0, -1.0, -98.0, 3.0, 4.0]
    assert got[2] == 0x0000  # -0 + +0 = +0: with a bias row a -0 leaves as +0 (the sampler keys the two alike)
    for bf16, r in ((False, _h([1.0, -2.5, -0.0, 0.0, 6e-8, -6e-8, 65504.0, -65504.0])), (True, _b([1.0, -2.5, -0.0, 0.0, 2.0 ** -133, 3.0, 4.0, -4.0]))):
        some = np.array([0, 1, PB, 7, PB | 1, 0, 2, 0], dtype=np.int32)
        assert np.array_equal(R.adjust(r, bf16, some), r)  # theta 1, alphas 0, no bias: the same bits, denormals included
        assert np.array_equal(R.decode(R.adjust(r, bf16, some, bias_bits=np.zeros(8, np.uint16)), bf16), R.decode(r, bf16))


def test_clamp_at_the_largest_finite_value_and_minus_infinity():
    w = np.array([1, 1, 0, 0, 1, 0, 0, 0], dtype=np.int32)
    row = _h([60000.0, -60000.0, -np.inf, 65504.0, -np.inf, 100.0, -100.0, 0.0])
    got = R.adjust(row, False, w, theta=0.5, bias_bits=_h([0, 0, 0, 100.0, 50.0, 65504.0, -65504.0, 0]))
    #                               120000 -> MAXF;  -30000;  -inf -> -MAXF;  65604 -> MAXF;  -inf -> -MAXF;  65604 -> MAXF; -65604 -> -MAXF
    assert _out(got, False) == [65504.0, -30000.0, -65504.0, 65504.0, -65504.0, 65504.0, -65504.0, 0.0]
    assert np.isfinite(R.decode(got, False)).all()
    mx = float(R.MAXF[True])
    assert mx == float.fromhex("0x1.fep127")
    brow = np.array([0x7F7F, 0xFF7F, 0xFF80, 0x7F7F, 0xFF80, 0x3F80, 0, 0], dtype=np.uint16)  # MAXF, -MAXF, -inf, MAXF, -inf, 1.0
    got = R.adjust(brow, True, w, theta=0.5, alpha_f=3e38)
    # MAXF / 0.5 overflows fp32 to +inf, minus a finite penalty stays +inf -> MAXF;  -MAXF * 0.5 - 3e38 overflows -> -MAXF
    assert got.tolist() == [0x7F7F, 0xFF7F, 0xFF7F, 0x7F7F, 0xFF7F, 0x3F80, 0, 0]


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _scalar(x, w, theta, ap, af, b):
    """the rule for one element in Python floats: an fp64 +, -, *, / of two fp32 values rounded to fp32 is the correctly rounded
    fp32 operation (53 >= 2 * 24 + 2 bits)"""
    theta, ap, af = _f32(theta), _f32(ap), _f32(af)
    n = w & 0x7FFFFFFF
    if w != 0:
        x = _f32(x / theta) if x > 0 else _f32(x * theta)
    if n > 0:
        x = _f32(x - _f32(af * _f32(float(n))))
        x = _f32(x - ap)
    if b is not None:
        x = _f32(x + b)
    return x


@pytest.mark.parametrize("bf16", [False, True])
def test_rule_against_a_scalar_restatement(bf16):
    g = np.random.default_rng(11)
    V = 4096
    bits = g.integers(0, 1 << 16, V).astype(np.uint16)
    x = R.decode(bits, bf16)
    bits = bits[np.isfinite(x)][:2048]
    V = bits.size
    w = g.choice(np.array([0, 0, 1, 3, PB, PB | 2, 1000, 0x7FFFFFFF], dtype=np.int64), V).astype(np.int32)
    bias = R.encode((g.standard_normal(V) * 3).astype(np.float32), bf16)
    for theta, ap, af, bb in ((1.3, 0.4, 0.1, bias), (0.7, -0.3, 0.05, None), (1.0, 0.0, 0.0, None)):
        got = R.decode(R.adjust(bits, bf16, w, theta, ap, af, bb), bf16)
        xs, bs = R.decode(bits, bf16).tolist(), (R.decode(bb, bf16).tolist() if bb is not None else [None] * V)
        mx = float(R.MAXF[bf16])
        with np.errstate(over="ignore"):
            want = [min(max(_scalar(xs[i], int(w[i]) & 0xFFFFFFFF, theta, ap, af, bs[i]), -mx), mx) for i in range(V)]
            want = R.decode(R.encode(np.array(want, dtype=np.float32), bf16), bf16)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_a_contracted_fma_would_give_other_bits():
    # x = 0.5, alpha_f = fl32(0.1) = 0.100000001490116..., n = 5.  Two roundings: fl32(alpha_f * 5) = 0.5 exactly (the product
    # 0.50000000745 rounds down), and 0.5 - 0.5 = +0.  One rounding: 0.5 - 0.50000000745... = -7.45e-9.
    w = np.array([5] + [0] * 7, dtype=np.int32)
    fused = R.fused_frequency(0.5, 0.1, 5)
    assert fused == np.float32(-2.0 ** -27) and np.float32(0.5) - np.float32(0.1) * np.float32(5) == 0.0
    got = R.adjust(_h([0.5] * 8), False, w, alpha_f=0.1)
    assert got[0] == 0x0000 and R.encode(np.array([fused]), False)[0] == 0x8000  # +0 against -0 (below fp16's smallest denormal)
    got = R.adjust(_b([0.5] * 8), True, w, alpha_f=0.1)
    assert got[0] == 0x0000 and R.encode(np.array([fused]), True)[0] == 0xB200   # +0 against -2^-27


def test_counting():
    w = R.prompt_state(16, [3, 3, 9])
    assert w.tolist() == [0, 0, 0, PB, 0, 0, 0, 0, 0, PB, 0, 0, 0, 0, 0, 0]
    w = R.count(R.count(R.count(w, 3), 5), 5)
    assert w[3] == PB | 1 and w[5] == 2 and int((w != 0).sum()) == 3
    assert np.array_equal(R.count(w, 16), w) and np.array_equal(R.count(w, -1), w)  # outside the vocabulary: nothing
    top = np.array([0x7FFFFFFF, -1], dtype=np.int32)
    assert np.array_equal(R.count(R.count(top, 0), 1), top)  # the count stays at 2^31 - 1, with and without the prompt bit


# ---- the unit ------------------------------------------------------------------------------------------------------------------
def test_logit_adjust_unit_is_built_declared_and_exported():
    assert "teal_logit_adjust.hip" in _lib.SOURCES and "teal_logit_adjust" in _lib.EXPORTS
    hdr = open(os.path.join(_lib.INCLUDE, "teal_hip.h")).read()
    assert re.search(r"\bint teal_logit_adjust\(", hdr)
    sec = hdr[hdr.index("teal_amd/csrc/teal_logit_adjust.hip"):hdr.index("int teal_logit_adjust(")]
    assert "separately rounded" in sec and "-MAXF" in sec
    src = open(os.path.join(_lib.CSRC, "teal_logit_adjust.hip")).read()
    for name in ("__fmul_rn", "__fsub_rn", "__fadd_rn", "__fdiv_rn"):
        assert name in src, name
    assert "asm" not in src and "atomic" not in src.split("#include")[1] and "fmaf" not in src


def test_logit_adjust_kernels_do_not_spill_to_scratch(tmp_path):
    res = _resources(tmp_path, "teal_logit_adjust.hip")
    assert len(res) == 4, sorted(res)  # {fp16, bf16} x {bias, no bias}
    assert all(v == (0, 0) for v in res.values()), res


class _Mem:
    """host memory at a 16-byte aligned address (never dereferenced: every call below is refused before any HIP call)"""

    def __init__(self, nbytes=8192):
        self.buf = ctypes.create_string_buffer(nbytes + 16)
        self.ptr = (ctypes.addressof(self.buf) + 15) & ~15


def _adjust_args(**kw):
    m = _Mem()
    a = dict(logits=m.ptr, stride=40, vocab=32, dtype=0, B=2, tokens=m.ptr + 1024, count=1, state=m.ptr + 2048, params=m.ptr + 3072,
             bias=m.ptr + 4096, out=m.ptr + 5120, out_stride=40, active=None, slot0=0, stream=None)
    a.update(kw)
    return m, tuple(a.values())


@pytest.mark.parametrize("kw,want", [
    (dict(vocab=12), SHAPE), (dict(vocab=0), SHAPE), (dict(vocab=131072 + 8), SHAPE), (dict(vocab=-8), SHAPE),
    (dict(logits=None), ARG), (dict(tokens=None), ARG), (dict(state=None), ARG), (dict(params=None), ARG), (dict(out=None), ARG),
    (dict(B=0), ARG), (dict(B=9), ARG), (dict(slot0=31), ARG), (dict(slot0=-1), ARG), (dict(slot0=30, B=3), ARG),
    (dict(dtype=2), DTYPE), (dict(dtype=-1), DTYPE), (dict(stride=36), ALIGN), (dict(out_stride=44), ALIGN),
])
def test_logit_adjust_error_codes_without_a_device(kw, want):
    L = _lib.load()
    keep, args = _adjust_args(**kw)
    assert L.teal_logit_adjust(*args) == want
    del keep


def test_odd_row_addresses_and_aliased_outputs_are_refused():
    L = _lib.load()
    keep, args = _adjust_args()
    names = ("logits", "stride", "vocab", "dtype", "B", "tokens", "count", "state", "params", "bias", "out")
    for name in ("logits", "state", "bias", "out"):
        i = names.index(name)
        assert L.teal_logit_adjust(*args[:i], args[i] + 2 + (2 if name == "state" else 0), *args[i + 1:]) == ALIGN, name
    i = names.index("out")
    assert L.teal_logit_adjust(*args[:i], args[0], *args[i + 1:]) == ARG            # out = logits
    assert L.teal_logit_adjust(*args[:i], args[0] + 64, *args[i + 1:]) == ARG       # out inside the logits' rows
    assert L.teal_logit_adjust(*args[:i], args[0] - 80 - 48, *args[i + 1:]) == ARG  # the logits inside out's rows
    del keep


# ---- requests and the batcher --------------------------------------------------------------------------------------------------
def test_parse_requests_accepts_and_refuses_the_processor_fields():
    lines = ['{"tokens": [1, 2, 3]}',
             '{"tokens": [4], "repetition_penalty": 1.3, "presence_penalty": 0.5, "frequency_penalty": -0.25, "logit_bias": {"7": -100, "9": 2.5}}',
             '{"tokens": [5], "frequency_penalty": 1}']
    rs = parse_requests(lines, 20)
    assert rs[0].controls() == {} and rs[0].repetition_penalty is None and rs[0].logit_bias is None
    assert rs[1].controls() == {"repetition_penalty": 1.3, "presence_penalty": 0.5, "frequency_penalty": -0.25,
                                "logit_bias": {"7": -100.0, "9": 2.5}}
    assert rs[2].controls() == {"frequency_penalty": 1.0}
    # the batcher's defaults fill what a request leaves open; a request's own "off" wins over a default
    assert rs[0].controls({"repetition_penalty": 1.2}) == {"repetition_penalty": 1.2}
    assert rs[1].controls({"repetition_penalty": 1.2})["repetition_penalty"] == 1.3
    assert parse_requests(['{"tokens": [1], "repetition_penalty": 1.0}'], 5)[0].controls({"repetition_penalty": 1.2}) == {}
    for bad, msg in [('{"tokens": [1], "repetition_penalty": 0}', "line 1.*repetition_penalty"), ('{"tokens": [1], "repetition_penalty": -1.5}', "> 0"),
                     ('{"tokens": [1], "repetition_penalty": "1.2"}', "repetition_penalty"), ('{"tokens": [1], "presence_penalty": true}', "presence_penalty"),
                     ('{"tokens": [1], "frequency_penalty": NaN}', "frequency_penalty"), ('{"tokens": [1], "frequency_penalty": Infinity}', "finite"),
                     ('{"tokens": [1], "logit_bias": [1, 2]}', "logit_bias"), ('{"tokens": [1], "logit_bias": {"a": 1}}', "logit_bias"),
                     ('{"tokens": [1], "logit_bias": {"-3": 1}}', "logit_bias"), ('{"tokens": [1], "logit_bias": {"3": "x"}}', "logit_bias")]:
        with pytest.raises(ValueError, match=msg):
            parse_requests([bad], 5)
    with pytest.raises(ValueError, match="line 2"):
        parse_requests(['{"tokens": [1]}', '{"tokens": [1], "presence_penalty": null}'], 5)


def test_check_controls_validates_with_the_reason():
    assert check_controls(32) == {"repetition_penalty": 1.0, "presence_penalty": 0.0, "frequency_penalty": 0.0, "logit_bias": None}
    assert check_controls(32, 1.3, 0.5, 1, {"7": -3, 9: 2.5})["logit_bias"] == {7: -3.0, 9: 2.5}
    assert is_identity(check_controls(32)) and is_identity({}) and not is_identity(check_controls(32, logit_bias={"1": 0.0}))
    for kw, msg in [(dict(repetition_penalty=0.0), "> 0"), (dict(repetition_penalty=float("inf")), "finite"), (dict(presence_penalty=float("nan")), "finite"),
                    (dict(frequency_penalty="1"), "finite number"), (dict(logit_bias={"32": 1.0}), "outside 0..31"), (dict(logit_bias={-1: 1.0}), "outside"),
                    (dict(logit_bias={"x": 1.0}), "not a token id"), (dict(logit_bias={3: float("inf")}), "finite"), (dict(logit_bias=[3]), "map")]:
        with pytest.raises(ValueError, match=msg):
            check_controls(32, **kw)
    # the parameter row is fp32: finite and positive as doubles is not enough
    for kw, msg in [(dict(repetition_penalty=1e-50), "> 0 in fp32"), (dict(repetition_penalty=1e39), "fp32"), (dict(frequency_penalty=1e39), "fp32"),
                    (dict(presence_penalty=-1e39), "fp32"), (dict(logit_bias={3: 1e39}), "fp32")]:
        with pytest.raises(ValueError, match=msg):
            check_controls(32, **kw)
    assert check_controls(32, 1e-44, 3e38, -3e38)["repetition_penalty"] == 1e-44  # an fp32 denormal is positive; 3e38 is finite
    for bad in ('{"tokens": [1], "repetition_penalty": 1e-50}', '{"tokens": [1], "frequency_penalty": 1e39}', '{"tokens": [1], "logit_bias": {"3": -1e39}}'):
        with pytest.raises(ValueError, match="line 1"):
            parse_requests([bad], 5)


def test_processors_refuse_a_vocabulary_the_launch_cannot_take():
    import torch
    from teal_amd.gpt_fast.logit_processors import LogitProcessors
    for vocab in (12, 4, 0, 131072 + 8, 50257):
        with pytest.raises(ValueError, match="multiple of 8 in 8..131072"):
            LogitProcessors(2, vocab, torch.float16, "cpu")  # refused before anything is allocated or launched


class FakeProcessorEngine(FakeEngine):
    """FakeEngine whose admit takes the processor keywords and records them; the draws stay the plain ones"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.on_calls, self.kws = [], []

    def set_logit_processors(self, on):
        self.on_calls.append(on)

    def admit(self, slot, tokens, budget, eos_id, seed, temperature, top_k, **kw):
        assert not kw or self.on_calls == [True], "controls before set_logit_processors(True)"
        self.kws.append((seed, dict(kw)))
        super().admit(slot, tokens, budget, eos_id, seed, temperature, top_k)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_batcher_passes_controls_for_exactly_the_requests_that_carry_them(K):
    carry = {1: dict(repetition_penalty=1.3), 4: dict(frequency_penalty=0.5, logit_bias={"7": -100.0}), 8: dict(presence_penalty=-0.25),
             9: dict(repetition_penalty=1.0)}  # (request 9 spells out "off": it carries nothing)
    reqs = [Request(q.tokens, q.max_new_tokens, **carry.get(r, {})) for r, q in enumerate(REQS)]
    eng = FakeProcessorEngine()
    b = ContinuousBatcher(eng, sync_every=K)
    res = b.run(reqs)
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(REQS)]
    assert len(set(s for s, _, _ in eng.log)) == 4 and len(eng.log) == len(REQS)  # 10 requests through 4 slots: refills
    want = {1234 + r: ({} if r == 9 else carry.get(r, {})) for r in range(len(REQS))}
    assert dict(eng.kws) == want and len(eng.kws) == len(REQS)
    b.run(reqs)
    assert eng.on_calls == [True]  # once per batcher: the call drops the engine's captured step


def test_batcher_defaults_reach_requests_that_set_none_of_their_own():
    reqs = [Request([1, 2], 3), Request([1, 2], 3, repetition_penalty=1.0, frequency_penalty=0.5), Request([1], 2, presence_penalty=0.0)]
    eng = FakeProcessorEngine()
    ContinuousBatcher(eng, sync_every=2, repetition_penalty=1.2, presence_penalty=0.1).run(reqs)
    assert [kw for _, kw in eng.kws] == [dict(repetition_penalty=1.2, presence_penalty=0.1), dict(presence_penalty=0.1, frequency_penalty=0.5),
                                         dict(repetition_penalty=1.2)]
    for bad in (dict(repetition_penalty=0.0), dict(presence_penalty=float("nan")), dict(frequency_penalty="x")):
        with pytest.raises(ValueError):
            ContinuousBatcher(FakeProcessorEngine(), **bad)


def test_an_engine_without_the_keywords_runs_plain_requests_unchanged():
    eng = FakeEngine()  # admit takes no processor keyword and there is no set_logit_processors
    assert not hasattr(eng, "set_logit_processors")
    res = ContinuousBatcher(eng, sync_every=3).run(REQS)
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(REQS)]


# ---- generate.py ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,msg", [
    (("--synthetic", "tiny-test", "--compile", "--repetition_penalty", "0"), "repetition_penalty must be a finite number > 0"),
    (("--synthetic", "tiny-test", "--compile", "--frequency_penalty", "nan"), "frequency_penalty must be a finite number"),
    (("--synthetic", "tiny-test", "--presence_penalty", "0.5"), "fused engine"),                            # the module path
    (("--synthetic", "tiny-test", "--compile", "--no_engine", "--repetition_penalty", "1.2"), "fused engine"),
    (("--synthetic", "tiny-test", "--compile", "--dense", "--frequency_penalty", "0.2"), "thresholds"),
    (("--synthetic", "tiny-test", "--compile", "--self_speculate", "--repetition_penalty", "1.2"), "speculative"),
    (("--checkpoint_path", "ck/Llama-2-7b/model.pth", "--compile", "--presence_penalty", "1"), "thresholds"),
])
def test_check_processor_args_refusals(extra, msg):
    with pytest.raises(SystemExit, match=msg):
        G.check_processor_args(_args(*extra))


def test_check_processor_args_refuses_tensor_parallel(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="tensor parallelism"):
        G.check_processor_args(_args("--synthetic", "tiny-test", "--compile", "--repetition_penalty", "1.2"))


def test_check_processor_args_accepts_the_engine_paths(tmp_path):
    a = _args()
    assert a.repetition_penalty is None and a.presence_penalty is None and a.frequency_penalty is None
    assert G.check_processor_args(_args("--synthetic", "tiny-test")) == {}
    assert G.check_processor_args(_args("--synthetic", "tiny-test", "--repetition_penalty", "1.0", "--presence_penalty", "0")) == {}  # off is off
    assert G.check_processor_args(_args("--synthetic", "tiny-test", "--compile", "--repetition_penalty", "1.2")) == {"repetition_penalty": 1.2}
    assert G.check_processor_args(_args("--synthetic", "tiny-test", "--engine", "--presence_penalty", "0.5", "--frequency_penalty", "-0.1")) == \
        {"presence_penalty": 0.5, "frequency_penalty": -0.1}
    assert G.check_processor_args(_args("--synthetic", "tiny-test", "--compile", "--batch_size", "4", "--frequency_penalty", "2")) == {"frequency_penalty": 2.0}
    assert G.check_processor_args(_args("--synthetic", "tiny-test", "--requests", str(tmp_path / "r.jsonl"), "--repetition_penalty", "1.1")) == \
        {"repetition_penalty": 1.1}
