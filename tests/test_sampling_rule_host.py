"""Host: the model of per-request sampling (tests/sampling_rule.py) pinned before tests/test_sampling_gpu.py holds teal_sample_rows
to it, and the host side of the feature (requests, check_sampling, the entry point's argument checks).

  1. with top_p = 1 and min_p = 0 the model's draws are sampler_rule.draws' on the shared sampler cases;
  2. hand-worked rows at V = 8, each with its kept count;
  3. on rows without equal values the kept set is a float64 restatement of HF's top-k, top-p and min-p warpers, in that order;
  4. parse_requests reads and validates "temperature", "top_k", "top_p", "min_p" and "seed"; Request defaults resolve; the batcher
     switches the feature on exactly when a setting differs from what the fused top-k samplers serve;
  5. check_sampling's refusals;
  6. teal_sample_rows' argument checks (before any HIP call: no device needed);
  7. the cap: on the GPU test's own case list the model calls at most 15 % of the rows of any configuration open — and the
     surveyed grid at most 10 %, while nearly flat rows (randn * 1, no top-k) are open most of the time and are not used.
"""
import ctypes

import numpy as np
import pytest

import sampler_cases as C
import sampler_rule as SR
import sampling_cases as SC
import sampling_rule as R
from teal_amd import _lib
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request, parse_requests
from teal_amd.gpt_fast.sampling import check_sampling, row_words
from test_continuous_host import FakeEngine, _args, _resources

OK, ARG, DTYPE, SHAPE, ALIGN = 0, -1, -2, -3, -4


@pytest.mark.parametrize("V", [8, 1000, 4096, 32768])
def test_without_top_p_and_min_p_the_draws_are_the_top_k_samplers(V):
    for law, top_k, T, seed in C.cases(V)[::3]:
        for bf16 in (False, True):
            bits = C.logits_bits(law, V, bf16)
            tok, ru, op, count, is_open, counts = R.draws(bits, bf16, T, top_k, 1.0, 0.0, seed, 0, 4)
            want = SR.draws(bits, bf16, top_k, T, seed, 0, 4)
            assert np.array_equal(tok, want[0]) and np.array_equal(ru, want[1]) and np.array_equal(op, want[2]), (law, top_k, T)
            assert count == int(SR.kept_set(bits, bf16, top_k).sum()) and not is_open and counts == (count,)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name,values,params,want", SC.HAND, ids=[h[0] for h in SC.HAND])
def test_hand_worked_rows(name, values, params, want, bf16):
    bits = SC.hand_bits(values, bf16)
    assert SR.decode(bits, bf16).tolist() == list(values)  # exact in both dtypes
    T, k, p, m = params
    mask, count, is_open, counts = R.kept(bits, bf16, T, k, p, m)
    assert count == want and mask.sum() == want and not is_open and counts == (want,)
    x = np.asarray(values)
    assert mask.tolist() == (x >= np.sort(x)[::-1][want - 1]).tolist()  # the `want` largest values, ties whole


def _hf_kept(x, T, top_k, top_p, min_p):
    """HF's TopKLogitsWarper, TopPLogitsWarper and MinPLogitsWarper, in this order, on scores x / T, in float64 (rows without equal
    values; min_tokens_to_keep = 1)"""
    s = np.asarray(x, dtype=np.float64) / T
    V = s.size
    if 0 < top_k < V:
        s = np.where(s < np.sort(s)[V - top_k], -np.inf, s)
    if top_p < 1.0:
        order = np.argsort(s)  # ascending
        e = np.exp(s[order] - s.max())
        cum = np.cumsum(e / e.sum())
        remove = cum <= 1.0 - top_p
        remove[-1] = False
        s = s.copy()
        s[order[remove]] = -np.inf
    if min_p > 0.0:
        e = np.exp(s - s.max())
        probs = e / e.sum()
        s = np.where(probs < min_p * probs.max(), -np.inf, s)
    return np.isfinite(s)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
def test_the_kept_set_is_hfs_warpers_in_order(bf16):
    g = np.random.default_rng(5 + bf16)
    checked = 0
    for V in (8, 32, 64):  # (larger rows nearly always hold two equal 16-bit values)
        for _ in range(80):
            bits = C._to_bits(g.standard_normal(V) * 3, bf16)
            x = SR.decode(bits, bf16).astype(np.float64)
            if np.unique(x).size != V:
                continue
            T = float(g.choice([0.5, 0.8, 1.0, 1.7]))
            k = int(g.choice([0, 1, 5, V // 2, V]))
            p = float(g.choice([0.1, 0.5, 0.9, 0.99, 1.0]))
            m = float(g.choice([0.0, 0.01, 0.1, 0.5]))
            # the model's t is rounded to fp32 twice, HF's here is float64: leave a row to the other tests where that could decide
            mask, count, is_open, _ = R.kept(bits, bf16, T, k, p, m, margin=1e-4)
            if is_open:
                continue
            assert np.array_equal(mask, _hf_kept(x, T, k, p, m)), (V, T, k, p, m)
            checked += 1
    assert checked > 80


def test_open_rows_name_both_neighbours():
    # weights 1, 1/2, 1/4, 1/4 exactly (T = 1 / ln 2 would need an irrational; use the model's own numbers instead): a top_p set ON a
    # boundary.  Masses above the classes of LADDER at T = 1: 0, 1, 1.36788, ...; top_p * Z = 1 exactly on the second class' boundary
    bits = SC.hand_bits(SC.LADDER, False)
    w = np.exp(np.arange(0, -8, -1, dtype=np.float64))
    p_on = 1.0 / w.sum()
    mask, count, is_open, counts = R.kept(bits, False, 1.0, 0, p_on, 0.0)
    assert is_open and set(counts) == {1, 2} and count in counts
    _, count, is_open, counts = R.kept(bits, False, 1.0, 0, p_on * 1.001, 0.0)
    assert not is_open and counts == (2,)
    _, count, is_open, counts = R.kept(bits, False, 1.0, 0, 1.0, float(w[3]))   # min_p on the fourth value
    assert is_open and set(counts) == {3, 4}
    _, count, is_open, counts = R.kept(bits, False, 1.0, 2, 1.0, float(w[3]))   # ... which top_k = 2 has dropped already
    assert counts == (2,) and not is_open
    _, count, is_open, counts = R.kept(bits, False, 1.0, 0, 1e-6, 0.0)          # a tiny nucleus: the maximum, and never open for it
    assert counts == (1,) and not is_open


# ---- requests, the batcher, the flags ---------------------------------------------------------------------------------------------
def test_parse_requests_reads_and_validates_the_sampling_fields():
    lines = ['{"tokens": [1, 2, 3]}',
             '{"tokens": [4], "temperature": 0, "top_k": 1, "top_p": 0.9, "min_p": 0.05, "seed": 77}',
             '{"tokens": [5], "top_p": 1, "top_k": 0}']
    rs = parse_requests(lines, 20)
    assert (rs[0].temperature, rs[0].top_k, rs[0].top_p, rs[0].min_p, rs[0].seed) == (None,) * 5
    assert (rs[1].temperature, rs[1].top_k, rs[1].top_p, rs[1].min_p, rs[1].seed) == (0.0, 1, 0.9, 0.05, 77)
    base = {"temperature": 0.8, "top_k": 200, "top_p": 0.95, "min_p": 0.0}
    assert rs[0].sampling(base) == base
    assert rs[1].sampling(base) == {"temperature": 0.0, "top_k": 1, "top_p": 0.9, "min_p": 0.05}
    assert rs[2].sampling(base) == {"temperature": 0.8, "top_k": 0, "top_p": 1.0, "min_p": 0.0}  # a request's own "off" wins
    assert Request([1], 3).sampling(dict(base, top_k=None))["top_k"] == 0
    for bad, msg in [('{"tokens": [1], "temperature": -0.5}', 'line 1: "temperature"'), ('{"tokens": [1], "temperature": "hot"}', "temperature"),
                     ('{"tokens": [1], "temperature": NaN}', "temperature"), ('{"tokens": [1], "temperature": 1e39}', "temperature"),
                     ('{"tokens": [1], "top_k": -1}', '"top_k" must be a non-negative integer'), ('{"tokens": [1], "top_k": 2.5}', "top_k"),
                     ('{"tokens": [1], "top_k": true}', "top_k"), ('{"tokens": [1], "top_p": 0}', '"top_p" must be a finite number > 0'),
                     ('{"tokens": [1], "top_p": -0.1}', "top_p"), ('{"tokens": [1], "top_p": Infinity}', "top_p"),
                     ('{"tokens": [1], "top_p": 1e-50}', "top_p"), ('{"tokens": [1], "top_p": null}', "top_p"),
                     ('{"tokens": [1], "min_p": 1}', r'"min_p" must be a number in \[0, 1\)'), ('{"tokens": [1], "min_p": -0.01}', "min_p"),
                     ('{"tokens": [1], "min_p": 0.99999999999}', "min_p"), ('{"tokens": [1], "min_p": "x"}', "min_p"),
                     ('{"tokens": [1], "seed": -1}', '"seed" must be a non-negative integer'), ('{"tokens": [1], "seed": 1.5}', "seed"),
                     ('{"tokens": [1], "seed": 9223372036854775808}', "seed")]:
        with pytest.raises(ValueError, match=msg):
            parse_requests([bad], 5)
    with pytest.raises(ValueError, match="line 2"):
        parse_requests(['{"tokens": [1]}', '{"tokens": [1], "top_p": 0}'], 5)
    assert parse_requests(['{"tokens": [1], "top_p": 3}'], 5)[0].top_p == 3.0  # 1 or more: the filter is off


class _SamplingEngine(FakeEngine):
    """FakeEngine that records what the batcher tells it about sampling"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.switched, self.admitted = [], []

    def set_sampling_params(self, on):
        self.switched.append(on)

    def admit(self, slot, tokens, budget, eos_id, seed, temperature, top_k, **kw):
        self.admitted.append((seed, temperature, top_k, kw))
        super().admit(slot, tokens, budget, eos_id, seed, temperature, top_k)


def test_the_batcher_switches_the_feature_on_exactly_when_a_setting_differs():
    plain = [Request([1, 2], 3), Request([3], 4, temperature=0.8, top_k=50, top_p=1.0, min_p=0.0), Request([4], 2, seed=9)]
    eng = _SamplingEngine(B=2)
    ContinuousBatcher(eng, temperature=0.8, top_k=50, use_graph=False).run(plain)
    assert eng.switched == [] and all(a[1:] == (0.8, 50, {}) for a in eng.admitted)  # today's calls, keyword for keyword
    assert [a[0] for a in eng.admitted] == [1234, 1235, 9]
    for reqs, kw in [([Request([1], 3, top_p=0.9)] + plain, {}), ([Request([1], 3, temperature=0.0)] + plain, {}),
                     ([Request([1], 3, top_k=0)] + plain, {}), ([Request([1], 3, min_p=0.1)] + plain, {}),
                     (plain, dict(top_p=0.95)), (plain, dict(min_p=0.05))]:
        eng = _SamplingEngine(B=2)
        b = ContinuousBatcher(eng, temperature=0.8, top_k=50, use_graph=False, **kw)
        b.run(reqs)
        assert eng.switched == [True]
        for (seed, T, k, akw), r in zip(eng.admitted, reqs):
            s = r.sampling({"temperature": 0.8, "top_k": 50, "top_p": kw.get("top_p", 1.0), "min_p": kw.get("min_p", 0.0)})
            assert (T, k, akw) == (s["temperature"], s["top_k"], {"top_p": s["top_p"], "min_p": s["min_p"]})
        b.run(plain)
        assert eng.switched == [True]  # once
    for kw, msg in [(dict(top_p=0.0), "top_p"), (dict(min_p=1.0), "min_p")]:
        with pytest.raises(ValueError, match=msg):
            ContinuousBatcher(FakeEngine(), **kw)


def test_check_sampling_validates_with_the_reason():
    assert check_sampling() == {"temperature": 0.8, "top_k": 0, "top_p": 1.0, "min_p": 0.0}
    assert check_sampling(0, 5, 2.0, 0.5) == {"temperature": 0.0, "top_k": 5, "top_p": 2.0, "min_p": 0.5}
    for kw, msg in [(dict(temperature=-1.0), ">= 0"), (dict(temperature=float("nan")), "finite"), (dict(temperature="1"), "finite number"),
                    (dict(temperature=1e39), "fp32"), (dict(top_k=-1), "non-negative integer"), (dict(top_k=1.5), "non-negative integer"),
                    (dict(top_k=True), "non-negative integer"), (dict(top_k=2 ** 31), "non-negative integer"),
                    (dict(top_p=0.0), "> 0"), (dict(top_p=-0.5), "> 0"), (dict(top_p=float("inf")), "finite"), (dict(top_p=float("nan")), "finite"),
                    (dict(top_p=1e-50), "> 0 in fp32"), (dict(min_p=1.0), r"\[0, 1\)"), (dict(min_p=-0.1), r"\[0, 1\)"),
                    (dict(min_p=1 - 1e-12), r"\[0, 1\) in fp32"), (dict(min_p=float("nan")), "finite")]:
        with pytest.raises(ValueError, match=msg):
            check_sampling(**kw)
    words = row_words(check_sampling(0.8, 200, 0.9, 0.05)).numpy()
    assert words.view(np.float32)[[0, 2, 3]].tolist() == [np.float32(0.8), np.float32(0.9), np.float32(0.05)] and words[1] == 200


@pytest.mark.parametrize("extra,msg", [
    (("--synthetic", "tiny-test", "--compile", "--top_p", "0"), "--top_p must be a finite number > 0 .1: off., got 0.0"),
    (("--synthetic", "tiny-test", "--compile", "--min_p", "1"), "--min_p must be a number in"),
    (("--synthetic", "tiny-test", "--compile", "--self_speculate", "--top_p", "0.9"), "speculative"),
    (("--synthetic", "tiny-test", "--top_p", "0.9"), "need a fused engine"),
    (("--synthetic", "tiny-test", "--compile", "--no_engine", "--min_p", "0.1"), "need a fused engine"),
    (("--checkpoint_path", "ck/model.pth", "--compile", "--top_p", "0.9"), "TEAL thresholds"),
])
def test_check_sampling_args_refusals(extra, msg):
    with pytest.raises(SystemExit, match=msg):
        G.check_sampling_args(_args(*extra))


def test_check_sampling_args_on_the_engine_paths(monkeypatch):
    assert G.check_sampling_args(_args("--synthetic", "tiny-test")) == {}
    assert G.check_sampling_args(_args("--synthetic", "tiny-test", "--top_p", "1.0", "--min_p", "0")) == {}  # spelled-out "off" needs nothing
    assert G.check_sampling_args(_args("--synthetic", "tiny-test", "--compile", "--top_p", "0.9")) == {"top_p": 0.9, "min_p": 0.0}
    assert G.check_sampling_args(_args("--synthetic", "tiny-test", "--requests", "r.jsonl", "--min_p", "0.1")) == {"top_p": 1.0, "min_p": 0.1}
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="tensor parallelism"):
        G.check_sampling_args(_args("--synthetic", "tiny-test", "--compile", "--top_p", "0.9"))


# ---- the entry point's argument checks ---------------------------------------------------------------------------------------------
class _Mem:
    """host memory at a 16-byte aligned address (never dereferenced: every call below is refused before any HIP call)"""

    def __init__(self, nbytes=8192):
        self.buf = ctypes.create_string_buffer(nbytes + 16)
        self.ptr = (ctypes.addressof(self.buf) + 15) & ~15


def _rows_args(**kw):
    m = _Mem()
    a = dict(logits=m.ptr, stride=40, vocab=32, dtype=0, B=2, params=m.ptr + 1024, rng_state=m.ptr + 2048, tokens=m.ptr + 3072,
             pos=m.ptr + 3200, history=m.ptr + 4096, history_len=4, kept=m.ptr + 3328, active=None, slot0=0, stream=None)
    a.update(kw)
    return m, tuple(a.values())


@pytest.mark.parametrize("kw,want", [
    (dict(vocab=12), SHAPE), (dict(vocab=0), SHAPE), (dict(vocab=131072 + 8), SHAPE), (dict(vocab=-8), SHAPE),
    (dict(logits=None), ARG), (dict(params=None), ARG), (dict(rng_state=None), ARG), (dict(tokens=None), ARG),
    (dict(B=0), ARG), (dict(B=9), ARG), (dict(slot0=31), ARG), (dict(slot0=-1), ARG), (dict(slot0=30, B=3), ARG), (dict(history_len=-1), ARG),
    (dict(dtype=2), DTYPE), (dict(dtype=-1), DTYPE), (dict(stride=36), ALIGN),
])
def test_sample_rows_error_codes_without_a_device(kw, want):
    L = _lib.load()
    keep, args = _rows_args(**kw)
    assert L.teal_sample_rows(*args) == want
    del keep


def test_sample_rows_refuses_an_odd_row_address():
    L = _lib.load()
    keep, args = _rows_args()
    assert L.teal_sample_rows(args[0] + 2, *args[1:]) == ALIGN
    keep, args = _rows_args(B=1, stride=36, logits=None)  # (one row: the stride is not looked at, the null pointer is)
    assert L.teal_sample_rows(*args) == ARG


def test_the_new_unit_is_built_like_the_logit_processors_and_its_resources_are_pinned(tmp_path):
    assert "teal_sample_rows.hip" in _lib.SOURCES and "teal_sample_rows.hip" not in _lib.PRELOAD
    res = _resources(tmp_path, "teal_sample_rows.hip")
    assert len(res) == 4, sorted(res)  # {fp16, bf16} x {4, 16 key vectors per thread}
    small = {k: v for k, v in res.items() if "Li4E" in k}
    large = {k: v for k, v in res.items() if "Li16E" in k}
    assert len(small) == 2 and all(v == (0, 0) for v in small.values()), res
    # 16 key vectors are 64 of the 128 VGPRs a thread of a 1024-thread workgroup can have: a few values spill, as in the fused
    # sampler's 16-vector window kernel.  Pinned where it stands so that growth is noticed.
    assert len(large) == 2 and all(sc <= 64 and sp <= 15 for sc, sp in large.values()), res


# ---- the cap ---------------------------------------------------------------------------------------------------------------------
def _open_share(rows, bf16, params):
    T, k, p, m = params
    return float(np.mean([R.kept(r, bf16, T, k, p, m)[2] for r in rows]))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
def test_at_most_15_percent_of_a_configurations_rows_are_open(bf16):
    """the GPU test's own list: every vocabulary, every configuration of the grid on the vocabulary's random rows, and the launch
    with eight different rows of settings"""
    for V in SC.VOCABS:
        rows = SC.random_rows(V, bf16)
        for params in SC.GRID:
            share = _open_share(rows, bf16, params)
            assert share <= 0.15, (V, params, share)
        mixed = np.mean([R.kept(rows[j], bf16, *SC.MIXED[j])[2] for j in range(SC.N_ROWS)])
        assert mixed <= 0.15, (V, "mixed", float(mixed))
        for name, bits in SC.special_rows(V, bf16):
            for params in SC.GRID[:2] + SC.GRID[4:]:
                _, count, is_open, counts = R.kept(bits, bf16, *params)
                assert not is_open, (V, name, params, counts)  # a degenerate row has no close decision


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
def test_the_surveyed_grid_is_open_in_at_most_10_percent_and_flat_rows_are_not_used(bf16):
    g = np.random.default_rng(99 + bf16)
    for V in SC.CAP_VOCABS:
        rows = [C._to_bits(g.standard_normal(V) * 3, bf16) for _ in range(20)]
        for p in (0.5, 0.9):
            for k in (0, 200):
                share = _open_share(rows, bf16, (0.8, k, p, 0.0))
                assert share <= 0.10, (V, k, p, share)
    # nearly flat rows: thousands of values per mass step of 1e-5 * Z — some boundary is nearly always inside the margin
    flat = [C._to_bits(g.standard_normal(32000), bf16) for _ in range(10)]
    assert _open_share(flat, bf16, (0.8, 0, 0.9, 0.0)) >= 0.5
