"""Host: the sampler's model (tests/sampler_rule.py) pinned before tests/test_sampler_gpu.py holds the kernels to it.

  1. the kept set by the kernels' 16-bit keys = the kept set by values (the reference's `logits < pivot -> -inf`);
  2. the race samples softmax(top-k logits / T): Pearson's chi-square over 40 000 counters;
  3. the (seed, counter) streams of continuous batching's default seeds do not coincide;
  4. on every input of the GPU test the model marks at most 1 % of the draws `open`.

NaN logits are out of scope (sampler_rule.py).
"""
import numpy as np
import pytest

import sampler_cases as C
import sampler_rule as R
from spec_rule import order_key16


def _bits(x, bf16):
    return C._to_bits(np.asarray(x, dtype=np.float32), bf16)


def _kept_by_keys(bits, top_k):
    """what row_probs and the kernels do: keys >= the k-th largest key"""
    keys = order_key16(bits)
    if not 0 < top_k < bits.size:
        return np.ones(bits.size, dtype=bool)
    return keys >= np.sort(keys)[::-1][top_k - 1]


def _finite_patterns(g, n, bf16):
    """random 16-bit patterns without NaN (all exponent bits set and a non-zero mantissa)"""
    b = g.integers(0, 1 << 16, n).astype(np.uint16)
    exp_mask, man_mask = (0x7F80, 0x007F) if bf16 else (0x7C00, 0x03FF)
    nan = ((b & exp_mask) == exp_mask) & ((b & man_mask) != 0)
    b[nan] &= np.uint16(~man_mask & 0xFFFF)  # -> +-inf
    return b


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
def test_kept_set_by_keys_equals_kept_set_by_values(bf16):
    g = np.random.default_rng(11 + bf16)
    inputs = {"random patterns": _finite_patterns(g, 4096, bf16),
              "normal": _bits(g.standard_normal(1000) * 3, bf16)}
    x = g.standard_normal(512) * 2
    x[g.choice(512, 60, replace=False)] = np.sort(x)[-20]   # 61 equal values straddling rank 20
    inputs["ties straddling the rank"] = _bits(x, bf16)
    x = g.standard_normal(256)
    x[::3] = -np.inf
    x[5] = np.inf
    inputs["-inf entries"] = _bits(x, bf16)
    sub = g.integers(1, 0x80 if bf16 else 0x400, 128).astype(np.uint16)  # subnormals of both signs around +-0
    sub[::2] |= 0x8000
    inputs["subnormals"] = np.concatenate([sub, np.array([0x0000, 0x8000], dtype=np.uint16), _bits(g.standard_normal(32) * 1e-3, bf16)])
    z = np.array([1.0, -0.0, 0.0, 2.0, -0.0, 0.0, -1.0, 0.0, -0.0, -2.0, 3.0, -0.0])
    inputs["both zeros, pivot on zero"] = _bits(z, bf16)
    assert {0x0000, 0x8000} <= set(inputs["both zeros, pivot on zero"].tolist())
    for name, bits in inputs.items():
        V = bits.size
        for k in sorted({0, 1, 2, 3, 4, 5, 6, 7, 8, 19, 20, 21, 60, 61, 80, 81, V // 2, V - 1, V, V + 1} & set(range(V + 2))):
            by_value, by_key = R.kept_set(bits, bf16, k), _kept_by_keys(bits, k)
            assert np.array_equal(by_value, by_key), (name, k, int(by_value.sum()), int(by_key.sum()))
            assert by_value.sum() >= min(k, V) if k > 0 else by_value.all()
    # the zero case by hand: three values above zero, then four -0.0 and three +0.0 — ranks 4 .. 10 are all "0"
    for k in range(4, 11):
        assert R.kept_set(inputs["both zeros, pivot on zero"], bf16, k).sum() == 10, k


CHI2_ISF_1E4 = {7: 29.878, 31: 69.106}  # scipy.stats.chi2.isf(1e-4, df)


@pytest.mark.parametrize("V,top_k,T", [(64, 8, 0.7), (64, 8, 1.0), (64, 8, 2.0), (32, 0, 0.7), (32, 0, 1.0), (32, 0, 2.0)])
def test_race_samples_softmax_of_the_kept_logits(V, top_k, T):
    n = 40000
    bits = _bits(np.random.default_rng(V).standard_normal(V) * (2.0 if top_k else 1.0), False)
    tok, _, _ = R.draws(bits, False, top_k, T, 2024, 0, n)
    kept = np.flatnonzero(R.kept_set(bits, False, top_k))
    assert kept.size == (top_k or V) and np.isin(tok, kept).all()
    z = R.decode(bits, False).astype(np.float64)[kept] / T
    p = np.exp(z - z.max())
    p /= p.sum()
    expect = p * n
    assert expect.min() > 5, expect.min()  # Pearson's approximation holds
    obs = np.array([(tok == i).sum() for i in kept])
    stat = float(((obs - expect) ** 2 / expect).sum())
    assert stat < CHI2_ISF_1E4[kept.size - 1], f"chi-square {stat:.2f} with {kept.size - 1} degrees of freedom"


def test_draw_is_draws_and_counters_and_seeds_use_their_low_words():
    bits = C.logits_bits("normal", 1000, True)
    tok, ru, op = R.draws(bits, True, 20, 0.8, 77, 5, 6)
    for j in range(6):
        assert R.draw(bits, True, 20, 0.8, 77, 5 + j) == (int(tok[j]), int(ru[j]), bool(op[j]))
    wrapped = R.draws(bits, True, 20, 0.8, 2 ** 32 + 77, 2 ** 32 - 2, 8)[0]
    assert wrapped[2:].tolist() == R.draws(bits, True, 20, 0.8, 77, 0, 6)[0].tolist()
    assert len(set(tok.tolist())) > 1 and (tok != ru).all()


def test_exact_ties_go_to_the_smallest_index():
    for V in (1000, 4096, 32768):
        seed, d, i, j = C.twin_case(V)
        bits = C.logits_bits("twins", V, False)
        tok, ru, op = R.draws(bits, False, 2, 1e-6, seed, 0, C.N_MAIN)
        assert i < j and set(tok.tolist()) <= {i, j} and tok[d] == i
        assert not op[d] and ru[d] == i  # nothing but its twin competes: no other answer is legitimate
    # all equal, T -> 0: a uniform draw over the vocabulary decided by u alone
    tok, _, _ = R.draws(C.logits_bits("equal", 4096, True), True, 0, 1e-6, 3, 0, 64)
    assert len(set(tok.tolist())) > 48


@pytest.mark.xfail(strict=True, reason="hash3's pre-mix words coincide for 8 pairs in this range, e.g. (seed 1250, counter 99) and "
                                       "(seed 1287, counter 1974), both 0x011eb98a: those two draws see the same noise at every "
                                       "vocabulary index (DESIGN.md, sampler parity); changing hash3 moves every token stream")
def test_streams_of_the_default_seeds_do_not_coincide():
    """generate.py and ContinuousBatcher seed request r with 1234 + r: 64 consecutive request seeds x counters 0 .. 4095"""
    words = np.concatenate([R.premix(1234 + r, np.arange(4096)) for r in range(64)])
    assert words.size == 262144
    assert np.unique(words).size == words.size, f"{words.size - np.unique(words).size} coinciding pre-mix words"


def test_premix_is_what_hash3_mixes():
    from spec_rule import hash3
    m = np.uint64(0xFFFFFFFF)
    c = np.arange(50, dtype=np.uint64)
    for seed, ctr in ((1234, 0), (1250, 99), (2 ** 32 + 5, 2 ** 32 - 4)):
        h = R.premix(seed, ctr) ^ ((((c + np.uint64(0x165667B1)) & m) * np.uint64(0xC2B2AE3D)) & m)
        h ^= h >> np.uint64(16)
        h = (h * np.uint64(0x85EBCA6B)) & m
        h ^= h >> np.uint64(13)
        h = (h * np.uint64(0xC2B2AE35)) & m
        h ^= h >> np.uint64(16)
        assert np.array_equal(h, hash3(seed, ctr, c))
    assert np.array_equal(hash3(1250, 99, c), hash3(1287, 1974, c))  # the coinciding pair of the test above


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", list(C.VOCABS))
def test_open_draws_are_rare_on_the_gpu_tests_inputs(V, bf16):
    """a condition on the inputs, not a measurement: a case above the cap gets another seed, the cap stays"""
    worst = 0.0
    for law, top_k, T, seed in C.cases(V):
        bits = C.logits_bits(law, V, bf16)
        for s, c0, n in C.blocks(seed):
            tok, ru, op = R.draws(bits, bf16, top_k, T, s, c0, n)
            assert R.kept_set(bits, bf16, top_k)[tok].all() and (0 <= tok).all() and (tok < V).all()
            assert op.mean() <= 0.01, (law, top_k, T, s, c0, float(op.mean()))
            worst = max(worst, float(op.mean()))
    print(f"V={V} {'bf16' if bf16 else 'fp16'}: {len(C.cases(V))} cases, largest share of open draws {worst:.4f}")
    if V >= 80:
        bits = C.logits_bits("tiemax", V, bf16)
        assert R.kept_set(bits, bf16, 20).sum() == 40  # the whole tie group straddling rank 20 stays drawable
        assert len(set(R.draws(bits, bf16, 20, 1.0, C.SEED, 0, C.N_MAIN)[0].tolist())) > 10
