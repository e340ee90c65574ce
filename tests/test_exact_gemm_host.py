"""CPU: the exact-integer probes of the GEMM chain (tests/exact_gemm.py) can see what they claim to see.

tests/test_exact_gemm_gpu.py compares every word the launches write with an integer reference, bit for bit.  Here, without a
GPU, a numpy model of the documented row walk (slices, phases of 2048 rows — 1024 for R = 16 —, 64-row chunks, the compacted
list dealt to 16 waves, guarded repeats, per-lane segment selection, pairs of slots) runs on the VERY cases the GPU test
launches, at the split the host's rule gives on a 256-CU device:

  * unmutated, the model equals the reference, word for word (slabs, sentinels, counts);
  * each mutant of the walk — a dropped list entry, a neighbour's mask, segment 0's tau past e0, a guarded repeat that adds,
    a skipped last partial chunk, the previous phase's list carried over, phase 2's first row counted twice, an inactive
    slot's activation let through — changes at least one checked word in EVERY case that lists it;
  * the rounding mutants — slices added last to first (a tie case where the order matters exists: exact_gemm.order_slabs),
    two roundings, truncation — change at least one word of every teal_batched_round_rows case and of every tie case of
    teal_prefill_resid_norm;
  * the builders' own assertions (the exactness bound, the tie margins of the producers, representability) hold for every
    case, and the cases together claim every ledger class the issue asks for.
"""
import math

import numpy as np
import pytest

import exact_gemm as X

GEMM = X.gemm_cases()
RESID = X.resid_cases()
ROUND = X.ROUND_CASES


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()  # (one case at a time: the large ones hold tens of megabytes)
            cache[name] = X.build(GEMM[name], GEMM[name].expect_split)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(GEMM))
def test_model_equals_reference_and_mutants_are_caught(built, name):
    b = built(name)
    c = b.case
    led = X.check_claims(b)  # at the expected split the case hits the classes it was written for
    words, cnt = X.walk(b)
    assert X.first_diff(words, b.slabs) is None, (name, X.first_diff(words, b.slabs))
    if b.counts is not None:
        assert X.first_diff(cnt, b.counts) is None, (name, X.first_diff(cnt, b.counts))
    assert b.bound < 2 ** 24
    for mut in c.mutants:
        assert mut in X.MUTANTS
        mw, mc = X.walk(b, mut)
        changed = X.first_diff(mw, b.slabs) is not None or (mc is not None and X.first_diff(mc, b.counts) is not None)
        assert changed, (name, mut, "not noticed", led)
    print(f"PROBE host {name} split={b.split} mutants={','.join(c.mutants) or '-'} caught")


def test_every_mutant_and_every_class_is_claimed():
    muts = set()
    for c in GEMM.values():
        muts |= set(c.mutants)
    assert muts == set(X.MUTANTS)
    # per kernel: what the issue's "done when" lists
    led = {n: X.ledger(X.build(c, c.expect_split)) for n, c in GEMM.items() if c.Z <= 4352}
    big = {n: c.claims for n, c in GEMM.items() if c.Z > 4352}
    for entry in ("batched", "prefill"):
        assert any(c.get("phases") == 2 and GEMM[n].entry == entry for n, c in big.items())
        assert {GEMM[n].mode for n in GEMM if GEMM[n].entry == entry} == {X.IN_XT, X.IN_NORM, X.IN_SILU_MUL}
    assert any(c.get("last_phase_rows") == [16] for c in big.values())
    lists = set().union(*[set(l["list"]) for l in led.values()])
    assert {"0", "<16", "16U-1", "16U", "16U+1", "32U-1", "32U", "32U+1", "all", "idle wave"} <= lists
    assert any(set(l["last_chunk_rows"]) & {16, 32, 48} for l in led.values())
    assert any(l["segs_per_tile"] == 3 for l in led.values())
    assert {l["NP"] for l in led.values() if l["entry"] == "batched"} == {1, 2, 3, 4}
    assert {l["NP"] for l in led.values() if l["entry"] == "prefill"} >= {1, 2, 3, 4, 5, 8}
    assert {l["R"] for l in led.values()} == {8, 16}
    assert {l["guarded"][-1] for l in led.values()} >= {1, 2}
    used = set()
    for c in GEMM.values():
        used |= set(c.tau)
    assert used == set(X.TAUS), sorted(set(X.TAUS) - used)


def test_rne16_is_the_formats_rounding():
    import torch
    rng = np.random.default_rng(3)
    for dt in ("fp16", "bf16"):
        v = np.concatenate([rng.integers(-16384, 16384, 4000).astype(np.float64), rng.normal(0, 50, 4000).astype(np.float32).astype(np.float64),
                            np.array([2049.0, 2051.0, 257.0, 259.0, 8197.0, 1029.0, 0.0, -2049.0])])
        v = v[(np.abs(v) >= 2.0 ** -14) | (v == 0)]
        want = torch.from_numpy(v).float().to(X.TDT[dt]).double().numpy()
        assert np.array_equal(X.rne16(v, dt), want)
        lo = X.TIE_LO[dt]
        assert X.rne16(lo + 1.0, dt) == lo and X.rne16(lo + 3.0, dt) == lo + 4          # ties to even
        assert X.rne16(4.0 * lo + 5.0, dt) == 4.0 * lo + 8 and X.rne16(4.0 * lo + 5.0, dt, "twice") == 4.0 * lo  # double rounding
        assert X.rne16(lo + 1.5, dt, "trunc") == lo


@pytest.mark.parametrize("dt,N,B,split", ROUND)
def test_round_rows_cases_kill_the_rounding_mutants(dt, N, B, split):
    parts, slabs, y = X.round_rows_case(dt, N, B, split, seed=N + B + split)
    X.bits16(y, dt)  # representable
    s = X.sum_slices_f32(parts)
    lo = X.TIE_LO[dt]
    assert (np.abs(s) < 65504).all() and (np.abs(s[1:]) >= lo).all()
    assert ((np.abs(s) < 2 * lo) & (np.mod(np.abs(s), 2) == 1))[:, :B].any(), "no exact tie among the checked words"
    for mut in ("twice", "trunc") + (("reverse",) if split >= 3 else ()):
        ym = X.round_slabs(parts, dt, mut)
        assert (ym != y)[:, :B].any(), (mut, "not noticed")
    if split >= 3:  # the slice-order probe: column 0, slot 0
        assert y[0, 0] == lo and X.round_slabs(parts, dt, "reverse")[0, 0] == lo + 2


@pytest.mark.parametrize("name", list(RESID))
def test_resid_norm_cases(name):
    c = RESID[name]
    b = X.build_resid(c)  # asserts: sums of squares exact integers, rstd a power of two, the tie margins, representability
    assert b.ht.shape == (c.dim, c.R) and not b.ht[:, c.T:].any()
    assert b.sumsq.shape == (c.nwg, c.R)
    if c.kind == "norm":
        assert b.xt is not None and not b.xt[:, c.T:].any()
    else:
        for mut in ("trunc",) + (("twice",) if c.dt == "bf16" else ()) + (("reverse",) if c.split >= 3 else ()):
            ym = X.round_slabs(b.parts, c.dt, mut)
            assert (ym != X.round_slabs(b.parts, c.dt)).any(), (name, mut, "not noticed")
    assert b.tokens.max() <= 18 and (c.path != "tokens" or c.split == 0 or c.T == 1 or len(set(b.tokens.tolist())) < c.T)


def test_resid_cases_cover_the_issue():
    cs = list(RESID.values())
    assert {c.dim for c in cs} == {64, 320, 4096, 16384}
    assert {c.T for c in cs if c.dim == 320} >= {1, 2, 7, 8, 9, 15, 16}
    assert {c.split for c in cs} == {0, 1, 3, 5, 16}
    assert {c.path for c in cs} == {"tokens", "ht_in"} and any(c.inplace for c in cs) and any(c.path == "ht_in" and not c.inplace for c in cs)
    assert {c.outputs for c in cs} >= {("xt", "last"), ("xt",), ("last",), ()}
    assert any(c.dim == 16384 and c.nwg == 64 for c in cs) and {c.eps for c in cs if c.kind == "norm"} == {0.0, 1e-5}  # (1e-5 in bf16 only: powers of two)
    assert math.isinf(X.TAUS[0])
