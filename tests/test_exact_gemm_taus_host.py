"""CPU: the exact-integer probes of teal_batched_sparse_gemm_slot_taus (tests/exact_gemm_taus.py) can see what they claim to see.

tests/test_exact_gemm_taus_gpu.py compares every slab and count word of the per-slot-threshold GEMM with an integer reference.
Here, without a GPU, the numpy model of the documented row walk runs on the VERY cases the GPU test launches:

  * unmutated, the model equals the reference, word for word (slabs, sentinels, counts);
  * each mutant of the staging compare — every slot under slot 0's column, slot b under column b + 1, the segment index ignored,
    the union taken under slot 0's column only, an inactive slot's column consulted — changes at least one checked word in
    EVERY case that lists it, and every mutant is listed;
  * the ledger's claims hold for every case: each slot keeps the prescribed rows (counted from the histogram of its |x|, not
    from the masks), some row is kept by exactly one slot, some row is kept by none and carries NaN weights, an inactive slot
    sits behind a NaN column; and the tables together hold -inf, ties at the threshold and a +inf column.
"""
import numpy as np
import pytest

import exact_gemm as X
import exact_gemm_taus as XT

CASES = XT.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_model_equals_reference_claims_hold_and_mutants_are_caught(name):
    c = CASES[name]
    b = XT.build(c, c.expect_split)
    led = XT.check_claims(b)
    words, cnt = XT.walk(b)
    assert X.first_diff(words, b.slabs) is None, (name, X.first_diff(words, b.slabs))
    assert X.first_diff(cnt, b.counts) is None, (name, X.first_diff(cnt, b.counts))
    assert b.bound < 2 ** 24
    for mut in c.tmutants:
        assert mut in XT.MUTANTS
        mw, mc = XT.walk(b, mut)
        assert X.first_diff(mw, b.slabs) is not None or X.first_diff(mc, b.counts) is not None, (name, mut, "not noticed")
    print(f"PROBE host {name} split={b.split} kept={led['kept'].tolist()} solo={led['solo']} none_poisoned={led['none_poisoned']} "
          f"nan_inactive={led['nan_inactive']} inf_columns={led['inf_columns']} ties={led['ties']} mutants={','.join(c.tmutants) or '-'} caught")


def test_every_mutant_every_claim_and_every_table_entry_is_covered():
    muts, claims, drawn = set(), set(), set()
    for c in CASES.values():
        muts |= set(c.tmutants)
        claims |= set(c.tclaims)
        live = np.array(c.live, bool)
        drawn |= {float(v) for v in c.taus[: c.nseg][:, live].ravel()}
        assert "kept" in c.tclaims, c.name
        # NaN only where nothing may be consulted: the table rows past the last segment and, by default, the inactive slots
        assert np.isnan(c.taus[c.nseg:]).all() and not np.isnan(c.taus[: c.nseg][:, live]).any(), c.name
    assert muts == set(XT.MUTANTS)
    assert claims >= {"kept", "solo", "none_poisoned", "nan_inactive", "inf_column", "neg_inf", "ties"}
    assert drawn == set(XT.POOL), sorted(set(XT.POOL) - drawn)
    # shapes: nothing larger than exact_gemm's own, one to three segments, both dtypes, the three producers, two phases
    assert max(c.Z for c in CASES.values()) <= max(g.Z for g in X.gemm_cases().values() if g.entry == "batched")
    assert {c.nseg for c in CASES.values()} == {1, 2, 3} and {c.dt for c in CASES.values()} == {"fp16", "bf16"}
    assert {c.mode for c in CASES.values()} == {X.IN_XT, X.IN_NORM, X.IN_SILU_MUL}
    assert any(c.claims.get("phases") == 2 for c in CASES.values())
    assert {c.NP for c in CASES.values()} == {1, 2, 3, 4}


def test_equal_columns_are_the_slots_reference():
    """with every column equal to the segment's threshold the table reference is exact_gemm's own `_slots` reference"""
    for name, g in X.gemm_cases().items():
        if g.entry != "slots" or g.Z > 512:
            continue
        b = X.build(g, g.expect_split)
        slabs, counts = b.slabs.copy(), b.counts.copy()
        g.taus, g.nseg = np.full((3, 8), np.nan), len(g.tau)
        g.taus[: g.nseg] = np.array(g.tau)[:, None]
        XT.reference(b)
        assert X.first_diff(b.slabs, slabs) is None and X.first_diff(b.counts, counts) is None, name
