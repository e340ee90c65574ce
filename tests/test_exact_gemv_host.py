"""CPU: the power of the exact-integer probes of the fused decode GEMV (tests/exact_gemv.py, tests/test_exact_gemv_gpu.py).

For every case of the GPU file, at the geometry the case was written for:
  * the preconditions hold on the reference alone — the 2^24 bounds (int8: in the kernels' bias form), the tie distances of the
    RMSNorm producer, silu's exactness on the gates, steered gate sums in {16, 24, 32} that are never 0, h that changes when any
    single kept term of gate or up is removed — most of them asserted while the case is built, the rest here;
  * the ledger classes the case claims (per-wave list sizes, early / late first chunk, odd / even batch counts, an empty
    workgroup) occur;
  * every mutant the case lists — a switch of the numpy reference or of its model of the per-wave row walk — changes at least
    one compared word of the case's own inputs.
Together the cases kill every mutant of exact_gemv.MUTANTS; the table is printed as `PROBE host` lines.
"""
import functools

import numpy as np
import pytest

import exact_gemv as X

CASES = X.cases()


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in a)


@functools.lru_cache(maxsize=None)
def _study(name):
    """(ledger, {mutant: killed}, words compared) of one case; the built inputs are dropped again"""
    c = CASES[name]
    geo = X.geometry(c)
    b = X.build(c, geo)
    ref = X.reference(b, geo)
    led = X.check_claims(b, geo)
    again = X.reference(b, geo)
    assert not _differs(ref, again), "the reference is not a function of its inputs"
    kills = {}
    for mut in c.mutants:
        got = X.reference(b, geo, mut=mut)
        assert set(got) == set(ref)
        kills[mut] = _differs(ref, got)
    extra = {}
    if c.steer:
        extra["insensitive_terms"] = X.sensitivity(b, geo)
        extra["gate_sums"] = sorted(set(np.unique(b.targets[0]).tolist()))
    extra["bound"] = b.bound
    return led, kills, sum(int(v.size) for v in ref.values()), extra


@pytest.mark.parametrize("name", list(CASES))
def test_case_preconditions_claims_and_mutants(name):
    c = CASES[name]
    led, kills, n, extra = _study(name)
    assert set(c.mutants) <= set(X.MUTANTS)
    alive = [m for m, k in kills.items() if not k]
    assert not alive, f"case {name}: mutants {alive} change no compared word"
    if c.layout != "order":
        assert extra["bound"] < 2 ** 24
    if c.steer:
        assert extra["insensitive_terms"] == 0, "a kept term of gate or up can be removed without changing h"
        assert set(extra["gate_sums"]) <= set(X.GATES) and 0.0 not in extra["gate_sums"]
    if led["kernel"] == "lean":
        assert c.Z % 64 == 0 and all(ncols % (led["lpr"] * 8) == 0 for ncols, _ in c.segs)


def test_every_mutant_is_killed_and_every_class_is_claimed():
    killers = {m: [] for m in X.MUTANTS}
    for name in CASES:
        for m, k in _study(name)[1].items():
            if k:
                killers[m].append(name)
    for m in X.MUTANTS:
        print(f"PROBE host mutant {m}: killed by {len(killers[m])} cases: {', '.join(killers[m][:6])}{' ...' if len(killers[m]) > 6 else ''}")
    assert not [m for m in X.MUTANTS if not killers[m]]
    # the instantiations and size classes the issue names all occur in some case's expectation
    lean = {(c.expect["mode"], c.expect["kr"]) for c in CASES.values() if c.expect["kernel"] == "lean"}
    assert {(0, 1), (0, 4), (0, 8), (1, 4), (1, 8), (1, 16), (2, 4), (3, 4), (4, 4)} <= lean, lean
    for flag in (True, False):
        assert any(c.expect.get("exact", False) == flag for c in CASES.values() if c.expect["kernel"] == "lean" and c.mode == 1)
    assert {c.mode for c in CASES.values() if c.expect["kernel"] == "general"} == {0, 1, 2, 3, 4}
    assert {c.mode for c in CASES.values() if c.w8 and c.expect["kernel"] == "lean"} == {0, 1, 2, 3, 4}
    assert {c.expect["lpr"] for c in CASES.values() if c.expect["kernel"] == "lean" and c.mode in (0, 1)} == {8, 16}
    claimed = set()
    for c in CASES.values():
        claimed |= set(c.claims)
    assert set(X.SIZE_CLAIMS) | {"empty_wg"} <= claimed


def test_chunk_rule_is_a_partition_balanced_to_one_chunk():
    """the documented chunk-to-slice rule: every chunk in exactly one (slice, wave), slices within one chunk of each other"""
    for Z in (64, 1024, 4096, 5120, 11008, 16384, 65536):
        for split in (1, 2, 3, 4, 5, 8):
            for mode in (X.IN_PLAIN, X.IN_RESID_NORM):
                if split > X.rounds_of(Z):
                    continue
                sl, wv = X.chunk_place(Z, split, mode)
                assert sl.min() >= 0 and sl.max() < split and wv.max() < 16
                cnt = np.bincount(sl, minlength=split)
                if mode != X.IN_RESID_NORM:
                    assert cnt.max() - cnt.min() <= 1
                assert cnt.sum() == Z // 64


def test_desc_parser():
    g = X.parse_desc("gemv_fast_kernel<true,1,false,8,4,true,false,4,false,true> grid (156,1) x 1024")
    assert g == dict(kernel="lean", bf16=True, mode=1, pair=False, lpr=8, kr=4, exact=True, w8=False, rope=True, ntiles=156, split=1)
    g = X.parse_desc("sparse_gemv_kernel<8,16,4,false,0,4,false,true> grid 6 x 1024")
    assert g["kernel"] == "general" and g["lpr"] == 8 and g["w8"] and g["workgroups"] == 6 and g["mode"] == 0
