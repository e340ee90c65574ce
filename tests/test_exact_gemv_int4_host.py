"""CPU: the power of the exact-integer probes of the int4 fused GEMV (tests/exact_gemv_int4.py,
tests/test_exact_gemv_int4_gpu.py).

For every case of the GPU file, at the geometry the case was written for:
  * the preconditions hold on the reference alone — activations on the producer's integer grid, nibbles 0..15, bf16
    power-of-two scales and integer zeros, the 2^24 bounds of the kernel's biased accumulators and of every (slice, column)
    sum — most of them asserted while the case is built, the rest here;
  * the ledger classes the case claims (kept-pair counts per unit, half-kept pairs of either parity, differing counts inside a
    GROUP pass, dead units, stale slots, an empty workgroup, rounding ties ...) occur;
  * every mutant the case lists — a switch of the numpy model — changes at least one compared word of the case's own inputs.
Together the cases kill every mutant of exact_gemv_int4.MUTANTS; the table is printed as `PROBE host` lines.
"""
import functools

import numpy as np
import pytest
import torch

import exact_gemv_int4 as X

CASES = X.cases()


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in a)


@functools.lru_cache(maxsize=None)
def _study(name):
    """(ledger, {mutant: killed}, words compared, facts) of one case; the built inputs are dropped again"""
    c = CASES[name]
    geo = X.geometry(c)
    b = X.build(c, geo)
    ref = X.reference(b, geo)
    led = X.check_claims(b, geo)
    assert not _differs(ref, X.reference(b, geo)), "the reference is not a function of its inputs"
    kills = {}
    for mut in c.mutants:
        got = X.reference(b, geo, mut=mut)
        assert set(got) == set(ref)
        kills[mut] = _differs(ref, got)
    xf = np.nan_to_num(b.x) / b.unit
    facts = dict(bound=b.bound, q=(int(b.Q.min()), int(b.Q.max())), dropped_nonzero=float((xf[~X.keepsets(c, b, b.x)[0]] != 0).mean()),
                 pad_ff=bool((b.image[:, c.img_n:] == 0xFF).all()), sz_nan_outside=bool(torch.isnan(b.sz_t[:, c.img_n:]).all()),
                 ld=b.ld, scale_ld=b.scale_ld)
    return led, kills, sum(int(v.size) for v in ref.values()), facts


@pytest.mark.parametrize("name", list(CASES))
def test_case_preconditions_claims_and_mutants(name):
    c = CASES[name]
    led, kills, n, facts = _study(name)
    assert set(c.mutants) <= set(X.MUTANTS)
    alive = [m for m, k in kills.items() if not k]
    assert not alive, f"case {name}: mutants {alive} change no compared word"
    if c.layout != "order":
        assert facts["bound"] < 2 ** 24
    assert facts["q"] == ((9, 15) if c.layout == "order" else (0, 15)) and facts["pad_ff"] and facts["sz_nan_outside"]
    assert facts["ld"] > c.img_n and facts["ld"] % 8 == 0 and facts["scale_ld"] > c.img_n
    if c.mode in (X.IN_PLAIN, X.IN_SILU_MUL) and c.layout != "eps":
        assert facts["dropped_nonzero"] > 0.5, "dropped rows must mostly hold +-1"
    # the expectation is what the shape rule gives on 256 CUs
    rule = X.shape_rule(c)
    assert {k: c.expect[k] for k in rule} == rule, (c.expect, rule)


def test_every_mutant_is_killed_and_every_class_occurs():
    killers = {m: [] for m in X.MUTANTS}
    for name in CASES:
        for m, k in _study(name)[1].items():
            if k:
                killers[m].append(name)
    for m in X.MUTANTS:
        print(f"PROBE host mutant {m}: killed by {len(killers[m])} cases: {', '.join(killers[m][:6])}{' ...' if len(killers[m]) > 6 else ''}")
    assert not [m for m in X.MUTANTS if not killers[m]]
    cs = list(CASES.values())
    assert {c.expect["kind"] for c in cs} == {X.SHARE, X.GROUP}
    assert {c.G for c in cs} == {32, 64, 128, 256}
    for kind in (X.SHARE, X.GROUP):
        assert 256 in {c.G for c in cs if c.expect["kind"] == kind}
    assert {1, 2, 8} <= {c.expect["split"] for c in cs}
    assert {c.mode for c in cs} == {X.IN_PLAIN, X.IN_RESID_NORM, X.IN_SILU_MUL, X.IN_ATTN_MERGE}
    for kind in (X.SHARE, X.GROUP):
        assert {c.mode for c in cs if c.expect["kind"] == kind} == {0, 1, 2, 4}
    assert {(c.out, c.il) for c in cs if c.out == X.OUT_SLABS} == {(X.OUT_SLABS, 0), (X.OUT_SLABS, 1)}
    for il in (0, 1):
        assert {1, 2, 8} <= {c.expect["split"] for c in cs if c.out == X.OUT_SLABS and c.il == il}
    assert {1, 2, 8} <= {c.expect["split"] for c in cs if c.out == X.OUT_ROUNDED}
    assert {c.nslabs for c in cs if c.mode == X.IN_RESID_NORM} >= {0, 1, 3, 4, 5, 8}
    assert {(c.att_ns, c.att_hd) for c in cs if c.mode == X.IN_ATTN_MERGE} == {(4, 64), (4, 128), (8, 64), (8, 128)}
    assert any(c.att_arg == 0 for c in cs if c.mode == X.IN_ATTN_MERGE)
    claimed = set()
    for c in cs:
        claimed |= set(c.claims)
    assert set(X.ALL_COUNTS) | set(X.ROWS) | {"empty_wg", "idle_wave", "dead_unit", "ragged_last_pass", "stale_after_full", "three_below_max",
                                             "zero_next_to_16", "all_kept", "tau_tie", "tie_up", "tie_down"} <= claimed


def test_image_builder_agrees_with_the_packer():
    """the builder's packing (written from the header's layout text) equals teal_amd.quantize.pack_int4_colmajor"""
    from teal_amd.quantize import pack_int4_colmajor
    rng = np.random.default_rng(5)
    Q = rng.integers(0, 16, (96, 136))
    mine = X.pack_image(Q, 136 + 24)
    theirs = pack_int4_colmajor(torch.from_numpy(Q.T.copy()), pad_bytes=24).numpy()
    assert np.array_equal(mine[:, :136], theirs[:, :136]) and (mine[:, 136:] == 0xFF).all()
    # dword g of pair-row p: nibble j of the low half = column 4g + j of row 2p, of the high half = row 2p + 1
    w = mine[:, :136].copy().view("<u4")
    for p, g, j in ((0, 0, 0), (5, 7, 3), (47, 33, 2)):
        assert (int(w[p, g]) >> (4 * j)) & 15 == Q[2 * p, 4 * g + j] and (int(w[p, g]) >> (16 + 4 * j)) & 15 == Q[2 * p + 1, 4 * g + j]


def test_unit_rule_is_a_partition():
    """the documented unit rule: every unit in exactly one (slice, wave, j); a wave's j-th unit is slice + split (wave + 16 j)"""
    for Z in (32, 256, 544, 1056, 4096, 12288, 65536):
        for split in (1, 2, 4, 8):
            sl, wv, jj = X.unit_place(Z, split)
            assert np.array_equal(sl + split * (wv + 16 * jj), np.arange(Z // 32))
            assert sl.max() < split and wv.max() < 16


def test_desc_parser():
    g = X.parse_desc("sparse_gemv_int4_kernel<true,1,0,false> grid (2,8) x 1024")
    assert g == dict(kernel="int4", bf16=True, mode=1, kind=X.GROUP, phase=False, ntiles=2, split=8)
    g = X.parse_desc("sparse_gemv_int4_kernel<false,4,1,false> grid (86,2) x 1024")
    assert g["kind"] == X.SHARE and g["mode"] == 4 and not g["bf16"] and (g["ntiles"], g["split"]) == (86, 2)
    with pytest.raises(AssertionError):
        X.parse_desc("gemv_fast_kernel<true,1,false,8,4,true,false,4,false,true> grid (156,1) x 1024")
    c = CASES["share_counts_fp16"]
    with pytest.raises(AssertionError):   # another split than *nslabs_out
        X.geometry(c, "sparse_gemv_int4_kernel<false,0,1,false> grid (1,8) x 1024", 4)
