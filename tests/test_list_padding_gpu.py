"""GPU: a wave's row list rounded up to whole batches (teal_amd/csrc/teal_gemv_fast.h: list padding).  The lean GEMV kernel
appends (last kept row << 16 | +0.0) entries until the wave-local list is a multiple of STEP = 4 * (64 / LPR) and streams whole
batches only; the general kernel (teal_gemv_kernel.h) keeps its guarded tail batch.  A pad that carried a non-zero activation, a
pad that replaced the last real entry, a row streamed twice with its activation, or a pad past the list would each change a sum.

The launches go through tests/exact_gemv.py (cases, integer reference, ledger) and tests/test_exact_gemv_gpu.py (_launch, _run),
with the ACTIVATION PATTERN replaced: activations are 0 or +-1..+-3 against tau = 0.5, placed so that the 16 waves of a slice
keep 0, 1, STEP - 1, STEP, STEP + 1, 2 STEP - 1, 2 STEP, 63, 64 (and seven other counts) rows — every one of them in every
launch, on different waves for the two rotations.  The per-wave counts are asserted on the host from the inputs the launch gets,
before it is made.  Shapes: Z = 1024 (one chunk per wave, KR = 1 in the element-wise modes), Z = 2048 (split 2), N = 64 (LPR 8,
STEP 32) and N = 128 (LPR 16, STEP 16).  Waves that own four chunks (RESID_NORM at Z = 4096, the EXACT instantiation: Z =
1024 KR) keep six whole batches more (the exact RMSNorm needs the rows; the partial last batch is the same) and fill their chunks
from the first on, from the last on, or evenly — the last kept row comes from a chunk that is not the wave's last, the early
issue after the first chunk runs and does not run.  (RESID_NORM at Z = 1024 is KR = 4 with three absent chunks per wave, the
non-EXACT form; both run.)

  (a) integer reference: weights +-2^(row mod E) (E = 14; int8 E = 7), fp32 outputs, compared to the bit;
  (b) lean == general bit for bit on random weights and activations: interleaved slabs, and the TEAL_OUT_SLAB_SUM output against
      the fp32 slice-order sum of the general kernel's slabs;
  (c) int8, PAIR with two thresholds (gate keeps every non-zero row, up |x| >= 2: the pad's |0| > tau is false for both),
      RESID_NORM non-EXACT and EXACT, ATTN_MERGE;
  (d) a NaN activation in the last kept row of a wave (the row the pads repeat): the same words NaN, the same words finite and
      equal, in both kernels.
"""
import numpy as np
import pytest
import torch

import exact_gemv as X
import helpers
import test_exact_gemv_gpu as G
from teal_amd import runtime

pytestmark = pytest.mark.gpu
TAU = 0.5
ROTS = (0, 9)


def _counts(step):
    want = [0, 1, step - 1, step, step + 1, 2 * step - 1, 2 * step, 63, 64]
    return want, want + [2, step + 2, 5, step // 2, 3, 62, 7]


def _pattern(Z, split, mode, step, rot, rng, ones=0.0, bump=0):
    """u [Z] in {0, +-1, +-2, +-3} and {(slice, wave): rows kept}.  ones: share of the kept rows that carry +-1 (RESID_NORM: the
    mean square has to land on a power of 4); bump: whole batches added to every non-empty list of a wave that owns several
    chunks (the same partial last batch, and enough rows for the mean square)"""
    _, table = _counts(step)
    sl, wv = X.chunk_place(Z, split, mode)
    u, plan = np.zeros(Z), {}
    for s in range(split):
        for w in range(X.WAVES):
            ch = np.nonzero((sl == s) & (wv == w))[0]
            n = table[(w + rot + 5 * s) % 16]
            if n and len(ch) > 1:
                n += bump
            plan[(s, w)] = n
            if len(ch) == 1:
                share = [n]
            elif w % 3 == 2:     # spread over the wave's chunks
                share = [n // len(ch) + (1 if j < n % len(ch) else 0) for j in range(len(ch))]
            else:                # from the first chunk on (early issue; the last kept row is not in the last chunk) or from the last
                share, left = [], n
                for _ in ch:
                    share.append(min(left, 64))
                    left -= share[-1]
                if w % 3 == 1:
                    share = share[::-1]
            for c, m in zip(ch, share):
                if m == 1:
                    lanes = np.array([0 if (w + rot) % 2 == 0 else 63])   # clz 63 and clz 0 of the chunk's mask
                else:
                    lanes = rng.permutation(64)[:m]
                mag = np.where(rng.random(m) < ones, 1, rng.integers(1, 4, m))
                u[c * 64 + lanes] = mag * rng.choice([-1, 1], m)
    return u, plan


def _wave_counts(x, Z, split, mode):
    sl, wv = X.chunk_place(Z, split, mode)
    row_sl, row_wv = np.repeat(sl, 64)[:Z], np.repeat(wv, 64)[:Z]
    keep = ~(np.abs(x) <= TAU)   # (a NaN is kept)
    return {(s, w): int((keep & (row_sl == s) & (row_wv == w)).sum()) for s in range(split) for w in range(X.WAVES)}


def _assert_counts(x, Z, split, mode, step, plan, free=(), bump=0):
    """the inputs keep what the case was written for: the planned count on every wave (but `free`, the wave of the always-kept
    correction rows), and every size of the issue's list on some wave of every slice"""
    got = _wave_counts(x, Z, split, mode)
    for k, n in plan.items():
        assert k in free or got[k] == n, (k, got[k], n)
    want, _ = _counts(step)
    for s in range(split):
        have = {got[(s, w)] for w in range(X.WAVES) if (s, w) not in free}
        assert {n + bump if n else 0 for n in want} <= have, (s, sorted(set(want) - have))


def _pow2_rows(modulus):
    def weights(rng, Z, N):
        sign = rng.choice([-1.0, 1.0], (Z, N))
        return (sign * np.exp2(np.arange(Z) % modulus)[:, None]).astype(np.float32)
    return weights


# ---- (a), (c): the integer reference ------------------------------------------------------------------------------------------

def _exact_cases():
    C = {}
    for dt in ("fp16", "bf16"):
        for N, lpr in ((64, 8), (128, 16)):
            for rot in ROTS:
                C[f"z1024_n{N}_r{rot}_{dt}"] = (X.Case(f"pad_z1024_n{N}_r{rot}_{dt}", dt, 1024, out=X.OUT_SLAB_SUM, lib=(lpr, 1), segs=[(N, TAU)],
                                                       xmax=3, expect=dict(kernel="lean", lpr=lpr, split=1, kr=1, mode=0)), rot, 14)
                C[f"z2048_n{N}_split2_r{rot}_{dt}"] = (X.Case(f"pad_z2048_n{N}_split2_r{rot}_{dt}", dt, 2048, out=X.OUT_SLABS, lib=(lpr, 2),
                                                              segs=[(N, TAU)], xmax=3, expect=dict(kernel="lean", lpr=lpr, split=2, kr=1, mode=0)), rot, 14)
                C[f"z2048_n{N}_ticket_r{rot}_{dt}"] = (X.Case(f"pad_z2048_n{N}_ticket_r{rot}_{dt}", dt, 2048, out=X.OUT_SLAB_SUM, lib=(lpr, 2),
                                                              segs=[(N, TAU)], xmax=3, expect=dict(kernel="lean", lpr=lpr, split=2, kr=1, mode=0)), rot, 14)
        for rot in ROTS:
            C[f"w8_z1024_r{rot}_{dt}"] = (X.Case(f"pad_w8_z1024_r{rot}_{dt}", dt, 1024, w8=True, out=X.OUT_SLAB_SUM, lib=(16, 1), segs=[(128, TAU)],
                                                 xmax=3, expect=dict(kernel="lean", lpr=16, split=1, kr=1, w8=True)), rot, 7)
        C[f"w8_z2048_split2_{dt}"] = (X.Case(f"pad_w8_z2048_split2_{dt}", dt, 2048, w8=True, out=X.OUT_SLABS, lib=(16, 2), segs=[(128, TAU)],
                                             xmax=3, expect=dict(kernel="lean", lpr=16, split=2, kr=1, w8=True)), 9, 7)
        # PAIR: the keep sets differ (gate: every non-zero row; up: |x| >= 2), exact_gemv's own weights with steered sums
        C[f"pair_two_tau_{dt}"] = (X.Case(f"pad_pair_two_tau_{dt}", dt, 1024, mode=X.IN_RESID_NORM, out=X.OUT_PAIR_SILU, lib=(8, 1),
                                          segs=[(128, TAU), (128, 1.5)], steer=True, nw_kind="sign", xmax=3,
                                          expect=dict(kernel="lean", lpr=8, split=1, kr=4, pair=True, exact=False)), 0, None)
        C[f"norm_z1024_{dt}"] = (X.Case(f"pad_norm_z1024_{dt}", dt, 1024, mode=X.IN_RESID_NORM, out=X.OUT_SLABS, lib=(8, 1), segs=[(64, TAU)],
                                        nw_kind="sign", xmax=3, expect=dict(kernel="lean", lpr=8, split=1, kr=4, mode=1, exact=False)), 9, 14)
        C[f"norm_z4096_exact_{dt}"] = (X.Case(f"pad_norm_z4096_exact_{dt}", dt, 4096, mode=X.IN_RESID_NORM, out=X.OUT_SLABS, lib=(16, 1),
                                              segs=[(128, TAU)], nw_kind="sign", xmax=3,
                                              expect=dict(kernel="lean", lpr=16, split=1, kr=4, mode=1, exact=True)), 0, 14)
        C[f"attn_merge_{dt}"] = (X.Case(f"pad_attn_merge_{dt}", dt, 1024, mode=X.IN_ATTN_MERGE, att_ns=4, att_hd=64, out=X.OUT_SLAB_SUM, lib=(8, 1),
                                        segs=[(64, TAU)], xmax=3, expect=dict(kernel="lean", lpr=8, split=1, kr=1, mode=4)), 9, 14)
    return C


EXACT = _exact_cases()


def _patch(monkeypatch, c, rot, modulus, seen):
    """exact_gemv's builders with the activation pattern of this file"""
    lpr, split = c.lib
    step = 4 * (64 // lpr)
    bump = 6 * step if c.Z > 1024 * split else 0   # waves that own four chunks

    def layout(cc, rng, geo):
        u, plan = _pattern(cc.Z, split, cc.mode, step, rot, rng, ones=0.7 if (cc.mode == X.IN_RESID_NORM and not cc.steer) else 0.0,
                           bump=bump)
        seen["plan"] = plan
        return u, False

    def fix_sumsq(h, free, classes, target, rng, _f=X._fix_sumsq):
        return _f(h, free, [(0,), (1, 2, 3)], target, rng)   # zeros stay zeros: the per-wave counts are the layout's

    def build_attn(cc, b, rng):
        # split 0 carries the pattern with weight exp(0) / 1 = 1, split 1 is empty (sum 0, o = NaN), splits 2 and 3 underflow
        u, plan = _pattern(cc.Z, split, cc.mode, step, rot, rng)
        seen["plan"] = plan
        hd, ns = cc.att_hd, cc.att_ns
        H = cc.Z // hd
        part = np.zeros((H, ns, hd + 2))
        part[:, 0, 0], part[:, 0, 1], part[:, 0, 2:] = 0.0, 1.0, u.reshape(H, hd)
        part[:, 1, 0], part[:, 1, 1], part[:, 1, 2:] = -np.inf, 0.0, np.nan
        part[:, 2:, 0], part[:, 2:, 1] = -200.0, 3.0
        part[:, 2:, 2:] = rng.integers(-4, 5, (H, ns - 2, hd))
        stats = [(1, [0], 1.0)] * H
        b.meta["part"], b.meta["stats"] = part, stats
        b.inputs["x"] = torch.from_numpy(part.reshape(-1)).float()
        return X._attn_x(cc, part, stats, None)

    monkeypatch.setattr(X, "_layout_u", layout)
    monkeypatch.setattr(X, "_fix_sumsq", fix_sumsq)
    monkeypatch.setattr(X, "_build_attn", build_attn)
    if modulus is not None:
        monkeypatch.setattr(X, "_weights", _pow2_rows(modulus))
    # (exact_gemv.build takes a "random" layout's geometry from nowhere but the launch's report)
    monkeypatch.setattr(X, "geometry", lambda cc, desc=None, ns=None, _g=X.geometry: _g(cc, desc, ns) if desc is not None else
                        dict(kernel="lean", lpr=lpr, split=split, kr=None, exact=False, rope=False, w8=cc.w8, pair=cc.pair, mode=cc.mode))

    def build(cc, geo=None, _b=X.build):
        b = _b(cc, geo)
        assert set(np.unique(np.abs(b.x))) <= {0.0, 1.0, 2.0, 3.0, 4.0} and b.taus[0] == TAU
        free = {(0, X.WAVES - 1)} if cc.steer else ()   # the correction rows Z - 2, Z - 1 (x = 4, 3) sit in the last wave's chunk
        _assert_counts(b.x, cc.Z, split, cc.mode, step, seen["plan"], free, bump)
        seen["checked"] = True
        return b

    monkeypatch.setattr(X, "build", build)


@pytest.mark.parametrize("name", list(EXACT))
def test_padded_lists_match_the_integer_reference(name, monkeypatch):
    c, rot, modulus = EXACT[name]
    seen = {}
    _patch(monkeypatch, c, rot, modulus, seen)
    led, n, desc = G._run(c)
    assert seen.get("checked") and n > 0
    print("\n" + X.probe_line(c, led, n))
    print(f"LEDGER {c.name}: {desc}")


# ---- (b), (d): lean against general on random numbers --------------------------------------------------------------------------

def _random_built(dt, Z, N, split, lpr, rot, seed):
    rng = np.random.default_rng(seed)
    step = 4 * (64 // lpr)
    u, plan = _pattern(Z, split, X.IN_PLAIN, step, rot, rng)
    keep = u != 0
    # kept rows |x| in [0.6, 3], dropped rows exactly 0 or |x| <= 0.4: no 16-bit rounding crosses tau = 0.5
    mag = np.where(keep, rng.uniform(0.6, 3.0, Z), np.where(rng.random(Z) < 0.5, 0.0, rng.uniform(0.0, 0.4, Z)))
    x = torch.from_numpy(mag * np.where(u < 0, -1.0, 1.0)).to(X.TDT[dt])
    b = X.Built()
    b.ld = [N + 64]
    b.images_t = [torch.from_numpy(rng.standard_normal((Z, N + 64)) * 0.05).to(X.TDT[dt])]
    b.scale_t, b.seg_img, b.taus, b.inputs = None, [(0, 0, N)], [TAU], {"x": x}
    return b, plan, step


def _both(dt, Z, N, split, lpr, b, out):
    """the same launch through the lean and the general kernel -> {fast: slab words}"""
    res = {}
    for fast in (1, 0):
        c = X.Case(f"pad_random_{fast}", dt, Z, out=out, lib=(lpr, split), fast=fast, segs=[(N, TAU)])
        with helpers.lib_for(fast=fast, tuning=(lpr, 0, split, 0)) as L:
            runtime.init()
            ws = runtime.new_workspace(Z, N)
            geo, got, desc = G._launch(L, c, b, ws)
            del ws
        assert geo["kernel"] == ("lean" if fast else "general") and geo["lpr"] == lpr and geo["split"] == split, desc
        res[fast] = got["slabs"]
    return res


def _fold32(slabs, N, split):
    """fp32 sum of the interleaved slabs in slice order, from +0.0: what the last slice of a TEAL_OUT_SLAB_SUM launch computes"""
    st = (split + 3) & ~3
    v = slabs[: N * st].view(np.float32).reshape(N, st)
    acc = np.zeros(N, np.float32)
    for k in range(split):
        acc = acc + v[:, k]
    return acc


def _same_words(a, b):
    """bit for bit; a NaN equals any NaN (the two kernels' NaN payloads are not part of the contract)"""
    fa, fb = a.view(np.float32), b.view(np.float32)
    na, nb = np.isnan(fa), np.isnan(fb)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


RANDOM = [(dt, Z, N, lpr, split, rot) for dt in ("fp16", "bf16") for N, lpr in ((64, 8), (128, 16)) for Z, split, rot in ((1024, 1, 0), (2048, 2, 9))]


@pytest.mark.parametrize("dt,Z,N,lpr,split,rot", RANDOM, ids=[f"{c[0]}_z{c[1]}_n{c[2]}_split{c[4]}" for c in RANDOM])
def test_lean_equals_general_on_random_numbers(dt, Z, N, lpr, split, rot):
    b, plan, step = _random_built(dt, Z, N, split, lpr, rot, seed=Z + N)
    _assert_counts(b.inputs["x"].double().numpy(), Z, split, X.IN_PLAIN, step, plan)
    slabs = _both(dt, Z, N, split, lpr, b, X.OUT_SLABS)
    assert not np.isnan(_fold32(slabs[0], N, split)).any()
    assert np.array_equal(slabs[1], slabs[0]), f"{int((slabs[1] != slabs[0]).sum())} slab words differ between the lean and the general kernel"
    c = X.Case("pad_random_sum", dt, Z, out=X.OUT_SLAB_SUM, lib=(lpr, split), segs=[(N, TAU)])
    with helpers.lib_for(fast=1, tuning=(lpr, 0, split, 0)) as L:
        runtime.init()
        ws = runtime.new_workspace(Z, N)
        geo, got, desc = G._launch(L, c, b, ws)
        del ws
    assert geo["kernel"] == "lean" and geo["split"] == split, desc
    want = _fold32(slabs[0], N, split)
    assert np.array_equal(got["slabs"][:N], want.view(np.int32)), "TEAL_OUT_SLAB_SUM differs from the slice-order sum of the general kernel's slabs"
    assert (got["slabs"][N:] == X.SENT32_I).all()


@pytest.mark.parametrize("dt", ("fp16", "bf16"))
@pytest.mark.parametrize("N,lpr", ((64, 8), (128, 16)))
def test_nan_in_a_wave_s_last_kept_row(dt, N, lpr):
    """the row the pads repeat carries NaN: its NaN reaches the sums once, through its own entry, as in the general kernel — slice
    0's slab is NaN in every column, slice 1's in none, and the finite words are equal"""
    Z, split = 2048, 2
    step = 4 * (64 // lpr)
    for n in (1, step, step + 1):
        b, plan, _ = _random_built(dt, Z, N, split, lpr, 9, seed=7 * n + N)
        x = b.inputs["x"].double().numpy()
        sl, wv = X.chunk_place(Z, split, X.IN_PLAIN)
        w = next(w for w in range(X.WAVES) if plan[(0, w)] == n)
        rows = np.nonzero(np.repeat((sl == 0) & (wv == w), 64) & (np.abs(x) > TAU))[0]
        assert len(rows) == n
        x[rows[-1]] = np.nan
        b.inputs["x"] = torch.from_numpy(x).to(X.TDT[dt])
        _assert_counts(x, Z, split, X.IN_PLAIN, step, plan)
        slabs = _both(dt, Z, N, split, lpr, b, X.OUT_SLABS)
        st = (split + 3) & ~3
        lean = slabs[1][: N * st].view(np.float32).reshape(N, st)
        assert np.isnan(lean[:, 0]).all() and not np.isnan(lean[:, 1]).any(), (n, w)
        assert _same_words(slabs[1][: N * st], slabs[0][: N * st]) and np.array_equal(slabs[1][N * st:], slabs[0][N * st:]), (n, w)
