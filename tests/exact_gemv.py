"""Exact-integer probes of the fused decode GEMV, teal_fused_gemv (not a test file): case builders, the integer reference,
the ledger and the mutants.  Shared by tests/test_exact_gemv_host.py (CPU: the probes' own power) and
tests/test_exact_gemv_gpu.py (the HIP launches through the C ABI).

tests/exact_gemm.py's principle applied to ONE activation vector: fed small integers, every fp32 partial sum of the GEMV is
exact in any order, so every output word must equal an integer reference BIT FOR BIT.

  * activations are integers in [-4, 4] (times a power of two where a producer scales them), weights NON-ZERO integers in
    [-3, 3]; sum |w| |x| per (slice, column), in units of the inputs' granularity, is asserted below 2^24.  int8 weights: the
    kernels accumulate (q + 1152) x and subtract 1152 sum x (kInt8Bias), so sum |q + 1152| |x| and 1152 sum |x| are asserted
    below 2^24 as well; the scales are powers of two;
  * RESID_NORM: integer residual and slabs, a sum of squares whose mean is an exact power of 4 (eps 0: h * rstd is a grid value
    whatever rsqrtf's last bit is; every h * rstd asserted 2^-12 away from a rounding tie), norm weights +-{1/2, 1, 2} or a
    small integer.  eps = 1e-5 only in the case whose reference shows that the 16-bit rounding absorbs it;
  * SILU_MUL: gates in {16, 24, 32}, where fp32 silu rounds to the gate itself (asserted to a quarter ulp in fp64); with
    gate_activated = 1 the gate half holds small integers instead, on which a second silu would show;
  * ATTN_MERGE: max - M in {0, -200} (expf gives exactly 1 or 0), sums are powers of two whose kept total is a power of two,
    o holds integers, one split per head is empty (sum 0, o = NaN);
  * act_seg0 / PAIR_SILU: the gate sums are steered onto {16, 24, 32} and the up sums onto small non-zero integers by the
    weights of always-kept correction rows, so h = round16(g * u) is an integer computation;
  * QKV_ROPE: a (cos, sin) table of {(1,0), (0,1), (-1,0), (1/2,1/2), (0,-1)} per (position, pair);
  * poison: the ld - N padding columns and, per (row, segment), the weights of rows the segment does not keep hold NaN (both
    kernels load listed rows only; their tail batch re-reads the last LISTED row) — int8 images cannot hold NaN and carry
    +127 / -128 there; sentinel words sit behind every output, in the slab padding lanes and in the slabs no slice writes.

The reference takes lanes-per-row, split and the kernel from what the launch REPORTED (*nslabs_out, teal_gemv_out.desc) and
never re-derives the host's geometry choice.  The chunk-to-slice rule it uses is the one include/teal_hip.h documents next
to TEAL_OUT_SLABS.  `ledger` classifies what a case executed; every case asserts the classes it was written for.  MUTANTS
are switches of the reference / of the numpy model of the per-wave row walk; tests/test_exact_gemv_host.py shows that each one
changes a compared word of at least one case.
"""
import math
import re

import numpy as np
import torch

from exact_gemm import (CODE, PBITS, POISON, SENT16_I, SENT32_I, TDT, TIE_LO, bits16, bits32, first_diff, rne16,  # noqa: F401
                        sum_slices_f32)

IN_PLAIN, IN_RESID_NORM, IN_SILU_MUL, IN_MASKED, IN_ATTN_MERGE = 0, 1, 2, 3, 4
OUT_ROUNDED, OUT_SLABS, OUT_PAIR_SILU, OUT_QKV_ROPE, OUT_SLAB_SUM = 0, 1, 2, 3, 4
IN_NAME = {0: "plain", 1: "resid_norm", 2: "silu_mul", 3: "masked", 4: "attn_merge"}
OUT_NAME = {0: "rounded", 1: "slabs", 2: "pair_silu", 3: "qkv_rope", 4: "slab_sum"}
WAVES = 16
SENT64_I = np.int64(0x5A5A5A5A5A5A5A5A)
TAIL = 64                       # sentinel words behind every output
MAX_SLABS = 32
ROPE_PAT = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.5, 0.5), (0.0, -1.0))
GATES = (16.0, 24.0, 32.0)
INT8_BIAS = 1152.0

MUTANTS = (
    "ge",                  # >= where > belongs
    "drop_last",           # last listed row of a wave dropped
    "tail_dup",            # the tail batch's clamped lanes not zeroed: the last row is doubled
    "skip_set_b",          # a wave's second register set skipped
    "seg_tau",             # wrong threshold for the first tile of segment 1 or 2
    "pair_tau",            # the gate's threshold used for up under PAIR
    "image2_col",          # second image read at the first image's column
    "slabs_reverse",       # slabs summed in reverse (the launch's own fold and the RESID_NORM consumer's sum)
    "slab_sum_twice",      # a double rounding of the slab sum
    "resid_before_round",  # residual added before the slab sum is rounded
    "normw_before_round",  # norm weight applied before the 16-bit rounding of h * rstd
    "up_offset0",          # `up` read at offset 0 instead of Z
    "gate_act_ignored",    # gate_activated ignored
    "empty_split",         # an empty split not ignored in the merge
    "head_off_by_one",     # head index off by one
    "rope_swap",           # the RoPE pair swapped
    "rope_sin_sign",       # the sine's sign flipped
    "v_rotated",           # v rotated
    "k_row_pos1",          # the k row written at pos + 1
    "int8_bias_all",       # int8 bias taken over all rows instead of the kept ones
)


class Case:
    """One teal_fused_gemv launch.  segs: [(ncols, tau)]; images 2: segment 1 lives in an image of its own (gate | up
    unpaired; PAIR always has two).  lib: None = the product library, else (lanes_per_row, split) forced through the
    diagnostics build; fast 0 forces the general kernel.  expect: what the launch must report (kernel, lpr, split, kr ...),
    asserted through the ledger; the "sizes" and "order" layouts are built for expect's geometry."""

    def __init__(self, name, dt, Z, mode=IN_PLAIN, out=OUT_ROUNDED, segs=((128, 1.0),), images=1, w8=False, lib=None, fast=1,
                 prepared=True, layout="random", expect=None, claims=(), mutants=(), seed=1, xmax=4, nslabs=0, slabs_il=1,
                 eps=0.0, row_index=False, nw_kind="pow2", resid_out=True, gate_activated=0, att_ns=4, att_hd=64, act_seg0=0,
                 il=1, rope=None, steer=False, probe_rounding=False, att_empty=True):
        self.name, self.dt, self.Z, self.mode, self.out = name, dt, Z, mode, out
        self.segs = [(int(n), float(t)) for n, t in segs]
        self.images, self.w8, self.lib, self.fast, self.prepared, self.layout = images, w8, lib, fast, prepared, layout
        self.expect = dict(expect or {})
        self.claims, self.mutants, self.seed, self.xmax = tuple(claims), tuple(mutants), seed, xmax
        self.nslabs, self.slabs_il, self.eps, self.row_index, self.nw_kind, self.resid_out = nslabs, slabs_il, eps, row_index, nw_kind, resid_out
        self.gate_activated, self.att_ns, self.att_hd, self.act_seg0 = gate_activated, att_ns, att_hd, act_seg0
        self.il, self.rope, self.steer, self.probe_rounding = il, rope, steer, probe_rounding
        self.att_empty = att_empty
        self.pair = out == OUT_PAIR_SILU
        self.N = self.segs[0][0] if self.pair else sum(n for n, _ in self.segs)
        assert Z % 64 == 0 or self.fast == 0

    def __repr__(self):
        return self.name


class Built:
    pass


# ---- geometry the header documents ------------------------------------------------------------------------------------------

def rounds_of(Z):
    return ((Z + 63) // 64 + WAVES - 1) // WAVES


def chunk_place(Z, split, mode):
    """per 64-element chunk c: (slice, wave) — include/teal_hip.h, TEAL_OUT_SLABS.  Element-wise producers: chunk c belongs to
    slice c mod split and, inside it, to wave (c div split) mod 16.  RESID_NORM: chunk w + 16 k belongs to wave w and to slice
    (k + w) mod split."""
    c = np.arange((Z + 63) // 64)
    if mode == IN_RESID_NORM:
        w, k = c % WAVES, c // WAVES
        return (k + w) % split, w
    return c % split, (c // split) % WAVES


def wave_local(Z, split, mode):
    """does the rule above apply (split <= the vector's rounds of 16 chunks, a slice's rounds fit the register cache and its
    lists the LDS), or does the general kernel cut ONE ascending list of the kept rows into `split` even shares"""
    owned = rounds_of(Z)
    sl = mode != IN_RESID_NORM and split > 1
    need = (owned + split - 1) // split if sl else owned
    krt = 4 if need <= 4 else (8 if need <= 8 else 16)
    capw = (need if sl else (krt + split - 1) // split) * 64
    return need <= krt and split <= owned and WAVES * capw * 4 <= 40 * 1024


def parse_desc(desc):
    """teal_gemv_out.desc -> {kernel, bf16, mode, pair, lpr, kr, exact, w8, rope, ntiles, split (lean only)}"""
    m = re.match(r"gemv_fast_kernel<(\w+),(\d+),(\w+),(\d+),(\d+),(\w+),(\w+),4,(\w+),(\w+)> grid \((\d+),(\d+)\) x 1024", desc)
    if m:
        g = m.groups()
        return dict(kernel="lean", bf16=g[0] == "true", mode=int(g[1]), pair=g[2] == "true", lpr=int(g[3]), kr=int(g[4]),
                    exact=g[5] == "true", w8=g[7] == "true", rope=g[8] == "true", ntiles=int(g[9]), split=int(g[10]))
    m = re.match(r"sparse_gemv_kernel<(\d+),(\d+),(\d+),(\w+),(\d+),(\d+),(\w+),(\w+)> grid (\d+) x (\d+)", desc)
    assert m, desc
    g = m.groups()
    return dict(kernel="general", lpr=int(g[0]), bf16=g[3] == "true", mode=int(g[4]), kr=int(g[5]), pair=g[6] == "true",
                w8=g[7] == "true", rope=False, exact=False, workgroups=int(g[8]))


def geometry(c, desc=None, nslabs_out=None):
    """the geometry the reference runs at: from the launch's own report, or (host tests) from the case's expectation"""
    if desc is None:
        e = c.expect
        return dict(kernel=e["kernel"], lpr=e["lpr"], split=e["split"], kr=e.get("kr"), exact=e.get("exact", False),
                    rope=e.get("rope", False), w8=c.w8, pair=c.pair, mode=c.mode)
    g = parse_desc(desc)
    if g["kernel"] == "lean":
        if nslabs_out is not None and c.out == OUT_SLABS:
            assert nslabs_out == g["split"], (desc, nslabs_out)
    else:
        cols = sum(n for n, _ in c.segs[: 1 if c.pair else None])
        tiles = sum((n + g["lpr"] * 8 - 1) // (g["lpr"] * 8) for n, _ in c.segs[: 1 if c.pair else None])
        assert cols and g["workgroups"] % tiles == 0, desc
        g["split"] = g["workgroups"] // tiles
        if nslabs_out is not None and c.out == OUT_SLABS:
            assert nslabs_out == g["split"], (desc, nslabs_out)
    return g


# ---- builders ---------------------------------------------------------------------------------------------------------------

def _weights(rng, Z, N):
    return (rng.integers(1, 4, (Z, N)) * rng.choice([-1, 1], (Z, N))).astype(np.float32)


def _fix_sumsq(h, free, classes, target, rng):
    """change free entries of the integer vector h inside their own magnitude class until sum h^2 == target"""
    h = h.copy()
    idx = np.nonzero(free)[0]
    cls_of = {}
    for cl in classes:
        for v in cl:
            cls_of[v] = cl
    diff = int(target - (h * h).sum())
    it = 0
    while diff != 0:
        it += 1
        assert it < 200000, "sum of squares not reachable"
        i = idx[rng.integers(0, len(idx))]
        a = int(abs(h[i]))
        cand = cls_of[a]
        best = min(cand, key=lambda v: abs(diff - (v * v - a * a)))
        if abs(diff - (best * best - a * a)) < abs(diff) or (it % 7 == 0 and len(cand) > 1):
            if not abs(diff - (best * best - a * a)) < abs(diff):
                best = cand[rng.integers(0, len(cand))]
            sign = -1.0 if h[i] < 0 else 1.0
            h[i] = sign * best
            diff -= best * best - a * a
    return h


def _layout_u(c, rng, geo):
    """the integer vector u in [-xmax, xmax] the producer is asked to deliver (times its scale), and whether row classes
    (|u| <= 1 dropped, |u| >= 2 kept at tau = 1 unit) are prescribed"""
    Z = c.Z
    if c.layout == "random":
        return rng.integers(-c.xmax, c.xmax + 1, Z).astype(np.float64), False
    if c.layout == "order":
        # slice-order probe: slice 0's partial is 2^24 (x = w = 2^12), the last slice's -2^24 when the output is rounded to 16
        # bits (a 16-bit word cannot tell 2^24 from 2^24 + 2), every other slice's 1
        return np.zeros(Z), True
    assert c.layout == "sizes"
    split, lpr = geo["split"], geo["lpr"]
    step = 4 * (64 // lpr)
    sl, wv = chunk_place(Z, split, c.mode)
    u = rng.choice([0.0, 1.0, -1.0], Z)
    for s in range(split):
        for w in range(WAVES):
            ch = np.nonzero((sl == s) & (wv == w))[0]
            rows = (ch[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
            want = [0, 1, step - 1, step, step + 1, 2 * step - 1, 2 * step, 2 * step + 1, 3 * step, len(rows), 3 * step + 1, step + 2,
                    2 * step + 3, 5, step, 4 * step][(w + 5 * s) % 16]
            n = min(want, len(rows))
            if s == split - 1 and split > 1 and "emptywg" in c.name:
                n = 0   # a workgroup that keeps nothing
            if n == 0:
                continue
            cap0 = min(64, len(rows))
            # even waves fill their first chunk first (>= STEP kept rows there: the early-issue path), odd waves keep it
            # below STEP while the wave's total reaches it
            f = min(n, cap0) if w % 2 == 0 else min(n, step - 1)
            f = min(max(f, n - (len(rows) - cap0)), cap0)
            pick = rows[:cap0][rng.permutation(cap0)[:f]]
            if n > f:
                pick = np.concatenate([pick, rows[cap0:][rng.permutation(len(rows) - cap0)[: n - f]]])
            u[pick] = rng.integers(2, c.xmax + 1, len(pick)) * rng.choice([-1, 1], len(pick))
    return u, True


def build(c, geo=None):
    """inputs (CPU torch tensors, poison included) of case c.  geo: the launch geometry a "sizes" / "order" layout is built
    for (default: the case's expectation)."""
    geo = geo or geometry(c)
    rng = np.random.default_rng(c.seed * 7919 + 13)
    b = Built()
    b.case, b.geo_built = c, dict(geo)
    Z, dt = c.Z, c.dt
    b.inputs, b.meta = {}, {}
    u, classed = _layout_u(c, rng, geo)
    unit = 1.0
    corr = []   # always-kept correction rows (steered sums)
    if c.steer:
        npairs = 4 if c.w8 else 1
        corr = list(range(Z - 2 * npairs, Z))
        for j, r in enumerate(corr):
            u[r] = 4.0 if j % 2 == 0 else 3.0
    if c.layout == "order":
        split = geo["split"]
        sl, _ = chunk_place(Z, split, c.mode)
        assert split >= 3 and wave_local(Z, split, c.mode)
        b.order_rows = [int(np.nonzero(sl == s)[0][0]) * 64 + 5 * s for s in range(split)]
        for s, r in enumerate(b.order_rows):
            u[r] = 4096.0 if s == 0 else (-4096.0 if (s == split - 1 and c.out != OUT_SLAB_SUM and c.out != OUT_SLABS) else 1.0)

    # ---- the producer's inputs and the activation vector x it must deliver (float64, numbers of dt's grid) ----
    if c.mode in (IN_PLAIN, IN_MASKED):
        x = u.copy()
        b.inputs["x"] = torch.from_numpy(x).to(TDT[dt])
    elif c.mode == IN_SILU_MUL:
        for gv in GATES:  # fp32 silu rounds to the gate itself: a quarter of a 16-bit ulp in fp64
            assert abs(gv / (1.0 + math.exp(-gv)) - gv) < 0.25 * gv * 2.0 ** -PBITS[dt]
        if c.gate_activated:
            g = rng.choice([1.0, 2.0, -1.0, -2.0, 3.0], Z)       # already activated: any 16-bit number; silu again would show
            if classed:
                g = np.full(Z, 2.0)
        else:
            g = np.full(Z, 16.0) if classed else rng.choice(GATES, Z)
        unit = abs(g[0]) if classed else 1.0
        x = g * u
        b.meta["gate"], b.meta["up"] = g, u
        b.inputs["x"] = torch.from_numpy(np.concatenate([g, u])).to(TDT[dt])
    elif c.mode == IN_RESID_NORM:
        x = _build_resid_norm(c, b, u, classed, corr, rng)
        unit = b.meta["unit"]
    else:
        x = _build_attn(c, b, rng)
    b.x = x + 0.0
    b.unit = unit
    bits16(b.x, dt)   # (asserts that x is made of numbers of dt)
    b.taus = [unit * 1.0 if c.layout == "sizes" else (0.5 if c.layout == "order" else t) for _, t in c.segs]
    if c.mode == IN_MASKED:  # the masks are those of tau[0] (the header's contract); x carries values the compare would treat
        keep0 = _keep(x, b.taus[0])  # the same: the kernel must take the masks, not x
        words = np.zeros((Z + 63) // 64, np.uint64)
        for m in np.nonzero(keep0)[0]:
            words[m >> 6] |= np.uint64(1) << np.uint64(m & 63)
        b.inputs["masks"] = torch.from_numpy(words.view(np.int64).copy())
        b.meta["keep0"] = keep0
    b.corr = corr
    _build_weights(c, b, rng, geo)
    if c.out == OUT_QKV_ROPE:
        _build_rope(c, b, rng)
    return b


def _keep(x, tau, ge=False):
    a, t = np.abs(x).astype(np.float32), np.float32(tau)
    return (a >= t) if ge else (a > t)


def _build_resid_norm(c, b, u, classed, corr, rng):
    Z, dt = c.Z, c.dt
    ns = c.nslabs
    if c.eps > 0:
        # mean square 1 and eps = 1e-5: rstd = 1 - 5e-6, absorbed by the rounding of h * rstd for these h (no powers of two:
        # h * rstd would sit just below them, less than 2^-12 above the tie in fp16).  One row carries g with g * nw an exact
        # 16-bit tie that rounds UP: applying the norm weight before the rounding of h * rstd lands below the tie instead.
        g0, w0 = (71.0, 29.0) if dt == "fp16" else (37.0, 7.0)
        rest = Z - int(g0 * g0) - 3 * 36 - 3 * 49
        n5 = next(n for n in range(3, 12) if (rest - 25 * n) % 9 == 0)
        vals = [6.0] * 3 + [7.0] * 3 + [5.0] * n5 + [3.0] * ((rest - 25 * n5) // 9)
        h = np.zeros(Z)
        where = 8 + rng.permutation(Z - 8)[: len(vals)]
        h[where] = np.array(vals) * rng.choice([-1, 1], len(vals))
        h[7] = g0
        ms = 1.0
        nw = rng.choice([1.0, -1.0, 2.0, -2.0], Z)
        nw[7] = w0
        b.meta["tie_row"] = 7
    else:
        assert c.layout != "order"
        h = u.copy()
        free = np.ones(Z, bool)
        free[corr] = False
        if c.probe_rounding:   # (the residual of row 3 is h - TIE_LO - 2: a number of dt only for even h)
            h[3] = 2.0
            free[[3, 11]] = False
        s0 = float((h * h).sum())
        # the mean square: the power of 4 nearest to what the layout gives
        ms = min((4.0 ** j for j in range(0, 3)), key=lambda m: abs(math.log(max(s0, 1.0) / (m * Z))))
        h = _fix_sumsq(h, free, [(0, 1), tuple(range(2, c.xmax + 1))] if classed else [tuple(range(0, c.xmax + 1))], ms * Z, rng)
        if c.nw_kind == "sign" or classed:
            nw = rng.choice([1.0, -1.0], Z)
        else:
            nw = rng.choice([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], Z)
    h = h + 0.0   # (no -0.0: with no slabs the kernels hand the residual's own bits on)
    rstd = 1.0 / math.sqrt(ms)
    assert math.log2(rstd) == round(math.log2(rstd)) and (h * h).sum() == ms * Z and ms * Z < 2 ** 24
    if c.steer:      # integer x everywhere: the correction weights that steer the sums are integers then
        nw = np.where(nw < 0, -1.0, 1.0) / rstd
    for r in corr:   # x = h on the correction rows
        nw[r] = 1.0 / rstd
    # h = resid + round16(sum of the slabs in slab order)
    S = np.zeros((ns, Z))
    if ns:
        S = rng.integers(-2, 3, (ns, Z)).astype(np.float64)
        if c.probe_rounding and ns >= 3:
            T = float(TIE_LO[dt])
            assert c.eps == 0
            # a slab sum T + 1.25 rounds to T + 2, through one extra bit to T; resid + (T + 1.25) rounds otherwise as well
            S[:, 3] = 0.0
            S[0, 3], S[1, 3], S[2, 3] = T, 1.0, 0.25
            # a slab sum whose order shows: (2^24 + 1) - 2^24 = 0 in slab order, 1 in reverse
            S[:, 11] = 0.0
            S[0, 11], S[1, 11], S[ns - 1, 11] = 2.0 ** 24, 1.0, -(2.0 ** 24)
    ysum = sum_slices_f32(S) if ns else np.zeros(Z)
    y16 = rne16(np.where(ysum == 0, 0.0, ysum), dt) if ns else ysum
    resid = h - y16
    b.meta.update(h=h, rstd=rstd, nw=nw, S=S, resid=resid, ms=ms, unit=rstd)
    assert np.array_equal(rne16(np.where(resid + y16 == 0, 0.0, resid + y16), dt), h)
    r_eps = 1.0 / math.sqrt(ms + float(np.float32(c.eps)))
    v = h * r_eps
    grid = h * rstd
    for f in (1 - 2.0 ** -12, 1 + 2.0 ** -12):  # h * rstd(eps) rounds to h * 2^k with 2^-12 (relative) to spare either way
        assert np.array_equal(rne16(np.where(v != 0, v * f, 0.0), dt), grid), "h * rstd too close to a rounding tie"
    prod = grid * nw
    x = rne16(np.where(prod == 0, 0.0, prod), dt)
    if c.eps == 0:
        assert np.array_equal(x, prod)
    rows = 3 if c.row_index else 1
    table = np.full((rows, Z), math.nan)
    table[rows - 1] = resid
    b.inputs["resid"] = torch.from_numpy(table.reshape(-1)).to(TDT[dt])
    if c.row_index:
        b.inputs["row_index"] = torch.tensor([rows - 1], dtype=torch.int32)
    b.inputs["norm_w"] = torch.from_numpy(nw).to(TDT[dt])
    if ns:
        if c.slabs_il:
            st = (ns + 3) & ~3
            il = np.full((Z, st), math.nan)    # the padding lanes are loaded with the rest of the 16 bytes and must not count
            il[:, :ns] = S.T
            b.inputs["slabs_in"] = torch.from_numpy(il.reshape(-1)).float()
        else:
            b.inputs["slabs_in"] = torch.from_numpy(S.reshape(-1)).float()
    return x


def _build_attn(c, b, rng):
    Z, hd, ns = c.Z, c.att_hd, c.att_ns
    H = Z // hd
    part = np.zeros((H, ns, hd + 2))
    stats = []
    for h in range(H):
        order = rng.permutation(ns)
        empty = int(order[0]) if c.att_empty else -1   # (att_empty False: every split contributes or underflows)
        nA = (1, 2, 3)[h % 3] if ns > 3 else 1
        A = [int(q) for q in order[1: 1 + nA]]
        a = float(2 ** (h % 3))
        sums = {1: [a], 2: [a, a], 3: [2 * a, a, a]}[nA]
        if not c.att_empty:   # every split at the maximum with equal sums: every weight is 1 / (ns a) > 0
            A, sums = [int(q) for q in order], [a] * ns
        M = float(rng.integers(-3, 9))
        L = sum(sums)
        assert math.log2(L) == round(math.log2(L))
        for q in range(ns):
            o = rng.integers(-4, 5, hd).astype(np.float64)
            if q == empty:
                part[h, q, 0], part[h, q, 1], part[h, q, 2:] = -math.inf, 0.0, math.nan
            elif q in A:
                part[h, q, 0], part[h, q, 1], part[h, q, 2:] = M, sums[A.index(q)], o
            else:
                part[h, q, 0], part[h, q, 1], part[h, q, 2:] = M - 200.0, 3.0, o
        stats.append((empty, A, L))
    assert float(np.exp(np.float32(-200.0))) == 0.0
    b.meta["part"], b.meta["stats"] = part, stats
    b.inputs["x"] = torch.from_numpy(part.reshape(-1)).float()
    return _attn_x(c, part, stats, None)


def _attn_x(c, part, stats, mut):
    Z, hd, ns, dt = c.Z, c.att_hd, c.att_ns, c.dt
    H = Z // hd
    x = np.zeros(Z)
    for h in range(H):
        hs = h
        if mut == "head_off_by_one" and h % 2 == 1:
            hs = (h + 1) % H
        empty, A, L = stats[hs]
        acc = np.zeros(hd)
        for q in range(ns):
            f = 1.0 if q in A else 0.0
            if q == empty and mut != "empty_split":
                continue
            if q == empty:
                f = 1.0
            acc = acc + part[h, q, 2:] * (f / L) if f else acc + part[h, q, 2:] * 0.0
        x[h * hd:(h + 1) * hd] = acc
    if np.isnan(x).any():
        return x
    return rne16(np.where(x == 0, 0.0, x), dt)


def _build_weights(c, b, rng, geo):
    """weight images [Z][ld] (ld = N + 64, NaN padding), int8 scales, per-(row, segment) poison, steering"""
    Z, dt = c.Z, c.dt
    wrng = np.random.default_rng(c.seed)
    nimg = 2 if (c.pair or c.images == 2) else 1
    widths = [c.segs[0][0], c.segs[1][0]] if nimg == 2 else [sum(n for n, _ in c.segs)]
    b.Wv = [_weights(wrng, Z, n) for n in widths]                      # the VALUES (float32 integers; q for int8)
    b.scale = [np.ones(n) for n in widths]
    if c.w8 and not c.steer:
        b.scale = [2.0 ** wrng.integers(-3, 2, n).astype(np.float64) for n in widths]
    if c.layout == "order":
        for W in b.Wv:
            W[:] = 1.0
            W[b.order_rows[0]] = 4096.0
            W[b.order_rows[-1]] = 4096.0
        assert not c.w8
    # segment s -> (image, first column inside the image, ncols)
    b.seg_img = []
    off = 0
    for s, (n, _) in enumerate(c.segs):
        if nimg == 2:
            b.seg_img.append((s, 0, n))
        else:
            b.seg_img.append((0, off, n))
            off += n
    keeps = keepsets(c, b)
    if c.steer:
        _steer(c, b, keeps, rng)
    # images with poison
    b.images, b.ld = [], []
    for i, W in enumerate(b.Wv):
        n = W.shape[1]
        ld = n + 64
        img = np.full((Z, ld), math.nan if not c.w8 else 127.0, np.float32)
        img[:, :n] = W
        if c.w8:
            img[1::2, n:] = -128.0
        b.images.append(img)
        b.ld.append(ld)
    for s, (i, c0, n) in enumerate(b.seg_img):
        dead = ~keeps[s]
        if c.w8:
            b.images[i][np.ix_(dead, np.arange(c0, c0 + n))] = np.where(np.arange(dead.sum())[:, None] % 2 == 0, 127.0, -128.0)
        else:
            b.images[i][np.ix_(dead, np.arange(c0, c0 + n))] = math.nan
    b.images_t = [torch.from_numpy(img).to(torch.int8 if c.w8 else TDT[dt]) for img in b.images]
    b.scale_t = [torch.from_numpy(sc).to(TDT[dt]) for sc in b.scale] if c.w8 else None
    # bounds: every fp32 partial sum an exact multiple of the granularity below 2^24
    gran = 2.0 ** 8
    while not np.array_equal(np.round(b.x / gran), b.x / gran):   # the largest power of two every x is a multiple of
        gran /= 2
    ax = np.abs(b.x) / gran
    bound = 0.0
    for s, (i, c0, n) in enumerate(b.seg_img):
        kx = ax * keeps[s]
        if c.w8:   # the kernels' bias form: sum (q + 1152) x and 1152 sum x, both exact
            bound = max(bound, float((kx[:, None] * np.abs(b.Wv[i][:, c0:c0 + n] + INT8_BIAS)).sum(0).max()), INT8_BIAS * float(kx.sum()))
        else:
            bound = max(bound, float((kx[:, None] * np.abs(b.Wv[i][:, c0:c0 + n])).sum(0).max()))
    b.bound, b.gran = bound, gran
    if c.layout != "order":   # (the order probes want inexact sums: their partials are 2^24, 1 and -2^24 by construction)
        assert bound < 2 ** 24, (c.name, bound)
    if c.pair:   # mask_tau at, just below and just above a value |h| takes
        hv = np.abs(rne16(b.targets[0] * b.targets[1], dt))
        v0 = float(np.sort(np.unique(hv))[len(np.unique(hv)) // 2])
        b.mask_taus = [v0, float(np.nextafter(np.float32(v0), np.float32(0))), float(np.nextafter(np.float32(v0), np.float32(1e9)))]
    else:
        b.mask_taus = []


def keepsets(c, b, mut=None):
    """per segment: which rows are kept"""
    out = []
    for s, _ in enumerate(c.segs):
        tau = b.taus[s]
        if c.pair and s == 1 and mut == "pair_tau":
            tau = b.taus[0]
        if c.mode == IN_MASKED:
            out.append(b.meta["keep0"].copy())   # the producer's masks, whatever x and tau[s] say
        else:
            out.append(_keep(b.x, tau, ge=(mut == "ge")))
    return out


def _steer(c, b, keeps, rng):
    """weights of the correction rows: gate sums onto {16, 24, 32}, up sums onto small non-zero integers"""
    corr = b.corr
    x = b.x
    assert all(keeps[s][corr].all() for s in range(len(c.segs))) and c.mode in (IN_RESID_NORM, IN_PLAIN)
    b.targets = []
    for s, (i, c0, n) in enumerate(b.seg_img[:2]):
        W = b.Wv[i]
        W[corr, c0:c0 + n] = 0.0
        base = (x * keeps[s]) @ W[:, c0:c0 + n].astype(np.float64)
        tgt = rng.choice(GATES, n) if s == 0 else rng.choice([-5.0, -4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0, 5.0], n)
        d = tgt - base
        npairs = len(corr) // 2
        for p in range(npairs):
            dp = np.floor(d / npairs) + (d - np.floor(d / npairs) * npairs if p == 0 else 0.0)
            bb = np.mod(3 * dp, 4)
            aa = (dp - 3 * bb) / 4
            assert np.array_equal(4 * aa + 3 * bb, dp)
            W[corr[2 * p], c0:c0 + n] = aa
            W[corr[2 * p + 1], c0:c0 + n] = bb
        lim = 127 if c.w8 else TIE_LO[c.dt]
        assert np.abs(W[corr, c0:c0 + n]).max() <= lim, "correction weight not representable"
        assert np.array_equal(W[corr, c0:c0 + n], np.round(W[corr, c0:c0 + n])), "correction weights must be integers"
        assert np.array_equal((x * keeps[s]) @ W[:, c0:c0 + n].astype(np.float64), tgt)
        b.targets.append(tgt)


def _build_rope(c, b, rng):
    r = c.rope
    hd, ms, pos = r["hd"], r["max_seq"], r["pos"]
    tab = np.zeros((ms, hd // 2, 2))
    for p in range(ms):
        for j in range(hd // 2):
            tab[p, j] = ROPE_PAT[(p * 7 + j * 3 + (j >> 2)) % 5]
    b.meta["rope"] = tab
    b.inputs["rope"] = torch.from_numpy(tab.reshape(-1)).to(TDT[c.dt])
    b.inputs["rope_pos"] = torch.tensor([pos], dtype=torch.int32)


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _producer(c, b, mut):
    """x (float64 numbers of dt's grid; NaN where a mutant lets poison through) and the residual stream"""
    dt = c.dt
    m = b.meta

    def r16(v):
        return rne16(np.where(v == 0, 0.0, v), dt)

    if c.mode in (IN_PLAIN, IN_MASKED):
        return b.x, None
    if c.mode == IN_SILU_MUL:
        g, up = m["gate"], m["up"]
        if mut == "up_offset0":
            up = g
        act = bool(c.gate_activated) and mut != "gate_act_ignored"
        if not act:
            sl = g / (1.0 + np.exp(-g))
            g16 = torch.from_numpy(sl).to(TDT[dt]).double().numpy()
            if mut is None:
                assert np.array_equal(g16, g)
            g = g16
        prod = g * up
        return torch.from_numpy(prod).to(TDT[dt]).double().numpy(), None
    if c.mode == IN_ATTN_MERGE:
        return _attn_x(c, m["part"], m["stats"], mut), None
    S, resid, nw, rstd = m["S"], m["resid"], m["nw"], m["rstd"]
    if c.nslabs:
        ys = sum_slices_f32(S[::-1] if mut == "slabs_reverse" else S)
        if mut == "resid_before_round":
            h = r16(resid + ys)
        else:
            y16 = rne16(np.where(ys == 0, 0.0, ys), dt, mode="twice" if mut == "slab_sum_twice" else "rne")
            h = r16(resid + y16)
    else:
        h = resid
    if mut is None:
        assert np.array_equal(h, m["h"])
    ms = float((h * h).sum()) / c.Z
    r_eps = 1.0 / math.sqrt(ms + float(np.float32(c.eps)))
    if mut == "normw_before_round":
        x = r16(h * r_eps * nw)
    else:
        # (the true path: h * rstd rounds to the grid value h * 2^k, asserted at build time with 2^-12 to spare)
        g = r16(h * r_eps) if mut is not None else h * rstd
        x = r16(g * nw)
    return x, h


def _walk_mult(c, keep, geo, mut):
    """rows' multiplicities under a mutant of the per-wave row walk (kernels with wave-local lists): STEP = 4 * (64 / LPR)
    list entries per batch, two register sets alternating, a guarded tail batch"""
    mult = keep.astype(np.float64)
    if mut not in ("drop_last", "tail_dup", "skip_set_b"):
        return mult
    split, step = geo["split"], 4 * (64 // geo["lpr"])
    sl, wv = chunk_place(c.Z, split, c.mode)
    row_sl, row_wv = np.repeat(sl, 64)[: c.Z], np.repeat(wv, 64)[: c.Z]
    for s in range(split):
        for w in range(WAVES):
            L = np.nonzero(keep & (row_sl == s) & (row_wv == w))[0]
            n = len(L)
            if n == 0:
                continue
            nb, rem = n // step, n % step
            if mut == "drop_last":
                mult[L[-1]] = 0
            elif mut == "tail_dup" and rem:
                mult[L[-1]] += step - rem
            elif mut == "skip_set_b":
                for i in range(1, nb, 2):
                    mult[L[i * step:(i + 1) * step]] = 0
    return mult


def _row_slices(c, keep, geo):
    """per row: the slice whose workgroup adds it"""
    split = geo["split"]
    if split == 1:
        return np.zeros(c.Z, np.int64)
    if geo["kernel"] == "lean" or wave_local(c.Z, split, c.mode):
        sl, _ = chunk_place(c.Z, split, c.mode)
        return np.repeat(sl, 64)[: c.Z]
    # the general kernel's workgroup-wide list: `split` even shares of the ascending kept rows
    out = np.zeros(c.Z, np.int64)
    L = np.nonzero(keep)[0]
    tot = len(L)
    for k in range(split):
        out[L[tot * k // split: tot * (k + 1) // split]] = k
    return out


def reference(b, geo, mut=None):
    """every output buffer of the launch, whole (sentinels included), as integer words: {name: array}"""
    c = b.case
    dt, Z, split, lpr = c.dt, c.Z, geo["split"], geo["lpr"]
    bn = lpr * 8
    x, h = _producer(c, b, mut)
    bb = b
    if x is not b.x:
        bb = Built()
        bb.__dict__.update(b.__dict__)
        bb.x = x
    keeps = keepsets(c, bb, mut)
    if c.mode == IN_MASKED:
        keeps = [b.meta["keep0"] for _ in c.segs]
    nseg = len(c.segs)
    ncols = [n for n, _ in c.segs]
    partial = []   # per segment [split][ncols] float64
    wl = geo["kernel"] == "lean" or wave_local(Z, split, c.mode)
    for s, (i, c0, n) in enumerate(b.seg_img):
        img = b.images[i]
        if mut == "image2_col" and i == 1:
            img = np.roll(img, -(b.seg_img[0][2] % b.ld[1]), axis=1)   # column = tile * BN instead of (tile - w1_tile) * BN
        P = np.zeros((split, n))
        groups = [(0, n, keeps[s])]
        if mut == "seg_tau" and s > 0 and not c.pair:
            groups = [(0, bn, keeps[s - 1]), (bn, n, keeps[s])]
        for lo, hi, keep in groups:
            mult = _walk_mult(c, keep, geo, mut) if wl else keep.astype(np.float64)
            rs = _row_slices(c, keep, geo)
            xk = np.where(mult > 0, x, 0.0) * mult
            for k in range(split):
                rows = np.nonzero((mult > 0) & (rs == k))[0]
                if len(rows) == 0 and not (c.w8 and mut == "int8_bias_all"):
                    continue   # a slice that keeps nothing in this group: +0.0 (int8: (0 - 0) * scale)
                Wk = img[rows, c0 + lo: c0 + hi].astype(np.float64)
                if c.w8:   # sum (q + 1152) x - 1152 sum x over the rows the workgroup multiplies, then the column's scale
                    acc = xk[rows] @ (Wk + INT8_BIAS)
                    xb = xk[rows].sum()
                    if mut == "int8_bias_all":
                        every = rs == k if (split > 1 and wl) else np.ones(Z, bool)
                        xb = np.where(np.isfinite(x), x, 0.0)[every].sum()
                    P[k, lo:hi] = (acc - INT8_BIAS * xb) * b.scale[i][c0 + lo: c0 + hi]
                else:
                    P[k, lo:hi] = xk[rows] @ Wk
        partial.append(P)
    out = {}

    def fold(P):   # the launch's own sum over the slices, fp32, slice order
        if np.isnan(P).any():
            return P.sum(0)
        return sum_slices_f32(P[::-1] if mut == "slabs_reverse" else P)

    def r16(v):
        fin = np.isfinite(v) & (np.abs(v) <= 65504)   # (only a mutant lets poison through or leaves the formats' range)
        out16 = np.where(fin, 0.0, np.nan)
        out16[fin] = rne16(np.where(v[fin] == 0, 0.0, v[fin]), dt)
        return out16

    def words16(v, tail=TAIL):
        w = np.full(len(v) + tail, SENT16_I, np.int16)
        fin = np.isfinite(v)
        w[: len(v)] = 0x7E00
        w[: len(v)][fin] = bits16(v[fin], dt)
        return w

    def words32(v):
        if np.isnan(v).any():
            return np.where(np.isnan(v), np.int32(0x7FC00000), 0).astype(np.int32)
        return bits32(v)

    if h is not None and c.resid_out:
        out["resid_out"] = words16(h)
    if c.out == OUT_ROUNDED:
        ys = []
        for s in range(nseg):
            v = r16(fold(partial[s]))
            if c.act_seg0 and s == 0:
                v = _silu16(v, dt, exact=(mut is None))
            ys.append(v)
        out["y"] = words16(np.concatenate(ys))
    elif c.out == OUT_SLAB_SUM:
        v = fold(partial[0])
        w = np.full(ncols[0] + TAIL, SENT32_I, np.int32)
        w[: ncols[0]] = words32(v)
        out["slabs"] = w
    elif c.out == OUT_SLABS or (c.out == OUT_QKV_ROPE and not geo.get("rope")):
        N = sum(ncols)
        P = np.concatenate(partial, 1)   # [split][N]
        w = np.full(MAX_SLABS * N + TAIL, SENT32_I, np.int32)
        if c.il:
            st = (split + 3) & ~3
            v = w[: N * st].reshape(N, st)
            v[:, :split] = words32(P).T
        else:
            w[: split * N] = words32(P).reshape(-1)
        out["slabs"] = w
        if c.out == OUT_QKV_ROPE:
            r = c.rope
            out["y"] = np.full(N + TAIL, SENT16_I, np.int16)
            for nm in ("kc", "vc"):
                out[nm] = np.full((ncols[1] // r["hd"]) * r["max_seq"] * r["hd"] + TAIL, SENT16_I, np.int16)
    elif c.out == OUT_PAIR_SILU:
        g16, u16 = r16(fold(partial[0])), r16(fold(partial[1]))
        hv = r16(_silu16(g16, dt, exact=(mut is None)) * u16)
        out["y"] = words16(hv)
        if mut is None:
            assert (g16 != 0).all()
        b.h_ref = hv
        for j, mt in enumerate(b.mask_taus):
            kp = _keep(np.where(np.isfinite(hv), hv, 1e30), mt)
            words = np.zeros(len(hv) // 64, np.uint64)
            for mcol in np.nonzero(kp)[0]:
                words[mcol >> 6] |= np.uint64(1) << np.uint64(mcol & 63)
            w = np.full(len(words) + 8, SENT64_I, np.int64)
            w[: len(words)] = words.view(np.int64)
            out[f"mask_out{j}"] = w
    elif c.out == OUT_QKV_ROPE:
        r = c.rope
        hd, ms = r["hd"], r["max_seq"]
        p = min(max(r["pos"], 0), ms - 1)
        tab = b.meta["rope"]
        q, k, v = (r16(fold(partial[s])) for s in range(3))

        def rot(vec):
            e, o = vec[0::2], vec[1::2]
            j = (np.arange(len(vec)) % hd)[0::2] // 2
            cs, sn = tab[p, j, 0], tab[p, j, 1]
            if mut == "rope_sin_sign":
                sn = -sn
            if mut == "rope_swap":
                e, o = o, e
            res = np.empty_like(vec)
            res[0::2] = e * cs - o * sn
            res[1::2] = o * cs + e * sn
            # (signed zeros as the kernels' helpers give them — rope_even = fma(x0, c, -(x1 s)), rope_odd = fma(x1, c, x0 s):
            #  -3 * 0 - 0 * 1 is -0.0 there and here, and the rounding keeps a zero's sign)
            fin = np.isfinite(res)
            res[fin] = rne16(res[fin], dt)
            return res

        out["y"] = words16(np.concatenate([rot(q), np.full(ncols[1] + ncols[2], 0.0)]))
        out["y"][ncols[0]: ncols[0] + ncols[1] + ncols[2]] = SENT16_I    # k, v land in the caches only
        nkv = ncols[1] // hd
        for nm, vec in (("kc", rot(k)), ("vc", rot(v) if mut == "v_rotated" else v)):
            w = np.full(nkv * ms * hd + TAIL, SENT16_I, np.int16)
            view = w[: nkv * ms * hd].reshape(nkv, ms, hd)
            prow = min(p + 1, ms - 1) if (mut == "k_row_pos1" and nm == "kc") else p
            view[:, prow, :] = words16(vec, 0).reshape(nkv, hd)
            out[nm] = w
        out["slabs"] = np.full(MAX_SLABS * sum(ncols) + TAIL, SENT32_I, np.int32)
    b.partial = partial
    return out


def _silu16(v, dt, exact):
    """round16(silu(v)) of 16-bit numbers; on the true path v is in {16, 24, 32} and the result is v itself"""
    if exact:
        assert np.isin(v, GATES).all(), "gate sums not steered onto {16, 24, 32}"
        return v
    fin = np.where(np.isfinite(v), v, 0.0)
    with np.errstate(over="ignore"):
        s = fin / (1.0 + np.exp(-fin))
    r = torch.from_numpy(s).to(TDT[dt]).double().numpy()
    return np.where(np.isfinite(v), r, v)


def sensitivity(b, geo):
    """PAIR / act_seg0: every column's h changes when any single kept non-zero term of gate or up is removed"""
    c = b.case
    keeps = keepsets(c, b)
    g, u = b.targets
    worst = 0
    for s in (0, 1):
        i, c0, n = b.seg_img[s]
        rows = np.nonzero(keeps[s] & (b.x != 0))[0]
        T = b.Wv[i][np.ix_(rows, np.arange(c0, c0 + n))].astype(np.float64) * b.x[rows, None]
        T = np.where(T == 0, np.nan, T)   # (a zero correction weight is no term)
        if s == 0:
            g2 = g[None, :] - T
            with np.errstate(over="ignore", invalid="ignore"):
                sv = np.nan_to_num(g2 / (1.0 + np.exp(-g2)))
            sl = torch.from_numpy(sv).to(TDT[c.dt]).double().numpy()
            h2 = sl * u[None, :]
        else:
            h2 = g[None, :] * (u[None, :] - T)
        same = (h2 == (g * u)[None, :]) & ~np.isnan(T)
        worst += int(same.sum())
    return worst


# ---- the ledger ---------------------------------------------------------------------------------------------------------------

def ledger(b, geo):
    """what the case executed, from the launch's report and the reference alone"""
    c = b.case
    led = dict(kernel=geo["kernel"], lpr=geo["lpr"], split=geo["split"], kr=geo.get("kr"), exact=bool(geo.get("exact")),
               mode=c.mode, pair=c.pair, w8=c.w8, rope=bool(geo.get("rope")), out=OUT_NAME[c.out], dt=c.dt)
    step = 4 * (64 // geo["lpr"])
    keeps = keepsets(c, b)
    sizes, flags = set(), set()
    wl = geo["kernel"] == "lean" or wave_local(c.Z, geo["split"], c.mode)
    if wl:
        sl, wv = chunk_place(c.Z, geo["split"], c.mode)
        row_sl, row_wv = np.repeat(sl, 64)[: c.Z], np.repeat(wv, 64)[: c.Z]
        names = {0: "0", 1: "1", step - 1: "STEP-1", step: "STEP", step + 1: "STEP+1", 2 * step - 1: "2STEP-1", 2 * step: "2STEP",
                 2 * step + 1: "2STEP+1", 3 * step: "3STEP"}
        for keep in keeps[:1]:
            for s in range(geo["split"]):
                tot = 0
                for w in range(WAVES):
                    mine = (row_sl == s) & (row_wv == w)
                    n = int((keep & mine).sum())
                    tot += n
                    if n in names:
                        sizes.add(names[n])
                    if n and n == int(mine.sum()):
                        sizes.add("all")
                    rows = np.nonzero(mine)[0]
                    if len(rows) > 64:
                        n0 = int(keep[rows[:64]].sum())
                        if n0 >= step:
                            flags.add("early")
                        elif n >= step:
                            flags.add("late")
                    if (n // step) % 2 == 1:
                        flags.add("odd_batches")
                    if n >= step and (n // step) % 2 == 0:
                        flags.add("even_batches")
                if tot == 0:
                    flags.add("empty_wg")
    led["sizes"], led["flags"], led["wave_local"] = sorted(sizes), sorted(flags), wl
    return led


def check_claims(b, geo):
    c = b.case
    led = ledger(b, geo)
    for k, v in c.expect.items():
        assert led.get(k) == v, f"case {c.name}: the launch reports {k} = {led.get(k)!r}, the case was written for {v!r} ({geo})"
    for cl in c.claims:
        assert cl in led["sizes"] or cl in led["flags"], f"case {c.name}: class {cl} not reached ({led['sizes']}, {led['flags']})"
    return led


def probe_line(c, led, n):
    return (f"PROBE gemv {c.name} Z={c.Z} N={'+'.join(str(s[0]) for s in c.segs)} {c.dt} in={IN_NAME[c.mode]} out={led['out']}"
            f"{'+act_seg0' if c.act_seg0 else ''} kernel={led['kernel']} MODE={led['mode']} PAIR={int(led['pair'])} LPR={led['lpr']} "
            f"KR={led['kr']} EXACT={int(led['exact'])} W8={int(led['w8'])} ROPE={int(led['rope'])} split={led['split']} "
            f"wave_local={int(led['wave_local'])} sizes={','.join(led['sizes']) or '-'} flags={','.join(led['flags']) or '-'} "
            f"words compared = {n}, differing = 0")


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def _lean(lpr, split, kr, mode, **k):
    d = dict(kernel="lean", lpr=lpr, split=split, kr=kr, mode=mode)
    d.update(k)
    return d


def _gen(lpr, split, mode, **k):
    d = dict(kernel="general", lpr=lpr, split=split, mode=mode)
    d.update(k)
    return d


SIZE_CLAIMS = ("0", "1", "STEP-1", "STEP", "STEP+1", "2STEP-1", "2STEP", "2STEP+1", "3STEP", "all", "early", "late", "odd_batches",
               "even_batches")
WALK = ("ge", "drop_last", "tail_dup", "skip_set_b")


def cases():
    """every case of tests/test_exact_gemv_gpu.py, keyed by name.  lib = (lanes_per_row, split): forced through the
    diagnostics build; lib None: the product library's own geometry (expect: what its rule gives on a 256-CU device — the GPU
    test confirms it through the ledger)."""
    C = {}

    def add(c):
        assert c.name not in C
        C[c.name] = c

    for dt in ("fp16", "bf16"):
        # ---- PLAIN: per-wave list sizes, thresholds, two images, every element-wise KR, both tile widths ----
        add(Case(f"plain_sizes_lpr8_{dt}", dt, 4096, lib=(8, 1), layout="sizes", segs=[(128, 1.0)], expect=_lean(8, 1, 4, 0),
                 claims=SIZE_CLAIMS, mutants=WALK))
        add(Case(f"plain_sizes_lpr16_{dt}", dt, 4096, lib=(16, 1), layout="sizes", segs=[(128, 1.0)], expect=_lean(16, 1, 4, 0),
                 claims=SIZE_CLAIMS, mutants=WALK))
        add(Case(f"plain_sizes_split2_emptywg_{dt}", dt, 8192, lib=(8, 2), layout="sizes", segs=[(128, 1.0)],
                 expect=_lean(8, 2, 4, 0), claims=("empty_wg", "STEP", "2STEP+1"), mutants=WALK))
        add(Case(f"plain_z64_{dt}", dt, 64, lib=(8, 1), segs=[(128, 2.0)], expect=_lean(8, 1, 1, 0), claims=("0",), mutants=("ge", "drop_last")))
        add(Case(f"plain_z1024_kr1_{dt}", dt, 1024, lib=(8, 1), segs=[(64, 2.0), (64, 1.5), (128, -1.0)], expect=_lean(8, 1, 1, 0),
                 mutants=("ge", "seg_tau")))
        add(Case(f"plain_3tau_lpr16_{dt}", dt, 2048, lib=(16, 1), segs=[(128, 3.0), (128, 0.0), (128, 2.5)], expect=_lean(16, 1, 4, 0),
                 mutants=("ge", "seg_tau")))
        add(Case(f"plain_2img_{dt}", dt, 2048, lib=(8, 1), segs=[(128, 2.0), (128, -math.inf)], images=2, expect=_lean(8, 1, 4, 0),
                 mutants=("ge", "seg_tau", "image2_col")))
        add(Case(f"plain_kr8_{dt}", dt, 8192, lib=(8, 1), segs=[(128, 3.0)], expect=_lean(8, 1, 8, 0), mutants=("ge",)))
        add(Case(f"plain_z65536_split8_slabs_{dt}", dt, 65536, out=OUT_SLABS, lib=(8, 8), segs=[(128, 3.0)], xmax=4,
                 expect=_lean(8, 8, 8, 0), mutants=("ge",)))
        add(Case(f"plain_product_ticket_{dt}", dt, 4096, segs=[(256, 2.0)], expect=_lean(8, 4, 1, 0), mutants=("ge",)))
        add(Case(f"plain_order_ticket_{dt}", dt, 4096, lib=(8, 4), layout="order", segs=[(128, 0.5)], expect=_lean(8, 4, 1, 0),
                 mutants=("slabs_reverse",)))
        add(Case(f"plain_order_slabsum_{dt}", dt, 4096, out=OUT_SLAB_SUM, lib=(8, 4), layout="order", segs=[(128, 0.5)],
                 expect=_lean(8, 4, 1, 0), mutants=("slabs_reverse",)))
        add(Case(f"plain_slabsum_{dt}", dt, 5120, out=OUT_SLAB_SUM, lib=(16, 3), segs=[(128, 1.0)], expect=_lean(16, 3, 4, 0),
                 mutants=("ge", "drop_last")))
        add(Case(f"plain_slabs_il_{dt}", dt, 5120, out=OUT_SLABS, lib=(8, 5), segs=[(64, 2.0), (64, 1.0)], expect=_lean(8, 5, 1, 0),
                 mutants=("ge", "seg_tau")))
        # ---- the general kernel on the same probes ----
        add(Case(f"gen_plain_sizes_{dt}", dt, 4096, lib=(8, 1), fast=0, layout="sizes", segs=[(128, 1.0)], expect=_gen(8, 1, 0),
                 claims=SIZE_CLAIMS, mutants=WALK))
        add(Case(f"gen_plain_order_reduce_{dt}", dt, 4096, lib=(8, 4), fast=0, layout="order", segs=[(128, 0.5)], prepared=False,
                 expect=_gen(8, 4, 0), mutants=("slabs_reverse",)))
        add(Case(f"gen_plain_planar_slabs_{dt}", dt, 4096, out=OUT_SLABS, il=0, lib=(8, 3), fast=0, segs=[(64, 2.0), (72, 1.0)],
                 expect=_gen(8, 3, 0), mutants=("ge",)))
        add(Case(f"gen_plain_even_shares_{dt}", dt, 1024, out=OUT_SLABS, il=0, lib=(8, 2), fast=0, segs=[(128, 2.0)],
                 expect=_gen(8, 2, 0), mutants=("ge",)))
        add(Case(f"gen_plain_ragged_segs_{dt}", dt, 2048, lib=(16, 1), fast=0, segs=[(40, 3.0), (24, 0.0), (128, 2.5)],
                 expect=_gen(16, 1, 0), mutants=("ge",)))
        # ---- RESID_NORM: every slab count, both slab layouts, every KR, EXACT both ways ----
        # (KR 16 caches the whole vector per workgroup; its lists fit the LDS from two slices on)
        for ns, Z, kr, ex, sp in ((0, 1024, 4, False, 1), (1, 2048, 4, False, 1), (3, 4096, 4, True, 1), (4, 5120, 8, False, 1),
                                  (5, 8192, 8, True, 1), (8, 11008, 16, False, 2), (3, 16384, 16, True, 2)):
            add(Case(f"norm_ns{ns}_z{Z}_{dt}", dt, Z, mode=IN_RESID_NORM, lib=(8, sp), nslabs=ns, row_index=(ns == 0),
                     segs=[(64, 1.0), (64, 0.5)], probe_rounding=(ns >= 3), expect=_lean(8, sp, kr, 1, exact=ex),
                     mutants=("ge", "seg_tau") + (("slabs_reverse", "slab_sum_twice", "resid_before_round") if ns >= 3 else ())))
        add(Case(f"norm_planar1_{dt}", dt, 4096, mode=IN_RESID_NORM, lib=(16, 1), nslabs=1, slabs_il=0, segs=[(128, 1.0)],
                 expect=_lean(16, 1, 4, 1, exact=True), mutants=("ge",)))
        add(Case(f"norm_sizes_split2_{dt}", dt, 8192, mode=IN_RESID_NORM, out=OUT_SLABS, lib=(8, 2), nslabs=2, layout="sizes",
                 segs=[(128, 1.0)], expect=_lean(8, 2, 8, 1, exact=True), claims=("STEP", "STEP+1", "2STEP", "early", "late"), mutants=WALK))
        add(Case(f"norm_eps_{dt}", dt, 8192, mode=IN_RESID_NORM, lib=(8, 1), nslabs=0, eps=1e-5, segs=[(64, 2.5)],
                 expect=_lean(8, 1, 8, 1, exact=True), mutants=("normw_before_round",)))
        add(Case(f"gen_norm_planar_{dt}", dt, 4096, mode=IN_RESID_NORM, lib=(8, 2), fast=0, nslabs=3, slabs_il=0, out=OUT_SLABS, il=0,
                 probe_rounding=True, segs=[(64, 1.0), (64, 2.0)], expect=_gen(8, 2, 1),
                 mutants=("ge", "slabs_reverse", "slab_sum_twice", "resid_before_round")))
        # ---- SILU_MUL ----
        add(Case(f"silu_{dt}", dt, 11008, mode=IN_SILU_MUL, out=OUT_SLABS, lib=(8, 4), segs=[(128, 32.0)], xmax=3,
                 expect=_lean(8, 4, 4, 2), mutants=("ge", "up_offset0")))
        add(Case(f"silu_activated_{dt}", dt, 2048, mode=IN_SILU_MUL, gate_activated=1, lib=(16, 1), segs=[(128, 2.0)],
                 expect=_lean(16, 1, 4, 2), mutants=("ge", "up_offset0", "gate_act_ignored")))
        add(Case(f"silu_sizes_{dt}", dt, 4096, mode=IN_SILU_MUL, lib=(8, 1), layout="sizes", segs=[(128, 1.0)], xmax=3,
                 expect=_lean(8, 1, 4, 2), claims=("STEP-1", "STEP", "2STEP+1"), mutants=WALK))
        add(Case(f"gen_silu_{dt}", dt, 4096, mode=IN_SILU_MUL, lib=(8, 2), fast=0, prepared=False, segs=[(128, 32.0)], xmax=3,
                 expect=_gen(8, 2, 2), mutants=("ge", "up_offset0")))
        add(Case(f"silu_kr1_{dt}", dt, 1024, mode=IN_SILU_MUL, lib=(8, 1), segs=[(64, 16.0), (64, 48.0)], xmax=3,
                 expect=_lean(8, 1, 1, 2), mutants=("ge", "seg_tau", "up_offset0")))
        add(Case(f"silu_kr8_{dt}", dt, 8192, mode=IN_SILU_MUL, lib=(16, 1), segs=[(128, 64.0)], xmax=3,
                 expect=_lean(16, 1, 8, 2), mutants=("ge", "up_offset0")))
        # ---- MASKED ----
        add(Case(f"masked_kr1_{dt}", dt, 1024, mode=IN_MASKED, lib=(16, 1), segs=[(128, 3.0)], expect=_lean(16, 1, 1, 3),
                 mutants=("drop_last",)))
        add(Case(f"masked_kr8_{dt}", dt, 8192, mode=IN_MASKED, lib=(8, 1), segs=[(64, 2.0)], expect=_lean(8, 1, 8, 3),
                 mutants=("drop_last", "skip_set_b")))
        add(Case(f"masked_{dt}", dt, 4096, mode=IN_MASKED, lib=(8, 2), out=OUT_SLABS, segs=[(128, 2.0)], expect=_lean(8, 2, 4, 3),
                 mutants=("drop_last", "tail_dup")))
        add(Case(f"gen_masked_{dt}", dt, 4096, mode=IN_MASKED, lib=(8, 1), fast=0, segs=[(128, 2.0)], expect=_gen(8, 1, 3),
                 mutants=("drop_last",)))
        # ---- ATTN_MERGE ----
        add(Case(f"attn_ns4_hd128_{dt}", dt, 4096, mode=IN_ATTN_MERGE, att_ns=4, att_hd=128, lib=(8, 1), segs=[(128, 1.0)],
                 expect=_lean(8, 1, 4, 4), mutants=("ge", "empty_split", "head_off_by_one")))
        add(Case(f"attn_ns8_hd64_{dt}", dt, 8192, mode=IN_ATTN_MERGE, att_ns=8, att_hd=64, lib=(8, 2), out=OUT_SLABS, segs=[(128, 0.5)],
                 expect=_lean(8, 2, 4, 4), mutants=("ge", "empty_split", "head_off_by_one")))
        add(Case(f"attn_product_ticket_{dt}", dt, 4096, mode=IN_ATTN_MERGE, att_ns=4, att_hd=128, segs=[(256, 1.0)],
                 expect=_lean(8, 4, 1, 4), mutants=("ge", "empty_split", "head_off_by_one")))
        add(Case(f"attn_no_empty_split_{dt}", dt, 2048, mode=IN_ATTN_MERGE, att_ns=4, att_hd=64, att_empty=False, lib=(8, 1),
                 segs=[(64, 1.0)], expect=_lean(8, 1, 4, 4), mutants=("ge", "head_off_by_one")))
        add(Case(f"attn_kr8_{dt}", dt, 8192, mode=IN_ATTN_MERGE, att_ns=4, att_hd=64, lib=(8, 1), segs=[(64, 0.25)],
                 expect=_lean(8, 1, 8, 4), mutants=("ge", "empty_split", "head_off_by_one")))
        # just outside the lean kernel (nine rounds of chunks in one slice): the general kernel serves it
        add(Case(f"attn_outside_lean_{dt}", dt, 9216, mode=IN_ATTN_MERGE, att_ns=4, att_hd=128, lib=(8, 1), segs=[(64, 1.0)],
                 expect=_gen(8, 1, 4), mutants=("ge", "empty_split")))
        add(Case(f"gen_attn_ns4_{dt}", dt, 2048, mode=IN_ATTN_MERGE, att_ns=4, att_hd=64, lib=(8, 1), fast=0, segs=[(128, 1.0)],
                 expect=_gen(8, 1, 4), mutants=("ge", "empty_split")))
        # ---- act_seg0 and PAIR_SILU ----
        add(Case(f"act_seg0_{dt}", dt, 1024, mode=IN_RESID_NORM, lib=(8, 1), segs=[(128, 1.0), (128, 2.0)], images=2, act_seg0=1,
                 steer=True, nw_kind="sign", expect=_lean(8, 1, 4, 1), mutants=("ge", "seg_tau", "drop_last")))
        for tg, tu in ((1.0, 2.0), (2.0, 1.0), (1.0, 1.0)):
            add(Case(f"pair_{tg:g}_{tu:g}_{dt}", dt, 1024, mode=IN_RESID_NORM, out=OUT_PAIR_SILU, lib=(8, 1), segs=[(128, tg), (128, tu)],
                     steer=True, nw_kind="sign", expect=_lean(8, 1, 4, 1, pair=True),
                     mutants=("ge",) + (("pair_tau",) if tg != tu else ())))
        add(Case(f"gen_pair_{dt}", dt, 1024, mode=IN_RESID_NORM, out=OUT_PAIR_SILU, lib=(8, 1), fast=0, segs=[(128, 1.0), (128, 2.0)],
                 steer=True, nw_kind="sign", expect=_gen(8, 1, 1, pair=True), mutants=("ge", "pair_tau")))
        add(Case(f"act_seg0_ticket_{dt}", dt, 2048, mode=IN_RESID_NORM, lib=(8, 2), segs=[(128, 1.0), (128, 2.0)], images=2, act_seg0=1,
                 steer=True, nw_kind="sign", expect=_lean(8, 2, 4, 1), mutants=("ge", "seg_tau", "drop_last")))
        add(Case(f"gen_act_seg0_reduce_{dt}", dt, 2048, lib=(8, 2), fast=0, prepared=False, segs=[(128, 1.0), (128, 2.0)], act_seg0=1,
                 steer=True, expect=_gen(8, 2, 0), mutants=("ge", "drop_last")))
        # ---- int8 weights: every MODE at LPR 16 ----
        add(Case(f"w8_sizes_split2_emptywg_{dt}", dt, 8192, w8=True, lib=(16, 2), layout="sizes", segs=[(128, 1.0)], xmax=3,
                 expect=_lean(16, 2, 4, 0, w8=True), claims=("empty_wg", "STEP", "2STEP+1"), mutants=WALK + ("int8_bias_all",)))
        add(Case(f"gen_w8_silu_{dt}", dt, 2048, w8=True, mode=IN_SILU_MUL, lib=(8, 1), fast=0, segs=[(128, 32.0)], xmax=2,
                 expect=_gen(8, 1, 2, w8=True), mutants=("ge", "up_offset0", "int8_bias_all")))
        add(Case(f"gen_w8_masked_{dt}", dt, 2048, w8=True, mode=IN_MASKED, lib=(16, 2), fast=0, out=OUT_SLABS, il=0, segs=[(128, 2.0)],
                 expect=_gen(16, 2, 3, w8=True), mutants=("drop_last", "int8_bias_all")))
        add(Case(f"gen_w8_attn_{dt}", dt, 512, w8=True, mode=IN_ATTN_MERGE, att_ns=8, att_hd=64, lib=(8, 1), fast=0, segs=[(128, 1.0)],
                 expect=_gen(8, 1, 4, w8=True), mutants=("ge", "empty_split", "int8_bias_all")))
        add(Case(f"gen_w8_pair_{dt}", dt, 1024, w8=True, mode=IN_RESID_NORM, out=OUT_PAIR_SILU, lib=(8, 1), fast=0,
                 segs=[(128, 1.0), (128, 2.0)], steer=True, nw_kind="sign", expect=_gen(8, 1, 1, pair=True, w8=True),
                 mutants=("ge", "pair_tau")))
        add(Case(f"w8_plain_{dt}", dt, 4096, w8=True, lib=(16, 1), layout="sizes", segs=[(128, 1.0)], xmax=3, expect=_lean(16, 1, 4, 0, w8=True),
                 claims=("0", "STEP", "2STEP+1"), mutants=WALK + ("int8_bias_all",)))
        add(Case(f"w8_norm_slabs_{dt}", dt, 4096, w8=True, mode=IN_RESID_NORM, out=OUT_SLABS, lib=(16, 2), nslabs=4, segs=[(128, 1.0)],
                 expect=_lean(16, 2, 4, 1, w8=True, exact=True), mutants=("ge", "int8_bias_all")))
        add(Case(f"w8_silu_slabsum_{dt}", dt, 4096, w8=True, mode=IN_SILU_MUL, out=OUT_SLAB_SUM, lib=(16, 2), segs=[(128, 32.0)], xmax=2,
                 expect=_lean(16, 2, 4, 2, w8=True), mutants=("ge", "int8_bias_all")))
        add(Case(f"w8_masked_{dt}", dt, 2048, w8=True, mode=IN_MASKED, lib=(16, 1), segs=[(128, 2.0)], expect=_lean(16, 1, 4, 3, w8=True),
                 mutants=("drop_last", "int8_bias_all")))
        add(Case(f"w8_attn_{dt}", dt, 512, w8=True, mode=IN_ATTN_MERGE, att_ns=4, att_hd=64, lib=(16, 1), segs=[(128, 1.0)],
                 expect=_lean(16, 1, 1, 4, w8=True), mutants=("ge", "int8_bias_all")))
        add(Case(f"w8_act_seg0_{dt}", dt, 1024, w8=True, mode=IN_RESID_NORM, lib=(16, 1), segs=[(128, 1.0), (128, 2.0)], images=2, act_seg0=1,
                 steer=True, nw_kind="sign", expect=_lean(16, 1, 4, 1, w8=True), mutants=("ge", "int8_bias_all")))
        add(Case(f"gen_w8_plain_{dt}", dt, 2048, w8=True, lib=(8, 2), fast=0, prepared=False, segs=[(64, 2.0), (64, 1.0)],
                 expect=_gen(8, 2, 0, w8=True), mutants=("ge", "int8_bias_all")))
        add(Case(f"gen_w8_norm_{dt}", dt, 2048, w8=True, mode=IN_RESID_NORM, lib=(8, 1), fast=0, nslabs=2, segs=[(128, 1.0)],
                 expect=_gen(8, 1, 1, w8=True), mutants=("ge", "int8_bias_all")))
        # ---- QKV_ROPE (the product library's own geometry: the fused epilogue refuses forced ones) ----
        for hd, q, kv, pos, Z in ((64, 3328, 3328, 0, 1024), (128, 8192, 1024, 5, 1024), (128, 8192, 1024, 9, 1024)):
            add(Case(f"rope_hd{hd}_{'mha' if q == kv else 'gqa'}_pos{pos}_z{Z}_{dt}", dt, Z, mode=IN_RESID_NORM, out=OUT_QKV_ROPE,
                     segs=[(q, 1.0), (kv, 2.0), (kv, 0.5)], nslabs=2, rope=dict(hd=hd, max_seq=6, pos=pos),
                     expect=_lean(8, 1, 4, 1, rope=True, exact=False),
                     mutants=("ge", "seg_tau", "rope_swap", "rope_sin_sign", "v_rotated") + (("k_row_pos1",) if pos < 5 else ())))
        add(Case(f"rope_fallback_slabs_{dt}", dt, 2048, mode=IN_RESID_NORM, out=OUT_QKV_ROPE, segs=[(128, 1.0), (64, 2.0), (64, 0.5)],
                 nslabs=2, rope=dict(hd=64, max_seq=6, pos=2), expect=_lean(8, 2, 4, 1, rope=False), mutants=("ge", "seg_tau")))
    return C
