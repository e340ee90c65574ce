"""Exact-integer probes of the multi-column GEMM chain (not a test file): case builders, the integer reference, the coverage
ledger and a numpy model of the documented row walk.  Shared by tests/test_exact_gemm_host.py (CPU: the probes' own power)
and tests/test_exact_gemm_gpu.py (the HIP launches through the C ABI).

The chain — teal_prefill_gemm, teal_prefill_resid_norm, teal_batched_sparse_gemm(_slots), teal_batched_round_rows — adds
products of two 16-bit values in fp32 and rounds at documented points.  Fed small integers, every partial sum is exact in any
order, fused or not, so the outputs must equal an integer reference BIT FOR BIT:

  * activations are integers in [-4, 4], weights NON-ZERO integers in [-3, 3] (exact in fp16 and bf16): every kept term is a
    non-zero integer unless the activation itself is 0, so a lost, extra or doubled term moves a sum by at least 1;
  * sum |w| |x| over all Z rows, in units of the inputs' granularity, stays below 2^24 (`Built.bound`, asserted): every fp32
    partial sum is an integer multiple of that granularity below 2^24, hence exact whatever the order;
  * the producers are made exact: IN_NORM gets sums of squares whose mean is an exact power of 4 (rstd a power of two up to
    rsqrtf's error, every h * rstd asserted 2^-12 away from a 16-bit rounding tie), IN_SILU_MUL gets gates in {0, 16, 24, 32},
    where fp32 silu rounds to the gate itself (asserted to a quarter ulp in fp64);
  * everything a launch must not read holds NaN or +-Inf (weight rows outside a tile's union, the ld - N padding columns,
    hand-over slots of absent or inactive sequences, sumsq rows >= nwg), everything it might write holds a sentinel, and the
    reference says which words must change and which must still hold the sentinel.

The reference takes `split` as an argument — the value the launch reported — and never re-derives the host's split rule.
Geometry it does use is what include/teal_hip.h documents: rows in groups of 16, group q belongs to slice q mod split.
`ledger` classifies what a case executes (phases, last chunk, union-list size classes, guarded batches ...) from the shapes,
the split and the reference alone; `walk` is the numpy model of the kernels' row walk with one switch per mutant.
"""
import math

import numpy as np
import torch

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
CODE = {"fp16": 0, "bf16": 1}
PBITS = {"fp16": 11, "bf16": 8}          # significand bits, the implicit one included
TIE_LO = {"fp16": 2048, "bf16": 256}     # integers from here on are spaced 2 apart: odd ones are exact ties
IN_XT, IN_NORM, IN_SILU_MUL = 0, 1, 2
MODE_NAME = {IN_XT: "xt", IN_NORM: "norm", IN_SILU_MUL: "silu_mul"}
TAUS = (-math.inf, -1.0, 0.0, 0.5, 1.5, 2.0, 2.5, 3.5, 4.0)
SENT32_I = np.array([0x7FC5A5A5], np.uint32).view(np.int32)[0]  # fp32 sentinel word: a NaN with a payload no arithmetic produces
SENT16_I = np.int16(0x7E5A)
SENT_CNT = -77
POISON = (math.nan, math.inf, -math.inf)
BN, WAVES = 256, 16


# ---- number formats: round to nearest even, written out --------------------------------------------------------------------

def rne16(v, dt, mode="rne"):
    """float64 array -> the nearest number of dt's grid (as float64), by integer arithmetic on the significand: ties to the
    even significand.  mode "trunc" drops the remainder, "twice" rounds to one more bit first (a double rounding).  Normal
    range only (asserted): the probes stay between 2^-14 and 65504."""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    assert np.isfinite(a).all() and (a[a > 0] >= 2.0 ** -14).all() and (a <= 65504).all()

    def to_bits(a, p, trunc=False):
        m, e = np.frexp(a)                 # a = m 2^e, m in [0.5, 1)
        sc = np.ldexp(m, p)                # exact: in [2^(p-1), 2^p)
        fl = np.floor(sc)
        rem = sc - fl
        up = np.zeros_like(fl) if trunc else ((rem > 0.5) | ((rem == 0.5) & (np.mod(fl, 2) == 1))).astype(np.float64)
        return np.ldexp(fl + up, e - p)

    p = PBITS[dt]
    if mode == "twice":
        a = to_bits(a, p + 1)
    out = to_bits(a, p, trunc=(mode == "trunc"))
    return np.copysign(out, v)  # (a zero keeps its sign, as in the formats' own conversions)


def bits16(v, dt):
    """int16 bit patterns of values that ARE numbers of dt (asserted); -0.0 keeps its sign (0 * -1 is -0.0 on the device too)"""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64)))
    h = t.to(TDT[dt])
    assert torch.equal(h.double(), t), "not representable"
    return h.view(torch.int16).numpy()


def bits32(v):
    """int32 bit patterns of float64 values that are exact in fp32 (asserted), -0.0 as +0.0"""
    v = np.asarray(v, np.float64) + 0.0
    f = v.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), v)
    return f.view(np.int32)


def sum_slices_f32(slabs):
    """the consumers' sum: fp32, slice order"""
    acc = np.zeros(slabs.shape[1:], np.float32)
    for k in range(slabs.shape[0]):
        acc = (acc + slabs[k].astype(np.float32)).astype(np.float32)
    return acc.astype(np.float64)


def round_slabs(slabs, dt, mut=None):
    """round(sum of slabs in slice order): the one rounding of rounded_row / teal_batched_round_rows.  Mutants: "reverse"
    adds the slices last to first, "twice" rounds through one extra bit, "trunc" truncates."""
    s = sum_slices_f32(slabs[::-1] if mut == "reverse" else slabs)
    return rne16(s, dt, mode=mut if mut in ("twice", "trunc") else "rne")


# ---- geometry the headers document ----------------------------------------------------------------------------------------

def rows_for(T):
    return 8 if T <= 8 else 16


class Case:
    """One GEMM launch.  entry: "prefill" (dense), "batched", "slots".  S = T or B.  layout (IN_XT only): "random", "sizes"
    (slice k's union has the k-th size of `size_classes`), "phase2_empty", "phase2_only".  claims: ledger classes the case was
    written for (asserted after the launch)."""

    def __init__(self, name, entry, dt, Z, n0=256, n1=0, pad=64, S=8, mode=IN_XT, col_end=None, tau=None, active=None,
                 layout="random", expect_split=1, claims=(), gu_split=3, eps=0.0, nwg=3, seed=1, mutants=()):
        self.name, self.entry, self.dt, self.Z, self.n0, self.n1, self.pad, self.S, self.mode = name, entry, dt, Z, n0, n1, pad, S, mode
        self.N = n0 + n1
        dense = entry == "prefill"
        self.col_end = [self.N] if (dense or col_end is None) else list(col_end)
        self.tau = [-math.inf] if dense else list(tau if tau is not None else [1.5])
        assert len(self.col_end) == len(self.tau) and self.col_end[-1] == self.N
        self.active = active if entry == "slots" else None
        self.layout, self.expect_split, self.claims, self.gu_split, self.eps, self.nwg, self.seed = \
            layout, expect_split, dict(claims), gu_split, eps, nwg, seed
        self.mutants = tuple(mutants)
        self.R = rows_for(S) if dense else 8
        self.NP = (S + 1) // 2
        self.U = (8 if self.R == 8 else 4) if dense else (8 if self.NP <= 2 else 4)
        self.phase_rows = 1024 * 16 // self.R if dense else 2048
        self.live = [s < S and (self.active is None or (self.active >> s) & 1) for s in range(self.R)]
        # the prompt-pass GEMM takes an IN_XT hand-over as it is (its producers write slots >= T as zero); every other
        # producer of either kernel zeroes the slots >= T / >= B itself, so those hand-over slots are poisoned
        self.raw_slots = dense and mode == IN_XT

    def __repr__(self):
        return self.name


def row_place(Z, split, phase_rows):
    """per row m: (slice, phase, local row of the phase)"""
    m = np.arange(Z)
    q = m >> 4
    sl, j = q % split, q // split
    pg = phase_rows // 16
    return sl, j // pg, (j % pg) * 16 + (m & 15)


def size_classes(U, nrows):
    """union-list sizes a "sizes" layout gives the slices in turn: 0, below 16, 16 U, 16 * 2 U and their neighbours, all"""
    want = [0, 1, 15, 16, 17, 16 * U - 1, 16 * U, 16 * U + 1, 32 * U - 1, 32 * U, 32 * U + 1, nrows - 1, nrows, 16 * U + 9, 16 * U + 8 * 16 + 1, 7]
    return [min(n, nrows) for n in want]


def list_class(n, nrows, U):
    names = {0: "0", 16 * U - 1: "16U-1", 16 * U: "16U", 16 * U + 1: "16U+1", 32 * U - 1: "32U-1", 32 * U: "32U", 32 * U + 1: "32U+1"}
    out = set()
    if n in names:
        out.add(names[n])
    if 0 < n < 16:
        out.add("<16")
    if n == nrows:
        out.add("all")
    return out or {"other"}


def guarded_batches(njw, U):
    """guarded batches a wave with njw rows runs after its whole pairs: 0, 1 or 2"""
    rem = njw % (2 * U)
    return 0 if rem == 0 else (1 if rem <= U else 2)


# ---- builders ---------------------------------------------------------------------------------------------------------------

class Built:
    pass


def _weights(rng, Z, N):
    return (rng.integers(1, 4, (Z, N)) * rng.choice([-1, 1], (Z, N))).astype(np.float64)


def _poison_cols(R, dead, rng, Z):
    """[Z][R] float64 with NaN / +Inf / -Inf in the `dead` slots (0 elsewhere)"""
    p = np.zeros((Z, R))
    for s in range(R):
        if dead[s]:
            p[:, s] = np.array(POISON)[rng.integers(0, 3, Z)]
    return p


def _xt_layout(c, split, rng):
    """IN_XT activations [Z][S] for the case's layout"""
    Z, S = c.Z, c.S
    x = rng.integers(-4, 5, (Z, S)).astype(np.float64)
    if c.layout == "random":
        return x
    tmin = min(c.tau)
    assert tmin >= 1.0, "a layout that places the union needs activations that are not kept"
    big = [v for v in range(1, 5) if v > tmin]
    small = [v for v in range(-4, 5) if abs(v) <= tmin and v != 0] + [0]
    assert big and small
    sl, ph, lr = row_place(Z, split, c.phase_rows)
    keep_row = np.zeros(Z, bool)
    if c.layout == "sizes":
        for k in range(split):
            rows = np.nonzero(sl == k)[0]
            n = size_classes(c.U, len(rows))[k % 16]
            pick = rng.permutation(len(rows))[:n]
            if 0 < n < len(rows):  # the slice's last row (its last chunk) always belongs to a non-empty list
                pick[0] = len(rows) - 1 if len(rows) - 1 not in pick else pick[0]
            keep_row[rows[pick]] = True
    elif c.layout == "phase2_empty":
        keep_row = (ph == 0) & (rng.random(Z) < 0.5)
    elif c.layout == "phase2_only":
        keep_row = (ph > 0) & (rng.random(Z) < 0.75)
    else:
        raise ValueError(c.layout)
    x = rng.choice(small, (Z, S)).astype(np.float64)
    who = rng.integers(0, S, Z)  # the sequence that certainly keeps a union row; the others keep it or not at random
    xb = rng.choice(big, (Z, S)) * rng.choice([-1, 1], (Z, S))
    some = rng.random((Z, S)) < 0.4
    some[np.arange(Z), who] = True
    live = np.array(c.live[:S])
    if not live.any():
        return x
    # the certain keeper must be a live slot, or the union would be smaller than asked for
    lives = np.nonzero(live)[0]
    who = lives[rng.integers(0, len(lives), Z)]
    some[np.arange(Z), who] = True
    x = np.where(keep_row[:, None] & some, xb, x)
    return x


def build(c, split):
    """inputs (CPU torch tensors, poison included) and the reference of case c at the split the launch reports"""
    rng = np.random.default_rng(c.seed * 7919 + split)
    b = Built()
    b.case, b.split = c, split
    Z, N, R, S, dt = c.Z, c.N, c.R, c.S, c.dt
    b.W = _weights(np.random.default_rng(c.seed), Z, N)  # (the weights do not depend on the split)
    dead = [not (s < S) for s in range(R)] if c.entry != "slots" else [not c.live[s] for s in range(R)]
    gran = 1.0
    if c.mode == IN_XT:
        x = np.zeros((Z, R))
        x[:, :S] = _xt_layout(c, split, rng)
        hand = x.copy()
        pz = _poison_cols(R, dead, rng, Z)
        if c.raw_slots:  # slots T .. 2 NP - 1 zero (the hand-over's contract), the slots no token pair touches poisoned
            pz[:, : 2 * c.NP] = 0.0
        hand = np.where(pz != 0, pz, hand)
        b.xt = torch.from_numpy(hand).to(TDT[dt])
    elif c.mode == IN_NORM:
        gran = 8.0
        h = np.zeros((Z, R))
        # (with eps > 0 a power of two h * rstd sits less than 2^-12 above the tie below it in fp16: those draws avoid them)
        h[:, :S] = rng.integers(-4, 5, (Z, S)) if c.eps == 0 else rng.choice([0, 3, -3, 5, -5, 6, -6, 7, -7], (Z, S))
        ms = np.array([4.0, 1.0, 16.0, 0.25] * 4)[:R]                     # mean square per token: exact powers of 4
        rstd = 1.0 / np.sqrt(ms)
        nw = rng.choice([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], Z)
        # sumsq [64][R]: nwg rows of integers whose total over the rows is ms * Z exactly (rows >= nwg NaN: never read)
        tot = ms * Z
        assert (tot == np.floor(tot)).all() and (tot < 2 ** 24).all()
        sq = np.full((64, R), math.nan)
        part = np.floor(tot / c.nwg)
        sq[: c.nwg] = part
        sq[0] += tot - part * c.nwg
        assert np.array_equal(sq[: c.nwg].sum(0), tot)
        sq[:, [s for s in range(R) if dead[s]]] = math.nan
        # margins, in fp64: h * rstd(eps) rounds to h * 2^k with 2^-12 (relative) to spare either way
        r_eps = 1.0 / np.sqrt(ms + float(np.float32(c.eps)))
        v = h * r_eps
        nz = v != 0
        for f in (1 - 2.0 ** -12, 1 + 2.0 ** -12):
            assert np.array_equal(rne16(np.where(nz, v * f, 0.0), dt), h * rstd), "h * rstd too close to a rounding tie"
        x = rne16(rne16(h * rstd, dt) * nw[:, None], dt)
        assert np.array_equal(x, h * rstd * nw[:, None])
        hand = np.where(np.array(dead)[None, :], _poison_cols(R, dead, rng, Z), h)
        b.xt = torch.from_numpy(hand).to(TDT[dt])
        b.sumsq = torch.from_numpy(sq).float()
        b.norm_w = torch.from_numpy(nw).to(TDT[dt])
    else:
        g = np.zeros((Z, R))
        u = np.zeros((Z, R))
        g[:, :S] = rng.choice([0.0, 16.0, 24.0, 32.0], (Z, S))
        u[:, :S] = rng.integers(-4, 5, (Z, S))
        for gv in (16.0, 24.0, 32.0):  # fp32 silu rounds to the gate itself: a quarter of a 16-bit ulp in fp64
            assert abs(gv / (1.0 + math.exp(-gv)) - gv) < 0.25 * gv * 2.0 ** -PBITS[dt]
        x = g * u + 0.0
        # [gu_split][2 Z][R] integer slices that sum to gate | up; poisoned dead slots
        tgt = np.concatenate([g, u], 0)
        parts = rng.integers(-8, 9, (c.gu_split, 2 * Z, R)).astype(np.float64)
        parts[-1] = tgt - parts[:-1].sum(0)
        assert np.array_equal(sum_slices_f32(parts), tgt)
        parts[:, :, [s for s in range(R) if dead[s]]] = _poison_cols(R, dead, rng, 2 * Z)[None][:, :, [s for s in range(R) if dead[s]]]
        b.gu = torch.from_numpy(parts).float()
    b.gran = gran
    b.x = np.where(np.array(c.live)[None, :], x, 0.0)       # what a live slot's staged activation is; dead slots +0
    assert np.array_equal(rne16(b.x, dt), b.x)
    # what the kernel would stage for a dead slot if it let it through (mutant "inactive"): the poison / raw hand-over
    b.x_raw = x.copy()
    if c.mode == IN_XT or c.mode == IN_NORM:
        raw = b.xt.double().numpy()
        b.x_raw = np.where(np.array(c.live)[None, :], x, raw)
    else:
        b.x_raw = np.where(np.array(c.live)[None, :], x, math.inf)
    reference(b)
    return b


def keep_masks(c, x):
    """[nseg][Z][R] bool: float32(|x|) > float32(tau), live slots only"""
    live = np.array(c.live)[None, :]
    with np.errstate(invalid="ignore"):
        return np.stack([(np.abs(x).astype(np.float32) > np.float32(t)) & live for t in c.tau])


def tile_segments(c, tile):
    """(sfirst, slast, per-column local segment index) of a 256-column tile"""
    cols = tile * BN + np.arange(BN)
    seg = np.zeros(BN, int)
    for e in c.col_end[:-1]:
        seg += cols >= e
    return int(seg[0]), int(seg[-1]), seg - seg[0]


def reference(b):
    """the integer reference, slice by slice.  Sets on b:
         slabs  int32 words [split .. 16][N][R]: the fp32 bits the launch must leave (slices >= split and slots >= 2 NP: the
                sentinel, slots S .. 2 NP - 1 exactly zero)
         counts int32 [16][3][9] or None (entries of absent segments and of slices >= split: the sentinel)
         keep   [nseg][Z][R], union [tiles][Z] bool, nlist {(tile, slice, phase): union rows}"""
    c, split = b.case, b.split
    Z, N, R = c.Z, c.N, c.R
    keep = keep_masks(c, b.x)
    b.keep = keep
    bound = (np.abs(b.W).T @ np.abs(b.x)).max() * b.gran
    assert bound < 2 ** 24, ("exactness bound", bound)
    b.bound = bound
    sl, ph, lr = row_place(Z, split, c.phase_rows)
    b.place = (sl, ph, lr)
    val = np.zeros((split, N, R))
    lo = 0
    for i, hi in enumerate(c.col_end):
        xk = b.x * keep[i]
        for k in range(split):
            rows = sl == k
            val[k, lo:hi] = b.W[rows, lo:hi].T @ xk[rows]
        lo = hi
    words = np.full((16, N, R), SENT32_I, np.int32)
    words[:split, :, : 2 * c.NP] = bits32(val[:, :, : 2 * c.NP])
    b.val, b.slabs = val, words
    tiles = N // BN
    b.union = np.zeros((tiles, Z), bool)
    b.nlist = {}
    nph = int(ph.max()) + 1
    for t in range(tiles):
        sf, sla, _ = tile_segments(c, t)
        b.union[t] = keep[sf: sla + 1].any((0, 2))
        for k in range(split):
            for p in range(nph):
                sel = (sl == k) & (ph == p)
                if sel.any():
                    b.nlist[(t, k, p)] = int(b.union[t][sel].sum())
    b.counts = None
    if c.entry != "prefill":
        cnt = np.full((16, 3, 9), SENT_CNT, np.int32)
        for i in range(len(c.col_end)):
            for k in range(split):
                rows = sl == k
                cnt[k, i, :8] = keep[i][rows].sum(0)
                cnt[k, i, 8] = keep[i][rows].any(1).sum()
        b.counts = cnt
    return b


def images(b):
    """the W^T images [Z][ld] as CPU torch tensors: NaN in the padding columns and in every row a tile's union leaves out"""
    c = b.case
    W = b.W.copy()
    for t in range(c.N // BN):
        W[~b.union[t], t * BN:(t + 1) * BN] = math.nan
    out = []
    for lo, n in ((0, c.n0), (c.n0, c.n1)):
        if n == 0:
            out.append(None)
            continue
        img = np.full((c.Z, n + c.pad), math.nan)
        img[:, :n] = W[:, lo:lo + n]
        out.append(torch.from_numpy(img).to(TDT[c.dt]))
    return out


# ---- the coverage ledger ----------------------------------------------------------------------------------------------------

def ledger(b):
    """what the case executes, from the shapes, the reported split and the reference only"""
    c, split = b.case, b.split
    sl, ph, lr = b.place
    led = {"entry": c.entry, "split": split, "NP": c.NP, "R": c.R, "U": c.U, "producer": MODE_NAME[c.mode],
           "mask": None if c.active is None else f"{c.active:#04x}"}
    rows_in = {}
    for k in range(split):
        for p in range(int(ph.max()) + 1):
            n = int(((sl == k) & (ph == p)).sum())
            if n:
                rows_in[(k, p)] = n
    led["phases"] = max(p for _, p in rows_in) + 1
    nph = {k: max(p for kk, p in rows_in if kk == k) + 1 for k in range(split)}
    led["last_phase_rows"] = sorted({rows_in[(k, nph[k] - 1)] for k in range(split)})
    led["last_chunk_rows"] = sorted({(rows_in[kp] - 1) % 64 + 1 for kp in rows_in})
    classes, guarded = set(), set()
    for (t, k, p), n in b.nlist.items():
        nrows = rows_in[(k, p)]
        if c.entry == "prefill":
            n = nrows  # dense: every row is streamed
        classes |= list_class(n, nrows, c.U)
        for w in range(WAVES):
            njw = (n - w + WAVES - 1) // WAVES if n > w else 0
            guarded.add(guarded_batches(njw, c.U))
            if njw == 0:
                classes.add("idle wave")
        if p > 0:
            classes.add("phase2 empty" if n == 0 else "phase2 listed")
            if b.nlist[(t, k, 0)] == 0 and n > 0:
                classes.add("phase2 only")
    led["list"] = sorted(classes)
    led["guarded"] = sorted(guarded)
    led["segs_per_tile"] = max(tile_segments(c, t)[1] - tile_segments(c, t)[0] + 1 for t in range(c.N // BN))
    led["images"] = 2 if c.n1 else 1
    return led


def check_claims(b):
    """every ledger class the case was written for was hit (a device with another CU count fails here, loudly)"""
    led = ledger(b)
    for key, want in b.case.claims.items():
        got = led[key]
        if isinstance(got, list):
            miss = [w for w in (want if isinstance(want, (list, tuple, set)) else [want]) if w not in got]
            assert not miss, (b.case.name, "split", b.split, key, "missing", miss, "hit", got)
        else:
            assert got == want, (b.case.name, "split", b.split, key, got, "expected", want)
    return led


# ---- the numpy model of the row walk, with one switch per mutant -----------------------------------------------------------

MUTANTS = ("drop", "neighbour", "seg0_tau", "guarded_adds", "skip_last_chunk", "carry_list", "dup_first", "inactive")


def walk(b, mut=None):
    """The documented walk: per (tile, slice) the phases of phase_rows rows; per phase the staged activations and keep masks,
    the union list compacted in row order from 64-row chunks, dealt to 16 waves (entry i to wave i mod 16), batches of U with
    the last partial pair guarded (repeats add nothing), a lane's columns under their own segment's mask bits, slot pairs
    < NP, waves added in order.  Returns (slab words [16][N][R] int32, counts or None) in the reference's format."""
    c, split = b.case, b.split
    Z, N, R, U = c.Z, c.N, c.R, c.U
    dense = c.entry == "prefill"
    live = np.array([s < c.S for s in range(R)]) if mut == "inactive" else np.array(c.live)
    x_all = np.where(live[None, :], b.x_raw if mut == "inactive" else b.x, 0.0)
    val = np.zeros((split, N, R))
    cnt = np.full((16, 3, 9), SENT_CNT, np.int32) if not dense else None
    starts = [0] + c.col_end[:-1]
    pg = c.phase_rows // 16
    for t in range(N // BN):
        sf, sla, colseg = tile_segments(c, t)
        nls = sla - sf + 1
        taus = [c.tau[sf + i] for i in range(nls)]
        if mut == "seg0_tau":
            colseg = np.zeros_like(colseg)
        report = [i for i in range(nls) if starts[sf + i] // BN == t]
        for k in range(split):
            nj = (Z // 16 - k + split - 1) // split
            xs = np.zeros((c.phase_rows, R))
            lst_r, lst_m = np.zeros(0, int), np.zeros((0, nls, R), bool)
            acc = np.zeros((WAVES, BN, R))
            if cnt is not None:
                for i in report:
                    cnt[k, sf + i] = 0
            for jb in range(0, nj, pg):
                nrows = min(pg, nj - jb) * 16
                r = np.arange(nrows)
                m_of = (k + split * (jb + (r >> 4))) * 16 + (r & 15)
                xp = x_all[m_of]
                with np.errstate(invalid="ignore"):
                    mk = np.stack([(np.abs(xp).astype(np.float32) > np.float32(tu)) & live[None, :] for tu in taus], 1)
                if dense:
                    mk[:] = True
                xs[:nrows] = xp
                nch = nrows // 64 if (mut == "skip_last_chunk" and nrows % 64) else (nrows + 63) // 64
                scan = min(nch * 64, nrows)
                rows = np.nonzero(mk[:scan].any((1, 2)))[0]
                if mut == "dup_first" and jb and len(rows):
                    rows = np.concatenate([rows[:1], rows])
                masks = mk[rows]
                if cnt is not None:
                    for i in report:
                        cnt[k, sf + i, :8] += masks[:, i].sum(0).astype(np.int32)
                        cnt[k, sf + i, 8] += int(masks[:, i].any(1).sum())
                if mut == "carry_list" and jb and len(lst_r) > len(rows):
                    masks = np.concatenate([masks, lst_m[len(rows):]])
                    rows = np.concatenate([rows, lst_r[len(rows):]])
                lst_r, lst_m = rows, masks
                if mut == "drop" and len(rows):
                    rows, masks = rows[:-1], masks[:-1]
                if mut == "neighbour" and len(rows):
                    masks = np.roll(masks, -1, 0)
                for w in range(WAVES):
                    er, em = rows[w::WAVES], masks[w::WAVES]
                    njw = len(er)
                    if njw == 0:
                        continue
                    if mut == "guarded_adds" and njw % U:  # the repeats of the wave's last entry keep its mask
                        rep = U - njw % U
                        er = np.concatenate([er, np.repeat(er[-1:], rep)])
                        em = np.concatenate([em, np.repeat(em[-1:], rep, 0)])
                    mm = (k + split * (jb + (er >> 4))) * 16 + (er & 15)
                    mm, xe = mm % Z, xs[er]  # (a stale entry of a carried list may point past the matrix: the model wraps it)
                    for i in range(nls):
                        cs = np.nonzero(colseg == i)[0]
                        if len(cs):
                            xk = np.where(em[:, i, :], xe, 0.0)
                            with np.errstate(invalid="ignore"):
                                acc[w][cs] += b.W[np.ix_(mm, t * BN + cs)].T @ xk
            for w in range(WAVES):
                val[k, t * BN:(t + 1) * BN] += acc[w]
    words = np.full((16, N, R), SENT32_I, np.int32)
    with np.errstate(invalid="ignore"):
        words[:split, :, : 2 * c.NP] = (val[:, :, : 2 * c.NP] + 0.0).astype(np.float32).view(np.int32)
    return words, cnt


def first_diff(got, want):
    """index of the first differing word, or None"""
    d = np.nonzero(np.asarray(got) != np.asarray(want))
    return None if len(d[0]) == 0 else tuple(int(a[0]) for a in d)


# ---- the GEMM cases ---------------------------------------------------------------------------------------------------------

def gemm_cases():
    """every GEMM case of tests/test_exact_gemm_gpu.py, keyed by name.  expect_split is what the host's rule gives on a 256-CU
    device: the GPU test confirms it through the ledger, the host test uses it to run the model."""
    C = {}

    def add(c):
        assert c.name not in C
        C[c.name] = c
    walk_m = ("drop", "guarded_adds")
    for dt in ("fp16", "bf16"):
        # -- small geometry
        add(Case(f"b_small256_{dt}", "batched", dt, 256, S=3, tau=[0.5], expect_split=1, seed=11, claims={"split": 1, "phases": 1},
                 mutants=("drop", "neighbour")))
        add(Case(f"b_small512_3seg_{dt}", "batched", dt, 512, S=5, col_end=[96, 160, 256], tau=[2.0, 0.5, 3.5], expect_split=2, seed=12,
                 claims={"split": 2, "segs_per_tile": 3, "NP": 3}, mutants=("drop", "neighbour", "seg0_tau")))
        add(Case(f"b_two_images_{dt}", "batched", dt, 512, n0=256, n1=256, S=8, col_end=[248, 512], tau=[1.5, 2.5], expect_split=2, seed=13,
                 claims={"segs_per_tile": 2, "images": 2, "NP": 4}, mutants=walk_m + ("seg0_tau", "neighbour")))
        add(Case(f"b_ld_eq_n_{dt}", "batched", dt, 256, pad=0, S=2, tau=[0.0], expect_split=1, seed=14, claims={"NP": 1}, mutants=walk_m))
        add(Case(f"b_nobody_keeps_{dt}", "batched", dt, 512, S=4, col_end=[128, 256], tau=[4.0, -1.0], expect_split=2, seed=15,
                 claims={"segs_per_tile": 2, "list": ["all"]}, mutants=("drop", "seg0_tau")))
        add(Case(f"b_every_row_{dt}", "batched", dt, 512, S=1, tau=[-math.inf], expect_split=2, seed=16, claims={"list": ["all"], "NP": 1},
                 mutants=("drop",)))
        add(Case(f"p_small256_{dt}", "prefill", dt, 256, S=3, expect_split=1, seed=17, claims={"R": 8, "NP": 2}, mutants=("drop",)))
        add(Case(f"p_two_images_{dt}", "prefill", dt, 512, n0=256, n1=256, S=16, expect_split=2, seed=18, claims={"R": 16, "NP": 8, "images": 2},
                 mutants=("drop",)))
        # -- union-list sizes: slice k gets the k-th size class (built after the launch has reported the split)
        for S, U in ((3, 8), (6, 4)):
            add(Case(f"b_sizes_B{S}_{dt}", "batched", dt, 4096, S=S, tau=[1.5], layout="sizes", expect_split=16, seed=20 + S,
                     claims={"split": 16, "U": U, "guarded": [0, 1, 2],
                             "list": ["0", "<16", "16U-1", "16U", "16U+1", "32U-1", "32U", "all", "idle wave"] + (["32U+1"] if U == 4 else [])},
                     mutants=walk_m + ("neighbour",)))
        add(Case(f"b_sizes4352_B4_{dt}", "batched", dt, 4352, S=4, col_end=[96, 160, 256], tau=[1.5, 2.5, 3.5], layout="sizes", expect_split=12,
                 seed=25, claims={"split": 12, "last_chunk_rows": [32, 48], "list": ["32U+1", "0", "<16"], "segs_per_tile": 3, "U": 8},
                 mutants=walk_m + ("skip_last_chunk", "seg0_tau")))
        add(Case(f"b_4352_random_{dt}", "batched", dt, 4352, S=7, tau=[2.0], expect_split=12, seed=26,
                 claims={"last_chunk_rows": [32, 48], "NP": 4}, mutants=walk_m + ("skip_last_chunk", "neighbour")))
        # -- the second staging phase
        two = {"split": 16, "phases": 2, "last_phase_rows": [16], "last_chunk_rows": [16, 64]}
        ph_m = ("drop", "carry_list", "dup_first", "skip_last_chunk")
        add(Case(f"b_two_phase_{dt}", "batched", dt, 33024, S=5, tau=[2.5], expect_split=16, seed=30, claims=dict(two, list=["phase2 listed"]),
                 mutants=ph_m + ("guarded_adds", "neighbour")))
        add(Case(f"b_phase2_empty_{dt}", "batched", dt, 33024, S=2, tau=[1.5], layout="phase2_empty", expect_split=16, seed=31,
                 claims=dict(two, list=["phase2 empty"]), mutants=("drop", "carry_list")))
        add(Case(f"b_phase2_only_{dt}", "batched", dt, 33024, S=8, tau=[2.0], layout="phase2_only", expect_split=16, seed=32,
                 claims=dict(two, list=["phase2 only", "0"]), mutants=("drop", "dup_first", "skip_last_chunk")))
        add(Case(f"p_two_phase_R8_{dt}", "prefill", dt, 33024, S=7, expect_split=16, seed=33, claims=dict(two, R=8, guarded=[0, 1]),
                 mutants=("drop", "carry_list", "dup_first", "skip_last_chunk")))
        add(Case(f"p_two_phase_R16_{dt}", "prefill", dt, 16640, S=9, expect_split=15, seed=34,  # (9 batches per wave at 15 and at 16: the fewer slabs)
                 claims={"split": 15, "phases": 2, "last_phase_rows": [80, 96], "last_chunk_rows": [16, 32, 64], "R": 16, "NP": 5}, mutants=("drop", "carry_list", "dup_first")))
    # -- two whole phases: Z = 65536 is the entry points' ceiling, 4096 rows per slice (Llama-3's lm_head gives a slice as many)
    full = {"split": 16, "phases": 2, "last_phase_rows": [2048]}
    add(Case("b_two_full_phases_fp16", "batched", "fp16", 65536, S=6, tau=[2.5], expect_split=16, seed=36, claims=dict(full, list=["phase2 listed"]),
             mutants=("carry_list", "dup_first")))
    add(Case("b_two_full_phases_bf16", "batched", "bf16", 65536, S=2, col_end=[96, 160, 256], tau=[3.5, 2.0, 1.5], expect_split=16, seed=37,
             claims=dict(full, segs_per_tile=3, U=8), mutants=("carry_list", "dup_first", "seg0_tau")))
    add(Case("p_two_full_phases", "prefill", "fp16", 65536, S=8, expect_split=16, seed=38, claims=dict(full, R=8, NP=4), mutants=("drop", "dup_first")))
    for dt in ("fp16", "bf16"):
        # -- producers: one small shape and the two-phase shape each
        for mode, extra in ((IN_NORM, {"eps": 1e-5, "nwg": 3}), (IN_SILU_MUL, {"gu_split": 5})):
            mn = MODE_NAME[mode]
            add(Case(f"b_{mn}_small_{dt}", "batched", dt, 512, S=6, col_end=[128, 256], tau=[0.5, 2.0], mode=mode, expect_split=2, seed=40 + mode,
                     claims={"producer": mn}, mutants=("drop", "neighbour"), **extra))
            add(Case(f"p_{mn}_small_{dt}", "prefill", dt, 512, S=5, mode=mode, expect_split=2, seed=44 + mode, claims={"producer": mn, "R": 8},
                     mutants=("drop",), **extra))
            add(Case(f"b_{mn}_two_phase_{dt}", "batched", dt, 33024, S=3, tau=[1.5], mode=mode, expect_split=16, seed=48 + mode,
                     claims=dict(two, producer=mn), mutants=("drop", "dup_first"),
                     **({"eps": 0.0, "nwg": 64} if mode == IN_NORM else {"gu_split": 16})))
            add(Case(f"p_{mn}_two_phase_{dt}", "prefill", dt, 16640, S=12, mode=mode, expect_split=15, seed=52 + mode,
                     claims={"phases": 2, "R": 16, "producer": mn}, mutants=("drop", "dup_first"),
                     **({"eps": 0.0, "nwg": 1} if mode == IN_NORM else {"gu_split": 3})))
    # -- tokens and sequences (fp16 and bf16 alternate: the dtype cross product is covered above)
    for T in (1, 2, 7, 8, 9, 15, 16):
        add(Case(f"p_T{T}", "prefill", "fp16" if T % 2 else "bf16", 4352, S=T, expect_split=12, seed=60 + T,
                 claims={"NP": (T + 1) // 2, "R": rows_for(T), "guarded": [1] if T <= 8 else [2]}, mutants=("drop", "guarded_adds")))
    for B in range(1, 9):
        add(Case(f"b_B{B}", "batched", "bf16" if B % 2 else "fp16", 4352, S=B, col_end=[96, 256], tau=[0.5, 2.5], expect_split=12, seed=80 + B,
                 claims={"NP": (B + 1) // 2}, mutants=walk_m))
    for B, mask in ((8, 0x00), (8, 0x01), (8, 0x80), (8, 0xA5), (8, 0xFF), (5, 0b10110)):
        for dt in ("fp16", "bf16"):
            add(Case(f"s_B{B}_{mask:#04x}_{dt}", "slots", dt, 512, S=B, col_end=[128, 256], tau=[1.5, 0.0], active=mask, expect_split=2,
                     seed=100 + mask, claims={"mask": f"{mask:#04x}"}, mutants=(("inactive",) if mask != (1 << B) - 1 else ()) +
                     (("drop",) if mask else ())))
    add(Case("s_sizes_0xA5", "slots", "fp16", 4096, S=8, tau=[2.0], active=0xA5, layout="sizes", expect_split=16, seed=120,
             claims={"list": ["0", "<16", "16U", "all"], "mask": "0xa5"}, mutants=("inactive", "drop", "guarded_adds")))
    add(Case("s_silu_0x16", "slots", "bf16", 512, S=5, tau=[0.0], active=0b10110, mode=IN_SILU_MUL, gu_split=4, expect_split=2, seed=121,
             claims={"producer": "silu_mul"}, mutants=("inactive", "drop")))
    add(Case("s_norm_0x81", "slots", "fp16", 512, S=8, tau=[0.5], active=0x81, mode=IN_NORM, eps=1e-5, nwg=2, expect_split=2, seed=122,
             claims={"producer": "norm"}, mutants=("inactive", "drop")))
    for gs in (1, 3, 4, 5, 16):
        add(Case(f"p_silu_gu{gs}", "prefill", "fp16" if gs % 2 else "bf16", 512, S=9 if gs in (3, 5) else 4, mode=IN_SILU_MUL, gu_split=gs,
                 expect_split=2, seed=130 + gs, claims={"producer": "silu_mul"}, mutants=("drop",)))
    return C


# ---- teal_batched_round_rows and teal_prefill_resid_norm --------------------------------------------------------------------

def tie_slabs(rng, split, shape, dt, hi_factor=8):
    """integer slabs [split][*shape] whose sums land in [TIE_LO, hi_factor TIE_LO): odd sums below 2 TIE_LO are exact ties,
    sums = 5 or 11 (mod 16) past 4 TIE_LO round differently when rounded twice; both signs"""
    lo = TIE_LO[dt]
    tgt = rng.integers(lo, int(hi_factor * lo), shape) * rng.choice([-1, 1], shape)
    parts = rng.integers(-lo, lo, (split,) + tuple(shape)).astype(np.float64)
    parts[-1] = tgt - parts[:-1].sum(0)
    assert np.abs(parts).max() < 2 ** 24 and np.array_equal(sum_slices_f32(parts), tgt)
    return parts, tgt.astype(np.float64)


def order_slabs(dt):
    """three slices of one value where the slice order matters: a + 2 h + 2 h with a an exact 16-bit tie (odd, TIE_LO + 1) and
    h half of a's fp32 ulp.  In slice order each h is a tie that rounds back to a (even fp32 significand), the sum is a and
    the 16-bit tie goes to the even side, TIE_LO; last slice first, h + h is a's whole ulp and the sum rounds up."""
    a = float(TIE_LO[dt] + 1)
    h = math.ldexp(1.0, math.frexp(a)[1] - 24 - 1)
    return np.array([a, h, h])


def round_rows_case(dt, N, B, split, seed):
    """slabs [split][N][8] fp32 (slots >= B poisoned), want int16 words y [B][N]"""
    rng = np.random.default_rng(seed)
    parts, _ = tie_slabs(rng, split, (N, 8), dt)
    lo = TIE_LO[dt]  # columns 1 .. 5, slot 0: ties to either side, a sum that two roundings move, both signs (N = 8 holds them all)
    for j, v in enumerate((lo + 3, lo + 1, 4 * lo + 5, -(4 * lo + 5), -(lo + 1)), start=1):
        parts[:, j, 0] = 0.0
        parts[split - 1, j, 0] = v
    if split >= 3:  # column 0, slot 0: the slice-order probe (exact zeros in the other slices)
        parts[:, 0, 0] = 0.0
        parts[0, 0, 0], parts[split - 2, 0, 0], parts[split - 1, 0, 0] = order_slabs(dt)
    y = round_slabs(parts, dt)
    dead = [s >= B for s in range(8)]
    ps = _poison_cols(8, dead, rng, N)
    slabs = np.where(np.array(dead)[None, None, :], ps[None], parts)
    return parts, slabs, y


class ResidCase:
    """teal_prefill_resid_norm.  kind "norm": every token's mean square is an exact power of 4, so xt_out and x_last are exact
    too; kind "tie": free integers, one (fp16) or eight (bf16) columns per workgroup whose slab sums are 16-bit ties; only the
    first launch runs (no xt_out / x_last), ht_out and sumsq are checked."""

    def __init__(self, name, dt, dim, T, path, split, kind, inplace=False, outputs=("xt", "last"), eps=0.0, seed=1):
        self.name, self.dt, self.dim, self.T, self.path, self.split, self.kind, self.inplace, self.outputs, self.eps, self.seed = \
            name, dt, dim, T, path, split, kind, inplace, tuple(outputs), eps, seed
        self.R = rows_for(T)
        self.nwg = (dim + 255) // 256

    def __repr__(self):
        return self.name


def _pow4_column(rng, dim, k):
    """dim integers (or halves for k < 0 ... never: see below) whose mean square is 4^k exactly: blocks {2^(k+1), 0, 0, 0},
    blocks {2^(k+1), 2^(k-1) x 4} (k >= 1) and singles 2^k (k >= 0), shuffled, random signs"""
    vals = []
    left = dim
    while left:
        kind = rng.integers(0, 3)
        if kind == 0 and left >= 4:
            vals += [2.0 ** (k + 1), 0.0, 0.0, 0.0]
            left -= 4
        elif kind == 1 and k >= 1 and left >= 5:
            vals += [2.0 ** (k + 1)] + [2.0 ** (k - 1)] * 4
            left -= 5
        elif k >= 0:
            vals.append(2.0 ** k)
            left -= 1
        elif left < 4:
            raise ValueError("dim must be a multiple of 4 for a mean square of 1/4")
    v = np.array(vals)
    assert (v * v).sum() == dim * 4.0 ** k and (v == np.floor(v)).all()
    return rng.permutation(v) * rng.choice([-1, 1], dim)


def build_resid(c):
    rng = np.random.default_rng(c.seed)
    b = Built()
    b.case = c
    dim, T, R, dt = c.dim, c.T, c.R, c.dt
    dead = [s >= T for s in range(R)]
    vocab = 19
    b.tokens = np.array([(3 * s) % vocab if s % 4 else vocab - 1 for s in range(T)], np.int32)  # repeats and the last row
    if T > 1:
        b.tokens[T - 1] = b.tokens[0]
    emb = rng.integers(-4, 5, (vocab, dim)).astype(np.float64)
    hin = rng.integers(-4, 5, (dim, R)).astype(np.float64)
    h0 = emb[b.tokens].T if c.path == "tokens" else hin[:, :T]  # [dim][T]
    parts = None
    if c.kind == "norm":
        ks = [1, 0, 2, -1]
        h = np.stack([_pow4_column(rng, dim, ks[s % 4]) for s in range(T)], 1)
        if c.split:
            y = h - h0
            parts = rng.integers(-8, 9, (c.split, dim, T)).astype(np.float64)
            parts[-1] = y - parts[:-1].sum(0)
        else:  # nothing to add: the input itself carries the structure
            h0 = h
            if c.path == "tokens":  # distinct tokens, one embedding row each
                assert T <= vocab
                b.tokens = np.arange(T, dtype=np.int32)[::-1].copy()
                b.tokens[0] = vocab - 1
                emb[b.tokens] = h.T
            else:
                hin[:, :T] = h
        # (split 0 adds nothing: the input's bits pass through, a -0.0 included; a sum of slabs starts from +0.0 and is never -0.0)
        hh = h0.copy() if parts is None else rne16(h0 + round_slabs(parts, dt), dt)
        assert np.array_equal(hh, h)
    else:
        assert c.split >= 1
        parts = rng.integers(-3, 4, (c.split, dim, T)).astype(np.float64)
        # (the sums of squares must stay exact integers below 2^24: one fp16 tie column per workgroup below 1.4 * 2048, two
        #  bf16 ones below 8 * 256 — far enough for a sum that two roundings move, which fp16 cannot reach here)
        ntie = 1 if dt == "fp16" else 2
        for wg in range(c.nwg):
            cols = wg * 256 + rng.permutation(min(256, dim - wg * 256))[:ntie]
            tp, _ = tie_slabs(rng, c.split, (len(cols), T), dt, hi_factor=1.4 if dt == "fp16" else 8)
            if wg == 0:  # one sum for certain that truncation (fp16: a tie that goes up) and two roundings (bf16) move
                tp[:, 0, 0] = 0.0
                tp[c.split - 1, 0, 0] = TIE_LO[dt] + 3 if dt == "fp16" else 4 * TIE_LO[dt] + 5
            parts[:, cols] = tp
        if c.split >= 3:
            parts[:, 5, 0] = 0.0
            parts[0, 5, 0], parts[c.split - 2, 5, 0], parts[c.split - 1, 5, 0] = order_slabs(dt)
        y_r = round_slabs(parts, dt)
        hh = rne16((h0 + y_r).astype(np.float32).astype(np.float64), dt)
    b.parts = parts
    b.h = hh
    # per-workgroup sums of squares: exact integers below 2^24 (asserted), slots >= T exactly 0
    sq = np.zeros((c.nwg, R))
    for wg in range(c.nwg):
        sq[wg, :T] = (hh[wg * 256:(wg + 1) * 256] ** 2).sum(0)
    assert (sq < 2 ** 24).all() and (sq == np.floor(sq * 4) / 4).all()
    b.sumsq = bits32(sq)
    ht = np.zeros((dim, R))
    ht[:, :T] = hh
    b.ht = bits16(ht, dt)
    b.norm_w = rng.choice([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], dim)
    b.xt = b.x_last = None
    if c.kind == "norm":
        ms = sq.sum(0)[:T] / dim
        rstd = 1.0 / np.sqrt(ms)
        assert np.array_equal(np.log2(rstd), np.round(np.log2(rstd)))
        v = hh / np.sqrt(ms + float(np.float32(c.eps)))
        for f in (1 - 2.0 ** -12, 1 + 2.0 ** -12):
            assert np.array_equal(rne16(v * f, dt), hh * rstd), "h * rstd too close to a rounding tie"
        x = rne16(rne16(hh * rstd, dt) * b.norm_w[:, None], dt)
        xt = np.zeros((dim, R))
        xt[:, :T] = x
        b.xv = xt
        b.xt = bits16(xt, dt)
        b.x_last = bits16(x[:, T - 1], dt)
    # device inputs with poison in the slots >= T
    pz = _poison_cols(R, dead, rng, dim)
    b.emb = torch.from_numpy(emb).to(TDT[dt])
    hin_p = np.where(np.array(dead)[None, :], pz, hin)
    b.ht_in = torch.from_numpy(hin_p).to(TDT[dt])
    if parts is not None:
        full = np.zeros((c.split, dim, R))
        full[:, :, :T] = parts
        full = np.where(np.array(dead)[None, None, :], pz[None], full)
        b.slabs = torch.from_numpy(full).float()
        assert np.array_equal(b.slabs[:, :, :T].double().numpy(), parts)
    else:
        b.slabs = None
    return b


ROUND_CASES = [(dt, N, B, split) for dt in ("fp16", "bf16")
               for N, B, split in ((8, 1, 1), (256, 3, 2), (264, 8, 16), (32000, 3, 3), (264, 1, 5), (32000, 8, 2))]


def build_chain(rb, entry, split, tau=0.5):
    """the hand-over the engines use: teal_prefill_resid_norm's first launch (rb: a built "norm" case: ht_out and the sums of
    squares in its scratch), then a TEAL_PREFILL_IN_NORM GEMM over them.  The reference of the composition: the GEMM reference on
    the x the resid case expects."""
    rc = rb.case
    c = Case(f"chain_{entry}_{rc.name}", entry, rc.dt, rc.dim, S=rc.T, mode=IN_NORM, tau=[tau], nwg=rc.nwg, eps=rc.eps, expect_split=16,
             seed=rc.seed, claims={"producer": "norm"})
    b = Built()
    b.case, b.split, b.gran = c, split, 8.0
    b.W = _weights(np.random.default_rng(c.seed), c.Z, c.N)
    x = np.zeros((c.Z, c.R))
    x[:, : rb.xv.shape[1]] = rb.xv[:, : c.R]
    b.x = np.where(np.array(c.live)[None, :], x, 0.0)
    b.norm_w = torch.from_numpy(rb.norm_w).to(TDT[c.dt])
    return reference(b)


def resid_cases():
    C = {}

    def add(c):
        assert c.name not in C
        C[c.name] = c
    i = 0
    for dt in ("fp16", "bf16"):
        for dim in (64, 320, 4096, 16384):
            Ts = (1, 2, 7, 8, 9, 15, 16) if dim == 320 else ((3, 16) if dim == 16384 else (5, 12))
            for T in Ts:
                i += 1
                path = "tokens" if i % 2 else "ht_in"
                split = (0, 1, 3, 5, 16)[i % 5]
                outs = (("xt", "last"), ("xt",), ("last",))[i % 3]
                add(ResidCase(f"r_norm_{dt}_d{dim}_T{T}", dt, dim, T, path, split, "norm", inplace=(path == "ht_in" and i % 4 == 0),
                              outputs=outs, eps=1e-5 if (dt == "bf16" and i % 2) else 0.0, seed=200 + i))
        for dim, T, path, split, inplace in ((320, 7, "tokens", 3, False), (320, 16, "ht_in", 5, True), (4096, 8, "ht_in", 16, False),
                                            (16384, 9, "tokens", 1, False), (64, 2, "ht_in", 3, True)):
            i += 1
            add(ResidCase(f"r_tie_{dt}_d{dim}_T{T}", dt, dim, T, path, split, "tie", inplace=inplace, outputs=(), seed=300 + i))
    return C
