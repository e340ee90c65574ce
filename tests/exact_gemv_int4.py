"""Exact-integer probes of the int4 fused GEMV, teal_fused_gemv with weight_bits = 4 (not a test file): case class, builders,
the integer reference, the ledger and the mutants.  Shared by tests/test_exact_gemv_int4_host.py (CPU: the probes' own power)
and tests/test_exact_gemv_int4_gpu.py (the HIP launches through the C ABI).

tests/exact_gemv.py's principle applied to teal_amd/csrc/teal_gemv_int4.hip, a kernel that shares no device code with the
16-bit / int8 ones: fed small integers, every fp32 value the kernel forms is exact in any order, so every output word must
equal an integer reference BIT FOR BIT.

  * activations are integers u in [-4, 4] times the producer's unit; tau = 1 unit drops |u| <= 1 (|u| = 1 is the strict
    compare's tie) and keeps |u| >= 2.  Dropped rows mostly hold +-1, so a dropped row that leaks through a half-kept pair shows;
  * nibbles q are uniform in 0..15, scales bf16 powers of two in {1/4 .. 2}, zeros bf16 integers in [-3, 3] times the smallest
    scale, both drawn per (group, column);
  * the image is packed here from the layout text of include/teal_hip.h (row pairs; dword g = columns 4g .. 4g+3, low half row
    2p, high half row 2p + 1) and compared once with teal_amd.quantize.pack_int4_colmajor on the host;
  * bounds, asserted while building (in units of the inputs' granularity): per (unit, column) the biased accumulator
    sum |x| (1024 + 16 q) <= sum |x| * 1264 (bf16: 143) and the correction 1032 sum |x| (bf16: 136) stay below 2^24, and so does
    sum |scale * x (q - 8)| + |zero * x| per (slice, column) — every fmaf(scale, t, zero * X) and every partial sum is then exact;
  * poison: rows a segment does not keep carry nibble 15 (int4 cannot hold NaN), the ld - N padding bytes 0xFF, the
    scales_and_zeros cells of columns outside the launch's segments NaN; sentinel words sit behind y and resid_out, in the slab
    padding lanes and in the slabs beyond split.

The reference takes split and kind from what the launch REPORTED (*nslabs_out, teal_gemv_out.desc) and uses the unit rule
include/teal_hip.h documents next to TEAL_OUT_SLABS: unit u (rows 32u .. 32u+31) belongs to slice u mod split and to wave
(u div split) mod 16; a wave's j-th unit is slice + split * (wave + 16 j); a pass is 2 (SHARE) or 4 (GROUP) consecutive j.
`ledger` classifies what a case executed; every case asserts the classes it was written for.  MUTANTS are switches of the numpy
model; tests/test_exact_gemv_int4_host.py shows that each one changes a compared word of the cases that list it.
"""
import math
import re

import numpy as np
import torch

import exact_gemv as XG
from exact_gemm import CODE, SENT16_I, SENT32_I, TDT, TIE_LO, bits16, bits32, first_diff, rne16, sum_slices_f32  # noqa: F401
from exact_gemv import (GATES, IN_ATTN_MERGE, IN_MASKED, IN_NAME, IN_PLAIN, IN_RESID_NORM, IN_SILU_MUL, OUT_NAME,  # noqa: F401
                        OUT_PAIR_SILU, OUT_QKV_ROPE, OUT_ROUNDED, OUT_SLAB_SUM, OUT_SLABS, TAIL, WAVES, Built)

SHARE, GROUP = "share", "group"
KIND_OF = {1: SHARE, 0: GROUP}          # the kernel's third template argument
UP = {SHARE: 2, GROUP: 4}               # units per pass
SLAB_ROOM = 12                          # fp32 words per column behind `slabs` (split <= 8: the rest must stay sentinels)
SMIN = 0.25                             # the smallest scale in use
NAN16 = {"fp16": np.int16(0x7E00), "bf16": np.int16(0x7FC0)}
BIAS8 = {"fp16": 1032.0, "bf16": 136.0}   # bias + 8: what the flush subtracts per unit of sum x
BIAS_HI = {"fp16": 1264.0, "bf16": 143.0}  # the largest biased weight: 1024 + 16 * 15 / 128 + 15
COUNTS = (0, 16, 1, 3, 4, 5, 8, 15)
PATTERNS = ("even", "odd", "both", "mixed")

MUTANTS = (
    "ge",                     # >= where > belongs
    "pair_leak",              # a dropped row of a fetched pair keeps its activation
    "pair_swap",              # the halves of (x[2p], x[2p+1]) swapped
    "drop_last_pair",         # per unit
    "share_rank_ge4",         # SHARE drops ranks >= 4
    "stale_slot",             # a slot past the count is consumed with the previous pass's entry
    "dead_unit_doubles",      # a dead unit of the last pass re-adds the pass's first unit
    "odd_nibble_unscaled",    # the 1/16 at the flush omitted (fp16)
    "nibble_order",           # columns 4g+1 and 4g+2 swapped
    "bias_all_rows",          # the 1032 / 136 correction over all rows of the unit instead of the kept ones
    "zero_all_rows",          # zero * sum of ALL rows of the unit
    "zero_ignored",
    "group_is_unit",          # group index = unit index for G > 32
    "group_prev",             # the previous group's parameters
    "seg_tau",                # the previous segment's threshold for the first tile of segment 1 or 2
    "seg_scale_col0",         # a segment's scales read at image column 0
    "slabs_reverse",          # slices summed last to first (the launch's fold and the RESID_NORM consumer's sum)
    "in_slabs_4to7_dropped",  # the producer's second 16-byte load of slabs ignored
    "resid_before_round",
    "normw_before_round",
    "up_offset0",
    "empty_split",
    "head_off_by_one",
    "ticket_not_rearmed",     # modelled as the second launch's output: no slice is ever the last to arrive
)


class Case:
    """One teal_fused_gemv launch with weight_bits = 4.  segs: [(col0, ncols, tau in producer units)] inside ONE image of img_n
    columns.  expect: kind / split / passes the launch must report (the product library has no switches on this path: the
    shape decides), asserted through the ledger.  twice: launched twice on the same workspace, both outputs compared."""

    def __init__(self, name, dt, Z, G=32, mode=IN_PLAIN, out=OUT_ROUNDED, il=1, segs=((0, 128, 1.0),), img_n=None, prepared=True,
                 layout="random", expect=None, claims=(), mutants=(), seed=1, nslabs=0, eps=0.0, row_index=False, att_ns=4,
                 att_hd=64, att_arg=None, twice=False, empty_slice=False, off=0, probe_rounding=False, also_rounded=False):
        self.name, self.dt, self.Z, self.G, self.mode, self.out, self.il = name, dt, Z, G, mode, out, il
        self.segs = [(int(c0), int(n), float(t)) for c0, n, t in segs]
        self.img_n = img_n or max(c0 + n for c0, n, _ in self.segs)
        self.prepared, self.layout, self.expect = prepared, layout, dict(expect or {})
        self.claims, self.mutants, self.seed = tuple(claims), tuple(mutants), seed
        self.nslabs, self.eps, self.row_index = nslabs, eps, row_index
        self.att_ns, self.att_hd, self.att_arg = att_ns, att_hd, (att_ns if att_arg is None else att_arg)
        self.twice, self.empty_slice, self.off, self.probe_rounding, self.also_rounded = twice, empty_slice, off, probe_rounding, also_rounded
        # what the producer builders of exact_gemv read from a case
        self.xmax, self.nw_kind, self.steer, self.slabs_il, self.att_empty, self.gate_activated, self.resid_out = 4, "pow2", False, 1, True, 0, True
        self.N = sum(n for _, n, _ in self.segs)
        assert Z % G == 0 and all(n % 128 == 0 and c0 % 8 == 0 for c0, n, _ in self.segs)

    def __repr__(self):
        return self.name


# ---- geometry -----------------------------------------------------------------------------------------------------------------

def unit_place(Z, split):
    """per 32-row unit u: (slice, wave, j) — include/teal_hip.h, TEAL_OUT_SLABS (int4)"""
    u = np.arange(Z // 32)
    return u % split, (u // split) % WAVES, u // (split * WAVES)


def shape_rule(c, num_cu=256):
    """the host's choice as the issue states it: split = min(8, num_cu / ntiles, nunits / 16), 1 when a ROUNDED launch has an
    unprepared workspace; SHARE iff a wave owns at most two units"""
    ntiles, nunits = c.N // 128, c.Z // 32
    split = max(1, min(8, num_cu // ntiles, nunits // 16))
    if c.out == OUT_ROUNDED and not c.prepared:
        split = 1
    upw = (nunits + split * 16 - 1) // (split * 16)
    kind = SHARE if upw <= 2 else GROUP
    return dict(kind=kind, split=split, passes=(upw + UP[kind] - 1) // UP[kind])


def parse_desc(desc):
    """teal_gemv_out.desc of an int4 launch -> {kernel, bf16, mode, kind, ntiles, split}"""
    m = re.match(r"sparse_gemv_int4_kernel<(\w+),(\d+),(\d+),(\w+)> grid \((\d+),(\d+)\) x 1024$", desc)
    assert m, desc
    g = m.groups()
    return dict(kernel="int4", bf16=g[0] == "true", mode=int(g[1]), kind=KIND_OF[int(g[2])], phase=g[3] == "true", ntiles=int(g[4]),
                split=int(g[5]))


def geometry(c, desc=None, nslabs_out=None):
    """the geometry the reference runs at: from the launch's own report, or (host tests) from the case's expectation"""
    if desc is None:
        return dict(kernel="int4", kind=c.expect["kind"], split=c.expect["split"], mode=c.mode, bf16=c.dt == "bf16", ntiles=c.N // 128)
    g = parse_desc(desc)
    assert g["mode"] == c.mode and g["bf16"] == (c.dt == "bf16") and g["ntiles"] == c.N // 128 and not g["phase"], (c.name, desc)
    assert nslabs_out is None or nslabs_out == g["split"], (desc, nslabs_out)
    return g


# ---- builders -----------------------------------------------------------------------------------------------------------------

def _mag(rng):
    return float(rng.integers(2, 5)) * float(rng.choice([-1, 1]))


def _fill_unit(rng, n, pat):
    """32 integers: n kept pairs (|u| >= 2 in the even row, the odd row or both), every other entry dropped (+-1, some 0);
    the dropped partner of a half-kept pair is +-1"""
    v = rng.choice([1.0, -1.0, 1.0, -1.0, 0.0], 32)
    for k, p in enumerate(rng.permutation(16)[:n]):
        md = pat if pat != "mixed" else PATTERNS[k % 3]
        v[2 * p], v[2 * p + 1] = float(rng.choice([-1, 1])), float(rng.choice([-1, 1]))
        if md in ("even", "both"):
            v[2 * p] = _mag(rng)
        if md in ("odd", "both"):
            v[2 * p + 1] = _mag(rng)
    return v


def _want(c, s, w, j, geo):
    """kept pairs and half pattern prescribed for the j-th unit of (slice s, wave w)"""
    if c.layout == "stale":   # a pass with 16 pairs in every unit, then a pass with 1 .. 3: slots 3 .. 15 hold stale entries
        P = j // UP[geo["kind"]]
        n = 16 if P % 2 == 0 else 1 + (w + j) % 3
        pat = "both" if n == 16 else PATTERNS[(w + j) % 4]
    else:
        n, pat = COUNTS[(w + 5 * s + j + c.off) % 8], PATTERNS[(w + s + j) % 4]
    if c.empty_slice and s == geo["split"] - 1:
        n = 0
    return n, pat


def _layout_u(c, rng, geo):
    Z, split = c.Z, geo["split"]
    nu = Z // 32
    b_extra = {}
    if c.layout in ("random", "nan", "eps"):   # (eps: the RMSNorm builder's own vector)
        u = rng.choice([-4.0, -3.0, -2.0, -1.0, -1.0, -1.0, 0.0, 1.0, 1.0, 1.0, 2.0, 3.0, 4.0], Z)
        if c.layout == "nan":   # NaN as the only kept row of a half-kept pair
            r = 32 * (nu // 2) + 7
            u[r - 1], u[r] = 1.0, math.nan
            b_extra["nan_row"] = r
        return u, b_extra
    u = rng.choice([1.0, -1.0], Z)
    if c.layout == "order":
        # slice-order probe: slice 0's partial is 2^24 (x = 4, q = 12, scale 2^20), the last slice's -2^24, every other slice's 1
        assert c.G == 32 and split >= 3 and nu >= split * split + 1
        units = [s + split * s for s in range(split)]   # wave s of slice s
        rows = [32 * uu + 5 for uu in units]
        for s, r in enumerate(rows):
            u[r] = -4.0 if s == split - 1 else 4.0
        b_extra["order_units"], b_extra["order_rows"] = units, rows
        return u, b_extra
    if c.layout == "round":
        # rounding probe: unit A adds (q - 8) T / 2 per column (up to 3.5 T: past the 11 / 8 significant bits, integers spaced 2 and
        # 4 apart), unit B small integers: sums on and next to the round-to-nearest-even ties
        ua, ub = 3, 6
        u[32 * ua + 7] = 4.0
        u[32 * ub: 32 * ub + 32] = _fill_unit(rng, 8, "both")
        b_extra["round_units"] = (ua, ub)
        return u, b_extra
    assert c.layout in ("counts", "stale")
    sl, wv, jj = unit_place(Z, split)
    for uu in range(nu):
        n, pat = _want(c, int(sl[uu]), int(wv[uu]), int(jj[uu]), geo)
        u[32 * uu: 32 * uu + 32] = _fill_unit(rng, n, pat)
    return u, b_extra


def pack_image(Q, ld):
    """nibbles [Z][N] -> bytes [Z / 2][ld] as include/teal_hip.h lays them out: the 32-bit word g of pair-row p holds columns
    4g .. 4g+3 of row 2p in its low half (nibble j = column 4g + j) and of row 2p + 1 in its high half; padding 0xFF"""
    Z, N = Q.shape
    q = Q.astype(np.uint8)
    by = q[:, 0::2] | (q[:, 1::2] << 4)              # [Z][N / 2]: byte j = columns 2j, 2j + 1
    body = np.empty((Z // 2, N // 4, 4), np.uint8)
    body[:, :, 0:2] = by[0::2].reshape(Z // 2, N // 4, 2)
    body[:, :, 2:4] = by[1::2].reshape(Z // 2, N // 4, 2)
    img = np.full((Z // 2, ld), 0xFF, np.uint8)
    img[:, :N] = body.reshape(Z // 2, N)
    return img


def _keep(x, tau, ge=False):
    a, t = np.abs(x).astype(np.float32), np.float32(tau)
    return ((a >= t) if ge else (a > t)) | np.isnan(x)


def keepsets(c, b, x, mut=None):
    return [_keep(x, t, ge=(mut == "ge")) for t in b.taus]


def build(c, geo=None):
    """inputs (CPU torch tensors, poison included) of case c.  geo: the launch geometry the prescribed layouts are built for
    (default: the case's expectation)."""
    geo = geo or geometry(c)
    rng = np.random.default_rng(c.seed * 7919 + 13)
    b = Built()
    b.case, b.geo_built, b.inputs, b.meta = c, dict(geo), {}, {}
    Z, dt, G = c.Z, c.dt, c.G
    u, extra = _layout_u(c, rng, geo)
    b.__dict__.update(extra)
    classed = c.layout in ("counts", "stale", "random")
    unit = 1.0
    if c.mode == IN_PLAIN:
        x = u + 0.0
        b.inputs["x"] = torch.from_numpy(x).to(TDT[dt])
    elif c.mode == IN_SILU_MUL:
        for gv in GATES:   # fp32 silu rounds to the gate itself
            assert abs(gv / (1.0 + math.exp(-gv)) - gv) < 0.25 * gv * 2.0 ** -XG.PBITS[dt]
        g = np.full(Z, 16.0) if c.layout != "random" else rng.choice(GATES, Z)
        unit = 16.0 if c.layout != "random" else 1.0
        x = g * u
        b.meta["gate"], b.meta["up"] = g, u
        b.inputs["x"] = torch.from_numpy(np.concatenate([g, u])).to(TDT[dt])
    elif c.mode == IN_RESID_NORM:
        x = XG._build_resid_norm(c, b, u, classed and c.eps == 0, [], rng)
        unit = b.meta["unit"]
    else:
        assert c.mode == IN_ATTN_MERGE
        x = XG._build_attn(c, b, rng)
    b.x, b.unit = x + 0.0, unit
    bits16(np.nan_to_num(b.x), dt)   # (asserts that x is made of numbers of dt)
    b.taus = [t * unit for _, _, t in c.segs]
    _build_weights(c, b, geo)
    return b


def _build_weights(c, b, geo):
    Z, dt, G, N = c.Z, c.dt, c.G, c.img_n
    wrng = np.random.default_rng(c.seed)
    ng, nu = Z // G, Z // 32
    Q = wrng.integers(0, 16, (Z, N)).astype(np.int64)
    SC = 2.0 ** wrng.integers(-2, 2, (ng, N)).astype(np.float64)
    ZR = wrng.integers(-3, 4, (ng, N)).astype(np.float64) * SMIN
    if c.layout == "order":
        SC[:], units = SMIN, b.order_units
        for k, (uu, r) in enumerate(zip(units, b.order_rows)):
            big = k in (0, len(units) - 1)
            SC[uu], ZR[uu], Q[r] = (2.0 ** 20 if big else SMIN), 0.0, (12 if big else 9)
    if c.layout == "round":
        ua, ub = b.round_units
        T = float(TIE_LO[dt])
        SC[ua], SC[ub] = T / 8.0, 1.0
        ZR[ua], ZR[ub] = np.round(ZR[ua] / SMIN) * SMIN, np.round(ZR[ub] / SMIN)
    assert Q.min() == 0 and Q.max() == 15 and (ZR != 0).mean() > 0.5
    if c.layout != "order":   # differing from group to group and from column to column
        assert ng == 1 or ((SC[1:] != SC[:-1]).mean() > 0.5 and (ZR[1:] != ZR[:-1]).mean() > 0.5)
        assert (SC[:, 1:] != SC[:, :-1]).mean() > 0.5 and (ZR[:, 1:] != ZR[:, :-1]).mean() > 0.5
    keeps = keepsets(c, b, b.x)
    covered = np.zeros(N, bool)
    for s, (c0, n, _) in enumerate(c.segs):
        assert not covered[c0:c0 + n].any()
        covered[c0:c0 + n] = True
        Q[np.ix_(~keeps[s], np.arange(c0, c0 + n))] = 15   # rows the segment does not keep: the largest nibble
    b.Q, b.SC, b.ZR = Q, SC, ZR
    b.ld = N + 64
    b.scale_ld = N + 8
    b.image = pack_image(Q, b.ld)
    sz = np.full((ng, b.scale_ld, 2), math.nan)
    sz[:, :N, 0] = np.where(covered[None, :], SC, math.nan)    # columns outside the launch's segments: NaN
    sz[:, :N, 1] = np.where(covered[None, :], ZR, math.nan)
    b.image_t = torch.from_numpy(b.image)
    b.sz_t = torch.from_numpy(sz).to(torch.bfloat16)
    chk = b.sz_t.double().numpy()
    assert np.array_equal(np.nan_to_num(chk, nan=-77.0), np.nan_to_num(sz, nan=-77.0)), "scales / zeros not bf16 numbers"
    assert (np.log2(SC) == np.round(np.log2(SC))).all()
    # ---- bounds: every fp32 value the kernel forms an exact multiple of the granularity below 2^24 ----
    xf = np.nan_to_num(b.x)
    gran = 2.0 ** 8
    while not np.array_equal(np.round(xf / gran), xf / gran):
        gran /= 2
    smin = float(min(SC.min(), np.abs(ZR[ZR != 0]).min())) if c.layout in ("order", "round") else SMIN
    bound = 0.0
    split = geo["split"]
    grp = (32 * np.arange(nu)) // G
    for s, (c0, n, _) in enumerate(c.segs):
        kx = (np.abs(xf) / gran * keeps[s]).reshape(nu, 32)
        U = kx.sum(1)
        bound = max(bound, float(U.max()) * BIAS_HI[dt], float(U.max()) * BIAS8[dt])
        aq = np.abs(Q[:, c0:c0 + n] - 8).astype(np.float64).reshape(nu, 32, n)
        T = np.matmul(kx[:, None, :], aq)[:, 0, :] * (SC[grp, c0:c0 + n] / smin) + U[:, None] * (np.abs(ZR[grp, c0:c0 + n]) / smin)
        for k in range(split):
            bound = max(bound, float(T[k::split].sum(0).max()))
    b.bound, b.gran = bound, gran * smin
    if c.layout != "order":   # (the order probe wants inexact sums: its partials are 2^24, 1 and -2^24 by construction)
        assert bound < 2 ** 24, (c.name, bound)


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _producer(c, b, mut):
    if mut == "in_slabs_4to7_dropped" and c.mode == IN_RESID_NORM:
        b2 = Built()
        b2.__dict__.update(b.__dict__)
        b2.meta = dict(b.meta)
        S = b.meta["S"].copy()
        S[4:] = 0.0
        if c.probe_rounding:   # (the order column holds +-2^24: losing half of it leaves the 16-bit range)
            S[:, 11] = b.meta["S"][:, 11]
        b2.meta["S"] = S
        return XG._producer(c, b2, mut)
    return XG._producer(c, b, mut)


def _walk(c, geo, x, keep, mut):
    """per unit: the 32 multipliers of the unit's weight rows and what the kernel sums as X, under a mutant of the list walk"""
    nu = c.Z // 32
    kind, split = geo["kind"], geo["split"]
    xu = x.reshape(nu, 32)
    xw = np.where(keep, x, 0.0).reshape(nu, 32)
    pk = keep.reshape(nu, 16, 2).any(2)
    if mut == "pair_leak":
        xw = np.where(np.repeat(pk, 2, axis=1), xu, 0.0)
    elif mut == "pair_swap":
        xw = xw.reshape(nu, 16, 2)[:, :, ::-1].reshape(nu, 32)
    elif mut == "drop_last_pair":
        xw = xw.copy()
        for uu in np.nonzero(pk.any(1))[0]:
            p = int(np.nonzero(pk[uu])[0][-1])
            xw[uu, 2 * p: 2 * p + 2] = 0.0
    elif mut == "share_rank_ge4" and kind == SHARE:
        rank = np.cumsum(pk, 1) - 1
        xw = np.where(np.repeat(pk & (rank >= 4), 2, axis=1), 0.0, xw)
    elif mut in ("stale_slot", "dead_unit_doubles"):
        xw = xw.copy()
        base = xw.copy()
        up = UP[kind]
        for s in range(split):
            for w in range(WAVES):
                units = list(range(s + split * w, nu, split * WAVES))
                for p0 in range(0, len(units), up):
                    cur = units[p0: p0 + up]
                    if mut == "dead_unit_doubles":
                        if p0 + up >= len(units):
                            xw[cur[0]] = base[cur[0]] * (1 + up - len(cur))
                        continue
                    if p0 == 0 or kind == SHARE:
                        continue
                    maxc = max(int(pk[uu].sum()) for uu in cur)
                    for i, uu in enumerate(cur):
                        prev = units[p0 - up + i]
                        cnt, lp = int(pk[uu].sum()), np.nonzero(pk[prev])[0]
                        for r in range(cnt, min(len(lp), maxc)):
                            p = int(lp[r])
                            xw[uu, 2 * p: 2 * p + 2] += base[prev, 2 * p: 2 * p + 2]
    return xw, xw.sum(1)


def _partials(c, b, geo, x, keep, lo, hi, c0, mut):
    """[split][hi - lo] partial sums of image columns c0 + lo .. c0 + hi under keep"""
    dt, G, split = c.dt, c.G, geo["split"]
    nu, ng, n = c.Z // 32, c.Z // c.G, hi - lo
    xw, Xs = _walk(c, geo, x, keep, mut)
    cols = np.arange(c0 + lo, c0 + hi)
    qc = cols.copy()
    if mut == "nibble_order":
        qc = np.where(cols % 4 == 1, cols + 1, np.where(cols % 4 == 2, cols - 1, cols))
    Qs = b.Q[:, qc].astype(np.float64).reshape(nu, 32, n)
    odd = (cols % 2 == 1)
    S1 = np.matmul(xw[:, None, :], Qs - 8.0)[:, 0, :]
    if mut == "odd_nibble_unscaled" and dt == "fp16":   # t = A - 72 X with A = sum x (1024 + 16 q)
        Sq = np.matmul(xw[:, None, :], Qs)[:, 0, :]
        S1 = np.where(odd[None, :], 16.0 * Sq + 952.0 * Xs[:, None], S1)
    Xall = np.nan_to_num(x).reshape(nu, 32).sum(1)
    if mut == "bias_all_rows":
        b8 = np.full(n, BIAS8[dt]) if dt == "bf16" else np.where(odd, 72.0, BIAS8[dt])
        S1 = S1 + b8[None, :] * (Xs - Xall)[:, None]
    g = (32 * np.arange(nu)) // G
    if mut == "group_is_unit" and G > 32:
        g = np.minimum(np.arange(nu), ng - 1)
    if mut == "group_prev":
        g = np.maximum(g - 1, 0)
    pc = cols - c0 if mut == "seg_scale_col0" else cols
    sc, zr = b.SC[g][:, pc], b.ZR[g][:, pc]
    Xz = Xall if mut == "zero_all_rows" else (np.zeros(nu) if mut == "zero_ignored" else Xs)
    C = sc * S1 + zr * Xz[:, None]
    return np.stack([C[k::split].sum(0) for k in range(split)])


def reference(b, geo, mut=None):
    """every output buffer of the launch, whole (sentinels included), as integer words: {name: array}"""
    c = b.case
    dt, split = c.dt, geo["split"]
    x, h = _producer(c, b, mut)
    keeps = keepsets(c, b, x, mut)
    partial = []
    for s, (c0, n, _) in enumerate(c.segs):
        groups = [(0, n, keeps[s])]
        if mut == "seg_tau" and s > 0:
            groups = [(0, 128, keeps[s - 1])] + ([(128, n, keeps[s])] if n > 128 else [])
        partial.append(np.concatenate([_partials(c, b, geo, x, kp, lo, hi, c0, mut) for lo, hi, kp in groups], 1))
    P = np.concatenate(partial, 1)   # [split][N]
    b.partial = P
    out = {}

    def words16(v):
        w = np.full(len(v) + TAIL, SENT16_I, np.int16)
        fin = np.isfinite(v) & (np.abs(v) <= 65504)
        w[: len(v)] = NAN16[dt]
        r = rne16(np.where(v[fin] == 0, 0.0, v[fin]), dt)
        w[: len(v)][fin] = bits16(r, dt)
        return w

    def words32(v):
        fin = np.isfinite(v)
        w = np.full(v.shape, np.int32(0x7FC00000), np.int32)
        w[fin] = bits32(v[fin])
        return w

    if h is not None:
        out["resid_out"] = words16(h)
    if c.out == OUT_ROUNDED:
        tot = P.sum(0) if not np.isfinite(P).all() else sum_slices_f32(P[::-1] if mut == "slabs_reverse" else P)
        out["y"] = words16(tot)
        b.total = tot
        if c.twice:
            out["y2"] = np.full_like(out["y"], SENT16_I) if mut == "ticket_not_rearmed" else out["y"].copy()
    else:
        w = np.full(SLAB_ROOM * c.N + TAIL, SENT32_I, np.int32)
        if c.il:
            st = (split + 3) & ~3
            w[: c.N * st].reshape(c.N, st)[:, :split] = words32(P).T
        else:
            w[: split * c.N] = words32(P).reshape(-1)
        out["slabs"] = w
    return out


def nan_sign_dropped(words, dt):
    """the launch's words with the sign bit of a default quiet NaN cleared (IEEE 754 leaves a NaN's sign through arithmetic
    unspecified, and whether the compiler negates an operand decides it here): everything else, a NaN's payload and the
    sentinels (NaNs with a payload of their own) included, stays as it is"""
    w = words.copy()
    if w.dtype == np.int32:
        w[w == np.int32(-0x400000)] = np.int32(0x7FC00000)
    else:
        w[w == np.int16(int(NAN16[dt]) - 0x8000)] = NAN16[dt]
    return w


def rounded_from_slabs(c, slabs_words, split):
    """the 16-bit words a ROUNDED launch must give, from the fp32 slabs a SLABS launch left: summed in slice order, rounded"""
    N = c.N
    if c.il:
        st = (split + 3) & ~3
        S = slabs_words[: N * st].reshape(N, st)[:, :split].T
    else:
        S = slabs_words[: split * N].reshape(split, N)
    tot = sum_slices_f32(S.copy().view(np.float32).astype(np.float64))
    w = np.full(N + TAIL, SENT16_I, np.int16)
    w[:N] = bits16(rne16(np.where(tot == 0, 0.0, tot), c.dt), c.dt)
    return w


# ---- the ledger ---------------------------------------------------------------------------------------------------------------

def ledger(b, geo):
    """what the case executed, from the launch's report and the reference alone"""
    c = b.case
    kind, split = geo["kind"], geo["split"]
    nu = c.Z // 32
    up = UP[kind]
    keeps = keepsets(c, b, b.x)
    counts, flags = set(), set()
    passes = 0
    for si, keep in enumerate(keeps):
        pk = keep.reshape(nu, 16, 2).any(2)
        ev, od = keep.reshape(nu, 16, 2)[:, :, 0], keep.reshape(nu, 16, 2)[:, :, 1]
        cnt = pk.sum(1)
        if c.segs[si][2] < 0:
            flags.add("all_kept")
        if (np.abs(b.x[np.isfinite(b.x)]).astype(np.float32) == np.float32(b.taus[si])).any():
            flags.add("tau_tie")
        if si:
            continue
        counts |= {int(v) for v in cnt}
        for uu in np.nonzero(cnt)[0]:
            e, o = ev[uu][pk[uu]], od[uu][pk[uu]]
            flags.add("only_even" if not o.any() else ("only_odd" if not e.any() else ("both_rows" if (e & o).all() else "mixed_rows")))
        xu = np.nan_to_num(b.x).reshape(nu, 16, 2)
        if ((ev & ~od) & (xu[:, :, 1] != 0)).any() and ((od & ~ev) & (xu[:, :, 0] != 0)).any():
            flags.add("half_kept_nonzero_partner")
        for s in range(split):
            if cnt[s::split].sum() == 0:
                flags.add("empty_wg")
            for w in range(WAVES):
                units = list(range(s + split * w, nu, split * WAVES))
                if not units:
                    flags.add("idle_wave")
                    continue
                np_w = (len(units) + up - 1) // up
                passes = max(passes, np_w)
                for p0 in range(0, len(units), up):
                    cur = units[p0: p0 + up]
                    cc = [int(cnt[uu]) for uu in cur]
                    if len(cur) < up:
                        flags.add("dead_unit")
                        if p0:
                            flags.add("ragged_last_pass")
                    if kind == GROUP and len(cur) == 4:
                        if sum(v < max(cc) for v in cc) == 3:
                            flags.add("three_below_max")
                        if any({cc[i], cc[i + 1]} == {0, 16} for i in range(3)):
                            flags.add("zero_next_to_16")
                    if p0:
                        prev = units[p0 - up: p0]
                        if any(cnt[prev[i]] == 16 and 1 <= cnt[uu] <= 3 for i, uu in enumerate(cur)):
                            flags.add("stale_after_full")
    if c.layout == "round" and c.out == OUT_ROUNDED:
        tot = b.partial.sum(0)
        r, lo = rne16(tot, c.dt), rne16(tot, c.dt, mode="trunc")
        inexact = r != tot
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(tot), 1e-9))) - XG.PBITS[c.dt] + 1)
        tie = inexact & (np.abs(tot - lo) * 2 == ulp)
        if (tie & (r == lo)).any():
            flags.add("tie_down")
        if (tie & (r != lo)).any():
            flags.add("tie_up")
        if (inexact & ~tie).any():
            flags.add("next_to_tie")
    if c.G > 32 and (b.SC[1:] != b.SC[:-1]).any() and split > 1:
        flags.add("group_boundary_across_slices")   # units 32u / G - 1 and 32u / G are consecutive: different slices
    return dict(kernel="int4", kind=kind, split=split, passes=passes, mode=c.mode, G=c.G, out=OUT_NAME[c.out], il=c.il, dt=c.dt,
                counts=sorted(counts), flags=sorted(flags))


def check_claims(b, geo):
    c = b.case
    led = ledger(b, geo)
    for k, v in c.expect.items():
        assert led.get(k) == v, f"case {c.name}: the launch reports {k} = {led.get(k)!r}, the case was written for {v!r} ({geo})"
    for cl in c.claims:
        ok = (cl in led["counts"]) if isinstance(cl, int) else (cl in led["flags"])
        assert ok, f"case {c.name}: class {cl} not reached ({led['counts']}, {led['flags']})"
    return led


def probe_line(c, led, n):
    return (f"PROBE gemv_int4 {c.name} Z={c.Z} N={'+'.join(f'{n_}@{c0}' for c0, n_, _ in c.segs)} G={c.G} {c.dt} in={IN_NAME[c.mode]} "
            f"out={led['out']}{'' if c.out == OUT_ROUNDED else ('/il' if c.il else '/planar')} kind={led['kind']} split={led['split']} "
            f"passes={led['passes']} counts={','.join(str(v) for v in led['counts'])} flags={','.join(led['flags']) or '-'} "
            f"words compared = {n}, differing = 0")


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def _e(kind, split, passes):
    return dict(kind=kind, split=split, passes=passes)


WALK = ("ge", "pair_leak", "pair_swap", "drop_last_pair")
ARITH = ("nibble_order", "bias_all_rows", "zero_all_rows", "zero_ignored")
ALL_COUNTS = (0, 1, 3, 4, 5, 8, 15, 16)
ROWS = ("only_even", "only_odd", "both_rows", "half_kept_nonzero_partner")


def cases():
    """every case of tests/test_exact_gemv_int4_gpu.py, keyed by name.  expect: what the shape rule gives on a 256-CU device —
    the GPU test confirms it through the ledger."""
    C = {}

    def add(c):
        assert c.name not in C
        C[c.name] = c

    for dt in ("fp16", "bf16"):
        f16 = ("odd_nibble_unscaled",) if dt == "fp16" else ()
        # ---- 1. SHARE, one unit per wave: prescribed counts, half patterns, an empty slice; ROUNDED through tickets ----
        add(Case(f"share_counts_{dt}", dt, 4096, layout="counts", empty_slice=True, expect=_e(SHARE, 8, 1), twice=True,
                 claims=ALL_COUNTS + ROWS + ("empty_wg", "tau_tie"),
                 mutants=WALK + ARITH + f16 + ("share_rank_ge4", "ticket_not_rearmed")))
        # ---- 2. SHARE, two units per wave, ragged; the minimum Z = G ----
        add(Case(f"share_ragged_z544_{dt}", dt, 544, layout="counts", expect=_e(SHARE, 1, 1), claims=("dead_unit",) + ROWS,
                 mutants=WALK + ("dead_unit_doubles", "share_rank_ge4")))
        add(Case(f"share_ragged_z1056_{dt}", dt, 1056, layout="counts", off=3, expect=_e(SHARE, 2, 1), claims=("dead_unit",),
                 mutants=WALK + ("dead_unit_doubles", "share_rank_ge4")))
        add(Case(f"share_min_z32_g32_{dt}", dt, 32, layout="counts", off=5, expect=_e(SHARE, 1, 1), claims=("idle_wave", 5),
                 mutants=WALK + ("share_rank_ge4",)))
        add(Case(f"share_min_z256_g256_{dt}", dt, 256, G=256, layout="counts", expect=_e(SHARE, 1, 1), claims=("idle_wave", 0, 16),
                 mutants=WALK + ARITH + ("share_rank_ge4",)))
        # ---- 3. GROUP, one full pass: the four units of a pass differ ----
        add(Case(f"group_onepass_{dt}", dt, 16384, layout="counts", expect=_e(GROUP, 8, 1),
                 claims=ALL_COUNTS + ROWS + ("three_below_max", "zero_next_to_16"), mutants=WALK + ARITH + f16))
        # ---- 4. GROUP: a dead unit per pass; several passes with stale slots; a ragged last pass ----
        add(Case(f"group_dead_z12288_{dt}", dt, 12288, layout="counts", expect=_e(GROUP, 8, 1), claims=("dead_unit",),
                 mutants=WALK + ("dead_unit_doubles",)))
        add(Case(f"group_4pass_z65536_{dt}", dt, 65536, layout="stale", expect=_e(GROUP, 8, 4), claims=("stale_after_full", 16, 1, 2, 3),
                 mutants=("ge", "pair_leak", "drop_last_pair", "stale_slot")))
        add(Case(f"group_unprepared_z5120_{dt}", dt, 5120, layout="stale", prepared=False, expect=_e(GROUP, 1, 3),
                 claims=("stale_after_full", "ragged_last_pass", "dead_unit"), mutants=("ge", "stale_slot", "dead_unit_doubles", "drop_last_pair")))
        add(Case(f"group_unprepared_z16384_{dt}", dt, 16384, G=64, layout="stale", prepared=False, expect=_e(GROUP, 1, 8),
                 claims=("stale_after_full",), mutants=("ge", "stale_slot", "group_prev")))
        add(Case(f"group_unprepared_z2048_{dt}", dt, 2048, layout="counts", prepared=False, expect=_e(GROUP, 1, 1),
                 claims=("three_below_max",), mutants=WALK))
        # ---- 5. wide outputs, small split; the ticket path twice on the same workspace ----
        add(Case(f"wide_n16384_{dt}", dt, 1024, segs=[(0, 16384, 1.0)], twice=True, expect=_e(SHARE, 2, 1),
                 mutants=("ge", "pair_leak", "ticket_not_rearmed", "nibble_order")))
        add(Case(f"wide_n11008_{dt}", dt, 1024, G=128, segs=[(0, 11008, 1.0)], twice=True, expect=_e(SHARE, 2, 1),
                 mutants=("ge", "ticket_not_rearmed", "group_is_unit", "group_prev")))
        # ---- 6. group sizes, both kinds ----
        for G in (64, 128, 256):
            add(Case(f"share_g{G}_{dt}", dt, 4096, G=G, out=OUT_SLABS, layout="counts", off=G // 64, expect=_e(SHARE, 8, 1),
                     claims=("group_boundary_across_slices",), mutants=("ge", "group_is_unit", "group_prev", "zero_all_rows")))
            add(Case(f"group_g{G}_{dt}", dt, 16384, G=G, layout="counts", off=G // 64, expect=_e(GROUP, 8, 1),
                     claims=("group_boundary_across_slices",), mutants=("ge", "group_is_unit", "group_prev", "zero_ignored")))
        # ---- 7. three segments of one image (col0 0 / 128 / 384, a gap, ld > N, scale_ld > N); two segments at N 256 ----
        add(Case(f"three_segs_{dt}", dt, 2048, segs=[(0, 128, 1.0), (128, 128, -1.0), (384, 256, 2.0)], img_n=640,
                 expect=_e(SHARE, 4, 1), claims=("all_kept", "tau_tie"), mutants=("ge", "seg_tau", "seg_scale_col0", "pair_leak")))
        add(Case(f"three_segs_group_g128_{dt}", dt, 16384, G=128, segs=[(0, 128, 2.0), (128, 128, 1.0), (384, 256, -1.0)], img_n=640,
                 out=OUT_SLABS, il=0, expect=_e(GROUP, 8, 1), claims=("all_kept", "tau_tie"),
                 mutants=("ge", "seg_tau", "seg_scale_col0", "group_prev")))
        add(Case(f"two_segs_n256_{dt}", dt, 16384, segs=[(0, 128, 1.0), (128, 128, 2.0)], expect=_e(GROUP, 8, 1),
                 mutants=("ge", "seg_tau", "seg_scale_col0")))
        # ---- 8. output forms ----
        for il in (1, 0):
            nm = "il" if il else "planar"
            add(Case(f"slabs_{nm}_split1_{dt}", dt, 544, out=OUT_SLABS, il=il, layout="counts", also_rounded=True, expect=_e(SHARE, 1, 1),
                     mutants=("ge", "pair_swap")))
            add(Case(f"slabs_{nm}_split2_{dt}", dt, 1024, out=OUT_SLABS, il=il, layout="counts", also_rounded=True, expect=_e(SHARE, 2, 1),
                     mutants=("ge", "pair_swap")))
            add(Case(f"slabs_{nm}_split8_{dt}", dt, 8192, G=64, out=OUT_SLABS, il=il, layout="counts", also_rounded=True,
                     expect=_e(SHARE, 8, 1), mutants=("ge", "pair_swap", "group_prev")))
        add(Case(f"order_ticket_{dt}", dt, 4096, layout="order", expect=_e(SHARE, 8, 1), mutants=("slabs_reverse",)))
        add(Case(f"round_ties_{dt}", dt, 1024, layout="round", expect=_e(SHARE, 2, 1), claims=("tie_up", "tie_down", "next_to_tie"),
                 mutants=("ge", "zero_ignored", "drop_last_pair")))
        # ---- 9. producers ----
        for ns, Z, N, out, G, kind in ((0, 1056, 128, OUT_ROUNDED, 32, SHARE), (1, 2048, 128, OUT_SLABS, 64, SHARE),
                                       (3, 4096, 256, OUT_ROUNDED, 32, SHARE), (4, 5152, 128, OUT_SLABS, 32, SHARE),
                                       (5, 8192, 256, OUT_ROUNDED, 128, SHARE), (8, 11040, 128, OUT_SLABS, 32, GROUP),
                                       (3, 16384, 256, OUT_ROUNDED, 256, GROUP)):
            add(Case(f"norm_ns{ns}_z{Z}_{dt}", dt, Z, G=G, mode=IN_RESID_NORM, out=out, segs=[(0, N, 1.0)], nslabs=ns, row_index=(ns == 0),
                     probe_rounding=(ns >= 3), expect=_e(kind, {1056: 2, 2048: 4}.get(Z, 8), 1),
                     mutants=("ge", "pair_leak") + (("slabs_reverse", "resid_before_round") if ns >= 3 else ())
                     + (("in_slabs_4to7_dropped",) if ns > 4 else ())))
        add(Case(f"norm_eps_{dt}", dt, 8192, mode=IN_RESID_NORM, layout="eps", eps=1e-5, segs=[(0, 128, 2.5)], expect=_e(SHARE, 8, 1),
                 mutants=("normw_before_round",)))
        add(Case(f"silu_share_{dt}", dt, 4096, mode=IN_SILU_MUL, segs=[(0, 128, 32.0)], expect=_e(SHARE, 8, 1),
                 mutants=("ge", "up_offset0", "pair_leak")))
        add(Case(f"silu_group_z11008_{dt}", dt, 11008, mode=IN_SILU_MUL, out=OUT_SLABS, layout="counts", expect=_e(GROUP, 8, 1),
                 claims=("dead_unit",), mutants=("ge", "up_offset0", "drop_last_pair", "dead_unit_doubles")))
        add(Case(f"attn_ns4_hd128_share_{dt}", dt, 4096, mode=IN_ATTN_MERGE, att_ns=4, att_hd=128, att_arg=0, expect=_e(SHARE, 8, 1),
                 mutants=("ge", "empty_split", "head_off_by_one")))
        add(Case(f"attn_ns8_hd64_share_{dt}", dt, 8192, G=64, mode=IN_ATTN_MERGE, att_ns=8, att_hd=64, out=OUT_SLABS, segs=[(0, 128, 0.5)],
                 expect=_e(SHARE, 8, 1), mutants=("ge", "empty_split", "head_off_by_one")))
        add(Case(f"attn_ns8_hd128_group_{dt}", dt, 12288, mode=IN_ATTN_MERGE, att_ns=8, att_hd=128, expect=_e(GROUP, 8, 1),
                 claims=("dead_unit",), mutants=("ge", "empty_split", "head_off_by_one")))
        add(Case(f"attn_ns4_hd64_group_{dt}", dt, 16384, G=256, mode=IN_ATTN_MERGE, att_ns=4, att_hd=64, segs=[(0, 128, 0.25)],
                 expect=_e(GROUP, 8, 1), mutants=("ge", "empty_split", "head_off_by_one")))
        # ---- a NaN activation as the only kept row of a half-kept pair ----
        add(Case(f"nan_half_pair_{dt}", dt, 1024, layout="nan", expect=_e(SHARE, 2, 1), mutants=()))
    return C
