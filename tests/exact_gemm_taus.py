"""Exact-integer probes of teal_batched_sparse_gemm_slot_taus (not a test file): tests/exact_gemm.py's case builder, integer
reference, ledger and numpy walk extended from one threshold per segment to the [3][8] table, segment-major and slot-minor.
Shared by tests/test_exact_gemm_taus_host.py (CPU: the probes' own power) and tests/test_exact_gemm_taus_gpu.py.

The rule under test: slot b keeps row m under segment s iff b is active and float32(|x_b[m]|) > taus[s][b].  The tables are
drawn from exact_gemm.TAUS and +inf: -inf (a slot that keeps every row, zeros included), thresholds that integer activations
tie with (|x| = 2 under tau = 2 is NOT kept) and a +inf column (an active slot that keeps nothing).  NaN stands behind the
inactive slots and in the table rows past the last segment: neither may be consulted.  segs->tau is poisoned (-inf) in every
launch: the entry must ignore it.
"""
import math

import numpy as np

import exact_gemm as X
from exact_gemm import BN, WAVES, SENT32_I, SENT_CNT

POOL = X.TAUS + (math.inf,)
MUTANTS = ("slot0_column", "next_column", "no_segment", "union_slot0", "inactive_column")


class TauCase(X.Case):
    """A `slots` case with a threshold table.  pool: what the active slots' entries are drawn from; inf_slot: an active slot
    whose whole column is +inf; fixed: {(segment, slot): entry} set by hand; dead: what stands behind the inactive slots (NaN unless the case probes the "inactive_column"
    mutant, which needs a column that WOULD keep)."""

    def __init__(self, name, dt, Z, active, pool, inf_slot=None, dead=math.nan, fixed=None, tclaims=(), tmutants=(), **kw):
        nseg = len(kw.get("col_end") or [0])
        kw.setdefault("tau", [4.0] * nseg)  # (the builder's layouts read it; the launch gets -inf in its place)
        super().__init__(name, "slots", dt, Z, active=active, **kw)
        assert set(pool) <= set(POOL)
        rng = np.random.default_rng(1000 + self.seed)
        t = np.full((3, 8), math.nan)
        for s in range(nseg):
            for b in range(8):
                t[s, b] = rng.choice(pool) if self.live[b] else dead
        if inf_slot is not None:
            assert self.live[inf_slot]
            t[:nseg, inf_slot] = math.inf
        for (s, b), v in (fixed or {}).items():
            assert s < nseg and self.live[b] and v in POOL
            t[s, b] = v
        self.taus, self.nseg = t, nseg
        self.tclaims, self.tmutants = tuple(tclaims), tuple(tmutants)


def thresholds(c, mut=None):
    """[nseg][R] the threshold slot b is compared with under segment s, per mutant"""
    t = c.taus[: c.nseg].copy()
    if mut == "slot0_column":
        t = np.repeat(t[:, :1], 8, 1)
    elif mut == "next_column":
        t = np.roll(t, -1, 1)
    elif mut == "no_segment":
        t = np.repeat(t[:1], c.nseg, 0)
    return t


def keep_masks(c, x, mut=None):
    """[nseg][Z][R] bool: float32(|x_b|) > float32(taus[s][b]) on the live slots ("inactive_column": on every slot — the staged
    activation of an inactive slot is +0, which a negative threshold keeps)"""
    live = np.ones(8, bool) if mut == "inactive_column" else np.array(c.live, bool)
    t = thresholds(c, mut)
    with np.errstate(invalid="ignore"):
        return np.stack([(np.abs(x).astype(np.float32) > t[s].astype(np.float32)[None, :]) & live[None, :] for s in range(c.nseg)])


def build(c, split):
    b = X.build(c, split)  # the inputs; its reference (one threshold per segment) is replaced
    return reference(b)


def reference(b):
    """exact_gemm.reference under the table: b.slabs, b.counts, b.keep, b.union, b.nlist"""
    c, split = b.case, b.split
    Z, N, R = c.Z, c.N, c.R
    keep = keep_masks(c, b.x)
    b.keep = keep
    sl, ph, lr = b.place
    val = np.zeros((split, N, R))
    lo = 0
    for i, hi in enumerate(c.col_end):
        xk = b.x * keep[i]
        for k in range(split):
            rows = sl == k
            val[k, lo:hi] = b.W[rows, lo:hi].T @ xk[rows]
        lo = hi
    words = np.full((16, N, R), SENT32_I, np.int32)
    words[:split, :, : 2 * c.NP] = X.bits32(val[:, :, : 2 * c.NP])
    b.val, b.slabs = val, words
    b.union = np.zeros((N // BN, Z), bool)
    b.nlist = {}
    for t in range(N // BN):
        sf, sla, _ = X.tile_segments(c, t)
        b.union[t] = keep[sf: sla + 1].any((0, 2))
        for k in range(split):
            for p in range(int(ph.max()) + 1):
                sel = (sl == k) & (ph == p)
                if sel.any():
                    b.nlist[(t, k, p)] = int(b.union[t][sel].sum())
    cnt = np.full((16, 3, 9), SENT_CNT, np.int32)
    for i in range(c.nseg):
        for k in range(split):
            rows = sl == k
            cnt[k, i, :8] = keep[i][rows].sum(0)
            cnt[k, i, 8] = keep[i][rows].any(1).sum()
    b.counts = cnt
    return b


def ledger(b):
    """exact_gemm.ledger plus what the table adds:
         kept            [nseg][8] rows each slot keeps, counted from the histogram of its |x| (not from the masks)
         solo            (segment, row) pairs kept by exactly one slot
         none_poisoned   rows some tile's union leaves out, whose weights the images hold as NaN
         nan_inactive    inactive slots (below S or not) behind an all-NaN column
         inf_columns     active slots whose column keeps nothing; neg_inf: entries that keep every row; ties: kept-or-not
                         decided by |x| == tau exactly"""
    c = b.case
    led = X.ledger(b)
    kept = np.zeros((c.nseg, 8), int)
    ties = 0
    for s in range(c.nseg):
        for sb in range(8):
            if not c.live[sb]:
                continue
            vals, n = np.unique(np.abs(b.x[:, sb]), return_counts=True)
            kept[s, sb] = sum(int(k) for v, k in zip(vals, n) if float(np.float32(v)) > float(np.float32(c.taus[s, sb])))
            ties += sum(int(k) for v, k in zip(vals, n) if v == c.taus[s, sb])
    led["kept"] = kept
    led["solo"] = int((b.keep.sum(2) == 1).sum())
    imgs = [t for t in X.images(b) if t is not None]
    nanrow = np.concatenate([np.isnan(t.double().numpy()[:, : t.shape[1] - c.pad]) for t in imgs], 1)  # [Z][N]
    led["none_poisoned"] = int(sum((~b.union[t] & nanrow[:, t * BN:(t + 1) * BN].all(1)).sum() for t in range(c.N // BN)))
    led["nan_inactive"] = [sb for sb in range(8) if not c.live[sb] and np.isnan(c.taus[:, sb]).all()]
    led["inf_columns"] = [sb for sb in range(8) if c.live[sb] and np.isposinf(c.taus[: c.nseg, sb]).all()]
    led["neg_inf"] = int(np.isneginf(c.taus[: c.nseg][:, np.array(c.live, bool)]).sum())
    led["ties"] = ties
    return led


def check_claims(b):
    """the classes of exact_gemm the case was written for, and its table claims:
         "kept": every slot keeps the prescribed rows — the reference's masks and counts agree with the histogram count;
         "solo" / "none_poisoned" / "nan_inactive" / "inf_column" / "neg_inf" / "ties": the ledger entry is non-empty"""
    c = b.case
    X.check_claims(b)
    led = ledger(b)
    for claim in c.tclaims:
        if claim == "kept":
            assert np.array_equal(b.keep.sum(1), led["kept"]), (c.name, "kept")
            assert np.array_equal(b.counts[: b.split, : c.nseg, :8].sum(0), led["kept"]), (c.name, "kept counts")
            assert not b.keep[:, :, ~np.array(c.live, bool)].any()
        elif claim == "inf_column":
            assert led["inf_columns"] and all(led["kept"][:, sb].sum() == 0 for sb in led["inf_columns"]), (c.name, claim)
        else:
            assert led[claim], (c.name, claim, led[claim])
    return led


def walk(b, mut=None):
    """exact_gemm.walk's documented row walk with the staging compare under the table: the phase's keep masks come from
    keep_masks (per mutant), the union list holds the rows with a non-zero mask ("union_slot0": the rows SOME live slot would
    keep under slot 0's column — the others' rows are lost, rows nobody keeps are streamed for nothing)."""
    c, split = b.case, b.split
    Z, N, R, U = c.Z, c.N, c.R, c.U
    live = np.array(c.live, bool)
    x_all = np.where(live[None, :], b.x, 0.0)
    keep = keep_masks(c, x_all, mut)                                        # [nseg][Z][R]
    ukeep = keep_masks(c, x_all, "slot0_column") if mut == "union_slot0" else keep
    val = np.zeros((split, N, R))
    cnt = np.full((16, 3, 9), SENT_CNT, np.int32)
    starts = [0] + c.col_end[:-1]
    pg = c.phase_rows // 16
    for t in range(N // BN):
        sf, sla, colseg = X.tile_segments(c, t)
        nls = sla - sf + 1
        report = [i for i in range(nls) if starts[sf + i] // BN == t]
        for k in range(split):
            nj = (Z // 16 - k + split - 1) // split
            acc = np.zeros((WAVES, BN, R))
            for i in report:
                cnt[k, sf + i] = 0
            for jb in range(0, nj, pg):
                nrows = min(pg, nj - jb) * 16
                r = np.arange(nrows)
                m_of = (k + split * (jb + (r >> 4))) * 16 + (r & 15)
                mk = np.stack([keep[sf + i][m_of] for i in range(nls)], 1)   # [nrows][nls][R]
                umk = np.stack([ukeep[sf + i][m_of] for i in range(nls)], 1)
                rows = np.nonzero(umk.any((1, 2)))[0]
                masks = mk[rows]
                for i in report:  # the counts are ballots over the staged masks of every row of the phase
                    cnt[k, sf + i, :8] += mk[:, i].sum(0).astype(np.int32)
                    cnt[k, sf + i, 8] += int(umk[:, i].any(1).sum())
                for w in range(WAVES):
                    er, em = rows[w::WAVES], masks[w::WAVES]
                    if len(er) == 0:
                        continue
                    mm = m_of[er]
                    for i in range(nls):
                        cs = np.nonzero(colseg == i)[0]
                        if len(cs):
                            acc[w][cs] += b.W[np.ix_(mm, t * BN + cs)].T @ np.where(em[:, i, :], x_all[mm], 0.0)
            for w in range(WAVES):
                val[k, t * BN:(t + 1) * BN] += acc[w]
    words = np.full((16, N, R), SENT32_I, np.int32)
    words[:split, :, : 2 * c.NP] = (val[:, :, : 2 * c.NP] + 0.0).astype(np.float32).view(np.int32)
    return words, cnt


def cases():
    """every case of tests/test_exact_gemm_taus_gpu.py, keyed by name: the `_slots` shapes of exact_gemm.gemm_cases() (Z = 512 with
    one, two — in one image or two — and three segments, the union-list sizes at Z = 4096, both producers) and its two-phase
    shape, Z = 33024; none larger."""
    C = {}

    def add(c):
        assert c.name not in C
        C[c.name] = c
    high = (2.0, 2.5, 3.5, 4.0)
    full = ("kept", "solo", "none_poisoned", "nan_inactive")
    for dt in ("fp16", "bf16"):
        add(TauCase(f"t_2seg_0xa5_{dt}", dt, 512, 0xA5, high, inf_slot=2, S=8, col_end=[128, 256], expect_split=2, seed=301,
                    claims={"mask": "0xa5", "segs_per_tile": 2, "NP": 4}, tclaims=full + ("inf_column", "ties"),
                    tmutants=("slot0_column", "next_column", "no_segment", "union_slot0")))
        add(TauCase(f"t_3seg_0x16_{dt}", dt, 512, 0b10110, (1.5,) + high, S=5, col_end=[96, 160, 256], expect_split=2, seed=302,
                    claims={"segs_per_tile": 3, "NP": 3}, tclaims=full + ("ties",),
                    tmutants=("slot0_column", "next_column", "no_segment", "union_slot0")))
        add(TauCase(f"t_keep_all_0x81_{dt}", dt, 512, 0x81, (-math.inf, -1.0, 0.0, 0.5), dead=-math.inf,
                    fixed={(0, 0): -math.inf, (1, 0): -1.0, (0, 7): 0.5, (1, 7): 0.0}, S=8, col_end=[128, 256],
                    expect_split=2, seed=303, claims={"mask": "0x81", "list": ["all"]}, tclaims=("kept", "solo", "neg_inf"),
                    tmutants=("inactive_column", "next_column")))
        add(TauCase(f"t_two_images_0x7e_{dt}", dt, 512, 0x7E, (2.5, 3.5, 4.0, math.inf), n0=256, n1=256, S=8, col_end=[248, 512],
                    expect_split=2, seed=304, claims={"images": 2, "segs_per_tile": 2}, tclaims=full,
                    tmutants=("slot0_column", "next_column", "no_segment", "union_slot0")))
        add(TauCase(f"t_B1_{dt}", dt, 512, 0x01, (3.5,), S=1, col_end=[256], expect_split=2, seed=305, claims={"NP": 1},
                    tclaims=("kept", "solo", "none_poisoned", "nan_inactive"), tmutants=("next_column",)))
        add(TauCase(f"t_B3_0x05_{dt}", dt, 512, 0x05, (0.0, 2.0, 3.5), dead=-1.0, S=3, col_end=[128, 256], expect_split=2, seed=306,
                    claims={"NP": 2}, tclaims=("kept", "solo"), tmutants=("inactive_column", "slot0_column")))
    add(TauCase("t_nobody_0x00", "fp16", 512, 0x00, (2.0,), S=8, col_end=[128, 256], expect_split=2, seed=307, claims={"mask": "0x00"},
                tclaims=("kept", "nan_inactive")))
    # the union-list boundary sizes: thresholds 2 and 2.5 keep the same integers, so the layout's sizes hold under the table
    add(TauCase("t_sizes_0xA5", "fp16", 4096, 0xA5, (2.0, 2.5), S=8, col_end=[256], tau=[2.0], layout="sizes", expect_split=16, seed=120,
                claims={"list": ["0", "<16", "16U", "all"], "mask": "0xa5"}, tclaims=("kept", "nan_inactive", "none_poisoned")))
    # the second staging phase: the parked thresholds are fetched again
    add(TauCase("t_two_phase_0x16", "bf16", 33024, 0b10110, (2.5, 3.5, 4.0), S=5, col_end=[256], expect_split=16, seed=308,
                claims={"split": 16, "phases": 2, "last_phase_rows": [16], "list": ["phase2 listed"]}, tclaims=full,
                tmutants=("slot0_column", "next_column", "union_slot0")))
    add(TauCase("t_silu_0x16", "bf16", 512, 0b10110, (0.0, 2.5, 4.0), inf_slot=2, S=5, col_end=[256], mode=X.IN_SILU_MUL, gu_split=4,
                expect_split=2, seed=309, claims={"producer": "silu_mul"}, tclaims=("kept", "nan_inactive", "inf_column", "ties"),
                tmutants=("slot0_column", "next_column")))
    add(TauCase("t_norm_0x81", "fp16", 512, 0x81, (0.5, 1.5, 2.0, 2.5, 3.5, 4.0), S=8, col_end=[128, 256], mode=X.IN_NORM, eps=1e-5, nwg=2,
                expect_split=2, seed=310, claims={"producer": "norm"}, tclaims=("kept", "solo", "nan_inactive"),
                tmutants=("slot0_column", "next_column", "no_segment", "union_slot0")))
    return C
