"""GPU: the epilogues' row-group reduction (teal_amd/csrc/teal_common.h: row_reduce_scatter, two accumulators per
v_permlane16_swap / v_permlane32_swap) against the `__shfl_xor` butterfly it replaces, on raw bit patterns through the
diagnostics entry point teal_probe_row_reduce.  Bit for bit, no tolerance:

  * lane 16 r + i (i < lanes per row) must hold in `lo` what the butterfly leaves in lane i for accumulator r, in `hi` for 4 + r;
  * powers of two that differ per (lane, accumulator) and whose sums are exact, so that a total names its terms: a
    mis-routed lane changes a sum;
  * random finite values (the order of the three or two adds shows in the last bit);
  * one NaN with a payload, +inf, -inf, -0.0 moved through every (lane, accumulator) position in turn.
"""
import numpy as np
import pytest
import torch

from teal_amd import _lib, runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _probe(pat, lpr):
    """pat: uint32 [nwaves, 64, 8] -> (scatter [nwaves, 64, 2], shuffle [nwaves, 64, 8]) as uint32 numpy"""
    runtime.init()
    D = _lib.load_diag()
    nw = pat.shape[0]
    x = torch.from_numpy(pat.view(np.int32).copy()).to(DEV)
    sc = torch.full((nw, 64, 2), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    sh = torch.full((nw, 64, 8), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rc = D.teal_probe_row_reduce(x.data_ptr(), sc.data_ptr(), sh.data_ptr(), nw, lpr, runtime.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return sc.cpu().numpy().view(np.uint32), sh.cpu().numpy().view(np.uint32)


def _check(pat, lpr, what):
    sc, sh = _probe(pat, lpr)
    r, i = np.arange(4)[:, None], np.arange(lpr)[None, :]
    lanes = (16 * r + i).reshape(-1)            # the lanes that hold totals
    src = np.broadcast_to(i, (4, lpr)).reshape(-1)
    acc = np.broadcast_to(r, (4, lpr)).reshape(-1)
    lo, hi = sc[:, lanes, 0], sc[:, lanes, 1]
    want_lo, want_hi = sh[:, src, acc], sh[:, src, acc + 4]
    for name, got, want in (("lo", lo, want_lo), ("hi", hi, want_hi)):
        bad = np.argwhere(got != want)
        assert bad.size == 0, (f"{what}, {lpr} lanes per row, {name}: {len(bad)} words differ; first in wave {bad[0][0]}, lane "
                               f"{lanes[bad[0][1]]}: got {int(got[tuple(bad[0])]):#010x}, want {int(want[tuple(bad[0])]):#010x}")
    return sc, sh


def _f2u(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("lpr", (8, 16))
def test_powers_of_two_name_their_lanes(lpr):
    """lane l, accumulator j carry 2^(3 g + j mod 3 + 12 (i mod 2)) with g = l div lpr the row group and i = l mod lpr the
    column group (wave w: times 1 + w): a total is a sum of distinct powers of two that names the row groups it was made of and
    differs between neighbouring column groups and accumulators.  The butterfly's totals are checked against the exact sum as
    well, so the reference form is pinned too"""
    pat = np.zeros((8, 64, 8), np.float32)
    lane, j = np.arange(64)[:, None], np.arange(8)[None, :]
    expo = (lane // lpr) * 3 + (j % 3) + 12 * ((lane % lpr) % 2)     # distinct inside every (column group, accumulator mod 3) sum
    full = np.ldexp(np.float32(1.0), expo).astype(np.float32)
    for w in range(8):
        pat[w] = full * (1.0 + w)          # eight scalings of the same pattern: still exact
    sc, sh = _check(pat.view(np.uint32), lpr, "powers of two")
    want = pat.reshape(8, 64 // lpr, lpr, 8).sum(1)                  # exact: < 2^24 distinct bits
    assert np.array_equal(sh.view(np.float32)[:, :lpr, :], want)


@pytest.mark.parametrize("lpr", (8, 16))
def test_distinct_power_per_lane_and_accumulator(lpr):
    """one wave per accumulator pair (j, 4 + j): lane l carries 2^(l mod 20) * (1 + l div 20) there and zero elsewhere — a
    distinct value per lane whose sums over 64 / lpr lanes stay exact; a lane routed to another row group changes a total"""
    pat = np.zeros((4, 64, 8), np.float32)
    lane = np.arange(64)
    val = np.ldexp(np.float32(1.0), lane % 20).astype(np.float32) * (1 + lane // 20).astype(np.float32)
    for w in range(4):
        pat[w, :, w] = val
        pat[w, :, 4 + w] = -val[::-1]
    sc, sh = _check(pat.view(np.uint32), lpr, "distinct powers")
    want = pat.reshape(4, 64 // lpr, lpr, 8).sum(1)
    assert np.array_equal(sh.view(np.float32)[:, :lpr, :], want)


@pytest.mark.parametrize("lpr", (8, 16))
def test_random_finite_values(lpr):
    rng = np.random.default_rng(20 + lpr)
    pat = (rng.standard_normal((64, 64, 8)) * np.exp2(rng.integers(-20, 20, (64, 64, 8)))).astype(np.float32)
    _check(pat.view(np.uint32), lpr, "random finite values")


@pytest.mark.parametrize("lpr", (8, 16))
@pytest.mark.parametrize("special", ("nan_payload", "+inf", "-inf", "-0.0"))
def test_special_value_in_every_position(lpr, special):
    """512 waves: the special value sits in (lane, accumulator) = (w div 8, w mod 8) of wave w, every other word a random finite
    value (for -0.0 the wave holds -0.0 everywhere and one +0.0: the total is -0.0 only where every term is)."""
    rng = np.random.default_rng(7)
    nw = 64 * 8
    if special == "-0.0":
        pat = np.full((nw, 64, 8), 0x80000000, np.uint32)            # all -0.0 ...
        word = np.uint32(0x00000000)                                   # ... and one +0.0: that total alone is +0.0
    else:
        pat = _f2u(rng.standard_normal((nw, 64, 8)).astype(np.float32)).copy()
        word = {"nan_payload": np.uint32(0x7FC12345), "+inf": np.uint32(0x7F800000), "-inf": np.uint32(0xFF800000)}[special]
    w = np.arange(nw)
    pat[w, w // 8, w % 8] = word
    sc, sh = _check(pat, lpr, special)
    if special == "nan_payload":   # the probe has power: the NaN reaches exactly one column group of one accumulator
        nan = np.isnan(sh.view(np.float32)[:, :lpr, :])
        assert np.array_equal(nan.sum((1, 2)), np.ones(nw, np.int64))
