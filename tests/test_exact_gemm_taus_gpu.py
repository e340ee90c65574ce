"""GPU: exact-integer probes of teal_batched_sparse_gemm_slot_taus through the C ABI (teal_amd/csrc/teal_batched.hip).

Every slab word and every count word of the launch is compared BIT FOR BIT with the integer reference of
tests/exact_gemm_taus.py: slot b keeps row m under segment s iff its bit of the active word is set and
float32(|x_b[m]|) > taus[s][b].  The buffers start out as sentinels (slabs of slices >= *split_out, slots >= 2 ceil(B / 2) and
counts of absent segments must still hold them), what the launch must not read holds NaN or +-Inf — weight rows outside a
tile's union, the inactive slots' hand-over AND their threshold columns, the table rows past the last segment — and segs->tau
is -inf in every launch: consulted, it would keep every row.  With every column equal to segs->tau the outputs are those of
teal_batched_sparse_gemm_slots, word for word.  tests/test_exact_gemm_taus_host.py shows on the CPU that a wrong column, a wrong
segment row, a union under one slot's column or a consulted inactive column changes a checked word in these very cases.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import exact_gemm as X
import exact_gemm_taus as XT
from teal_amd import _lib, runtime
from teal_amd.gpt_fast.prefill import PrefillIn
from teal_amd.kernels.sparse_gemv import batched_segs
from test_exact_gemm_gpu import _compare, _gemm_inputs, _probe_line, _ptr, _sent32

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = XT.cases()
SLOTS = {n: c for n, c in X.gemm_cases().items() if c.entry == "slots"}
NAME = "teal_batched_sparse_gemm_slot_taus"


def _ready():
    L = _lib.load()
    runtime.init()
    return L


def _launch(L, c, gin, imgs, taus, seg_tau, entry=NAME, expect_rc=0):
    """one launch into sentinel-filled buffers -> (split, slab words [16][N][8] int32, counts [16][3][9]); taus: a device tensor"""
    w0, w1 = imgs
    slabs = _sent32(16 * c.N * c.R)
    cnt = torch.full((16 * 27,), X.SENT_CNT, dtype=torch.int32, device=DEV)
    split = ctypes.c_int(-1)
    sg = batched_segs(c.col_end, seg_tau)
    act = torch.tensor([c.active], dtype=torch.int32, device=DEV)
    args = (ctypes.byref(gin), ctypes.byref(sg), w0.data_ptr(), w0.stride(0), c.n0, _ptr(w1), w1.stride(0) if w1 is not None else 0, c.n1,
            slabs.data_ptr(), slabs.numel() * 4, c.Z, c.S, act.data_ptr())
    tail = (cnt.data_ptr(), X.CODE[c.dt], ctypes.byref(split), runtime.stream_ptr())
    if entry == NAME:
        rc = L.teal_batched_sparse_gemm_slot_taus(*args, _ptr(taus) if isinstance(taus, torch.Tensor) else taus, *tail)
    else:
        rc = L.teal_batched_sparse_gemm_slots(*args, *tail)
    torch.cuda.synchronize()
    assert rc == expect_rc, (entry, c.name, "rc", rc)
    return split.value, slabs.cpu().numpy().reshape(16, c.N, c.R), cnt.cpu().numpy().reshape(16, 3, 9)


def _table(t):
    return torch.from_numpy(np.asarray(t, np.float32)).to(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_slot_taus_bit_exact(name):
    L = _ready()
    c = CASES[name]
    poison = [-math.inf] * c.nseg
    b = XT.build(c, c.expect_split)
    keep = []
    imgs = [None if t is None else t.to(DEV) for t in X.images(b)]
    split, words, cnt = _launch(L, c, _gemm_inputs(b, keep), imgs, _table(c.taus), poison)
    if split != b.split:  # another device: the activations (and the reference) follow the split the launch reported
        b = XT.build(c, split)
        keep.clear()
        imgs = [None if t is None else t.to(DEV) for t in X.images(b)]
        split2, words, cnt = _launch(L, c, _gemm_inputs(b, keep), imgs, _table(c.taus), poison)
        assert split2 == split
    led = XT.check_claims(b)
    n = _compare(f"{NAME} slabs", name, words, b.slabs, ("slice", "column", "slot"))
    n += _compare(f"{NAME} counts", name, cnt, b.counts, ("slice", "segment", "entry"))
    print(_probe_line(c, led, n).replace("teal_batched_sparse_gemm_slots", NAME) +
          f" kept={led['kept'].tolist()} solo={led['solo']} none_poisoned={led['none_poisoned']} nan_inactive={led['nan_inactive']}")


@pytest.mark.parametrize("name", list(SLOTS))
def test_equal_columns_are_the_slots_launch_word_for_word(name):
    L = _ready()
    c = SLOTS[name]
    b = X.build(c, c.expect_split)
    keep = []
    imgs = [None if t is None else t.to(DEV) for t in X.images(b)]
    gin = _gemm_inputs(b, keep)
    split, words, cnt = _launch(L, c, gin, imgs, None, c.tau, entry="slots")
    if split != b.split:  # (the images' poisoned rows follow the split through the layout: rebuild, as the exact test does)
        b = X.build(c, split)
        keep.clear()
        imgs = [None if t is None else t.to(DEV) for t in X.images(b)]
        gin = _gemm_inputs(b, keep)
        split, words, cnt = _launch(L, c, gin, imgs, None, c.tau, entry="slots")
    t = np.full((3, 8), math.nan, np.float32)
    t[: len(c.tau)] = np.array(c.tau, np.float32)[:, None]
    split2, words2, cnt2 = _launch(L, c, gin, imgs, _table(t), [-math.inf] * len(c.tau))
    assert split2 == split
    n = _compare(f"{NAME} slabs against teal_batched_sparse_gemm_slots", name, words2, words, ("slice", "column", "slot"))
    n += _compare(f"{NAME} counts against teal_batched_sparse_gemm_slots", name, cnt2, cnt, ("slice", "segment", "entry"))
    n += _compare(f"{NAME} slabs", name, words2, b.slabs, ("slice", "column", "slot"))
    print(f"PROBE {NAME} == teal_batched_sparse_gemm_slots {name} split={split} words compared = {n}, differing = 0")


def test_refusals_write_nothing():
    L = _ready()
    c = CASES["t_2seg_0xa5_fp16"]
    b = XT.build(c, c.expect_split)
    keep = []
    imgs = [None if t is None else t.to(DEV) for t in X.images(b)]
    gin = _gemm_inputs(b, keep)
    poison = [-math.inf] * c.nseg
    big = torch.zeros(64, dtype=torch.float32, device=DEV)
    assert big.data_ptr() % 32 == 0
    big[4:28] = _table(c.taus).view(-1)

    def untouched(out):
        split, words, cnt = out
        assert split == -1 and (words == X.SENT32_I).all() and (cnt == X.SENT_CNT).all()
    untouched(_launch(L, c, gin, imgs, None, poison, expect_rc=-1))                       # taus null: TEAL_ERR_ARG
    for off in (1, 2, 4):                                                                 # 4, 8 and 16 bytes off a 32-byte boundary
        untouched(_launch(L, c, gin, imgs, big[off:], poison, expect_rc=-4))              # TEAL_ERR_ALIGN
    # the `_slots` refusals, unchanged: a null active word, B outside 1..8, a segment list that does not end at n0 + n1
    sg = batched_segs(c.col_end, poison)
    slabs, split = _sent32(16 * c.N * 8), ctypes.c_int(-1)
    args = lambda B, act, segs: (ctypes.byref(gin), ctypes.byref(segs), imgs[0].data_ptr(), imgs[0].stride(0), c.n0, None, 0, 0,  # noqa: E731
                                 slabs.data_ptr(), slabs.numel() * 4, c.Z, B, act, big.data_ptr(), None, X.CODE[c.dt], ctypes.byref(split),
                                 runtime.stream_ptr())
    act = torch.tensor([c.active], dtype=torch.int32, device=DEV)
    assert L.teal_batched_sparse_gemm_slot_taus(*args(8, None, sg)) == -1
    assert L.teal_batched_sparse_gemm_slot_taus(*args(9, act.data_ptr(), sg)) == -3
    assert L.teal_batched_sparse_gemm_slot_taus(*args(8, act.data_ptr(), batched_segs([128, 248], poison))) == -3
    torch.cuda.synchronize()
    assert bool((slabs == int(X.SENT32_I)).all()) and split.value == -1
    # and the aligned table 16 floats into the buffer is accepted: the same words as the table on its own
    big[8:32] = _table(c.taus).view(-1)
    split1, words1, cnt1 = _launch(L, c, gin, imgs, big[8:], poison)
    assert X.first_diff(words1, b.slabs) is None and X.first_diff(cnt1, b.counts) is None
