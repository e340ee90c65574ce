"""GPU: exact-integer probes of the prompt-pass and batched GEMM chain through the C ABI (teal_amd/csrc/teal_prefill.hip,
teal_amd/csrc/teal_batched.hip): teal_prefill_gemm, teal_prefill_resid_norm, teal_batched_sparse_gemm,
teal_batched_sparse_gemm_slots, teal_batched_round_rows.

The inputs are small integers (tests/exact_gemm.py), so every fp32 partial sum is exact in any order and every launch is
compared BIT FOR BIT with an integer reference: fp32 slabs as int32, 16-bit outputs as int16, the kept counts, and the
sentinel words the launch must leave alone (slabs of slices >= *split_out, slab slots >= 2 ceil(B / 2), counts of absent
segments, rows past an output's end).  What a launch must not read holds NaN or +-Inf.  No tolerance anywhere.

After each GEMM launch the test reads *split_out and has the reference classify what the case executed (phases, the last
phase's and the last chunk's rows, the size class of every (slice, phase) union list, guarded batches, segments per tile,
NP, R, producer, slot mask); each case asserts the classes it was written for, so a device whose CU count gives another split
fails loudly.  tests/test_exact_gemm_host.py shows on the CPU that a dropped, doubled or misattributed row, a stale list, a
second rounding ... changes a checked word in these very cases.  Each test prints a `PROBE` line (profiles/exact_gemm.txt).
"""
import ctypes

import numpy as np
import pytest
import torch

import exact_gemm as X
from teal_amd import _lib, runtime
from teal_amd.gpt_fast.prefill import PrefillIn
from teal_amd.kernels.sparse_gemv import batched_segs

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEMM = X.gemm_cases()
RESID = X.resid_cases()
ENTRY = {"prefill": "teal_prefill_gemm", "batched": "teal_batched_sparse_gemm", "slots": "teal_batched_sparse_gemm_slots"}


def _ready():
    L = _lib.load()
    runtime.init()
    return L


def _sent32(n):
    return torch.full((n,), int(X.SENT32_I), dtype=torch.int32, device=DEV)


def _sent16(shape):
    return torch.full(shape, int(X.SENT16_I), dtype=torch.int16, device=DEV)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _gemm_inputs(b, keep):
    """device tensors of a built case (kept alive in `keep`) and the teal_prefill_in_t"""
    c = b.case
    if c.mode == X.IN_XT:
        xt = b.xt.to(DEV)
        keep.append(xt)
        return PrefillIn(mode=X.IN_XT, xt=xt.data_ptr())
    if c.mode == X.IN_NORM:
        xt, sq, nw = b.xt.to(DEV), b.sumsq.to(DEV), b.norm_w.to(DEV)
        keep += [xt, sq, nw]
        return PrefillIn(mode=X.IN_NORM, xt=xt.data_ptr(), sumsq=sq.data_ptr(), nwg=c.nwg, norm_w=nw.data_ptr(), eps=c.eps)
    gu = b.gu.to(DEV)
    keep.append(gu)
    return PrefillIn(mode=X.IN_SILU_MUL, gu_slabs=gu.data_ptr(), gu_split=c.gu_split)


def _launch(L, b, gin, imgs, entry=None, S=None):
    """one GEMM launch into sentinel-filled buffers -> (split, slab words [16][N][R] int32, counts [16][3][9] or None)"""
    c = b.case
    entry = entry or c.entry
    S = S or c.S
    w0, w1 = imgs
    slabs = _sent32(16 * c.N * c.R)
    split = ctypes.c_int(-1)
    st = runtime.stream_ptr()
    cnt = act = None
    if entry == "prefill":
        rc = L.teal_prefill_gemm(ctypes.byref(gin), w0.data_ptr(), w0.stride(0), c.n0, _ptr(w1), w1.stride(0) if w1 is not None else 0, c.n1,
                                 slabs.data_ptr(), slabs.numel() * 4, c.Z, S, X.CODE[c.dt], ctypes.byref(split), st)
    else:
        cnt = torch.full((16 * 27,), X.SENT_CNT, dtype=torch.int32, device=DEV)
        sg = batched_segs(c.col_end, c.tau)
        args = (ctypes.byref(gin), ctypes.byref(sg), w0.data_ptr(), w0.stride(0), c.n0, _ptr(w1), w1.stride(0) if w1 is not None else 0, c.n1,
                slabs.data_ptr(), slabs.numel() * 4, c.Z, S)
        tail = (cnt.data_ptr(), X.CODE[c.dt], ctypes.byref(split), st)
        if entry == "slots":
            act = torch.tensor([c.active], dtype=torch.int32, device=DEV)
            rc = L.teal_batched_sparse_gemm_slots(*args, act.data_ptr(), *tail)
        else:
            rc = L.teal_batched_sparse_gemm(*args, *tail)
    torch.cuda.synchronize()
    assert rc == 0, (ENTRY[entry], c.name, "rc", rc)
    assert 1 <= split.value <= 16, (ENTRY[entry], c.name, "split_out", split.value)
    return split.value, slabs.cpu().numpy().reshape(16, c.N, c.R), None if cnt is None else cnt.cpu().numpy().reshape(16, 3, 9)


def _compare(what, name, got, want, axes):
    d = X.first_diff(got, want)
    if d is not None:
        n = int((np.asarray(got) != np.asarray(want)).sum())
        where = ", ".join(f"{a} {i}" for a, i in zip(axes, d))
        g, w = got[d], want[d]
        fl = ""
        if np.asarray(got).dtype == np.int32 and axes[0] == "slice" and len(axes) == 3 and what.endswith("slabs"):
            fl = f" (as fp32: got {np.array([g], np.int32).view(np.float32)[0]!r}, want {np.array([w], np.int32).view(np.float32)[0]!r})"
        raise AssertionError(f"{what} case {name}: {n} words differ; first at {where}: got {int(g):#x}, want {int(w):#x}{fl}")
    return int(np.asarray(want).size)


def _run_gemm(L, c):
    """launch, learn the split, (re)build the case for it, compare every word; -> (built case, ledger, words compared)"""
    keep = []
    b = X.build(c, c.expect_split)
    imgs = [None if t is None else t.to(DEV) for t in X.images(b)]
    split, words, cnt = _launch(L, b, _gemm_inputs(b, keep), imgs)
    if split != b.split:  # another device: the activations (and the reference) follow the split the launch reported
        b = X.build(c, split)
        imgs = [None if t is None else t.to(DEV) for t in X.images(b)]
        keep.clear()
        split2, words, cnt = _launch(L, b, _gemm_inputs(b, keep), imgs)
        assert split2 == split
    led = X.check_claims(b)
    n = _compare(f"{ENTRY[c.entry]} slabs", c.name, words, b.slabs, ("slice", "column", "slot"))
    if cnt is not None:
        n += _compare(f"{ENTRY[c.entry]} counts", c.name, cnt, b.counts, ("slice", "segment", "entry"))
    return b, led, n, imgs, keep, words


def _probe_line(c, led, n):
    return (f"PROBE gemm {ENTRY[c.entry]} {c.name} Z={c.Z} N={c.n0}+{c.n1} ld=N+{c.pad} S={c.S} {c.dt} producer={led['producer']} mask={led['mask']} "
            f"split={led['split']} phases={led['phases']} last_phase_rows={led['last_phase_rows']} last_chunk_rows={led['last_chunk_rows']} "
            f"list={led['list']} guarded={led['guarded']} segs_per_tile={led['segs_per_tile']} NP={led['NP']} R={led['R']} U={led['U']} "
            f"words compared = {n}, differing = 0")


@pytest.mark.parametrize("name", [n for n in GEMM if GEMM[n].entry != "slots"])
def test_gemm_bit_exact(name):
    L = _ready()
    c = GEMM[name]
    b, led, n, *_ = _run_gemm(L, c)
    print(_probe_line(c, led, n))


@pytest.mark.parametrize("name", [n for n in GEMM if GEMM[n].entry == "slots"])
def test_slots_bit_exact_and_equal_to_the_compacted_batch(name):
    L = _ready()
    c = GEMM[name]
    b, led, n, imgs, keep, words = _run_gemm(L, c)
    act = [s for s in range(c.S) if (c.active >> s) & 1]
    if c.active == 0:  # nothing runs: every slab word of the written pairs is zero, every count is zero
        assert not words[: b.split, :, : 2 * c.NP].any() and not b.counts[: b.split, : len(c.tau)].any()
    if act and c.mode == X.IN_XT:  # the header's promise: on the active slots, the bits of the compacted batch
        xt2 = torch.full((c.Z, 8), float("nan"), dtype=X.TDT[c.dt])
        xt2[:, : len(act)] = b.xt[:, act]
        xt2 = xt2.to(DEV)
        gin = PrefillIn(mode=X.IN_XT, xt=xt2.data_ptr())
        split2, words2, cnt2 = _launch(L, b, gin, imgs, entry="batched", S=len(act))
        assert split2 == b.split
        n += _compare("teal_batched_sparse_gemm (compacted batch) slabs", name, words2[:split2, :, : len(act)], words[:split2][:, :, act],
                      ("slice", "column", "slot"))
        n += _compare("teal_batched_sparse_gemm (compacted batch) counts", name, cnt2[:split2, : len(c.tau), : len(act)],
                      b.counts[:split2, : len(c.tau)][:, :, act], ("slice", "segment", "entry"))
    print(_probe_line(c, led, n))


@pytest.mark.parametrize("dt,N,B,split", X.ROUND_CASES)
def test_round_rows_ties(dt, N, B, split):
    L = _ready()
    parts, slabs, y = X.round_rows_case(dt, N, B, split, seed=N + B + split)
    sl = torch.from_numpy(slabs).float().to(DEV)
    assert np.array_equal(sl[:, :, :B].cpu().double().numpy(), parts[:, :, :B])
    out = _sent16((8, N))
    rc = L.teal_batched_round_rows(sl.data_ptr(), split, N, B, out.data_ptr(), X.CODE[dt], runtime.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    want = np.full((8, N), X.SENT16_I, np.int16)  # y is [B][N] with row stride N: what follows row B - 1 is not the launch's
    want.reshape(-1)[: B * N] = X.bits16(y[:, :B].T, dt).reshape(-1)
    got = out.cpu().numpy()
    n = _compare("teal_batched_round_rows y", f"{dt} N={N} B={B} split={split}", got, want, ("row", "column"))
    ties = int(((np.abs(X.sum_slices_f32(parts)) % 2 == 1)[:, :B]).sum())
    print(f"PROBE round_rows {dt} N={N} B={B} split={split} odd sums (ties below {2 * X.TIE_LO[dt]}) = {ties} "
          f"slice-order probe = {split >= 3} words compared = {n}, differing = 0")


def _run_resid(L, c, b):
    """the launch(es) of one teal_prefill_resid_norm case into sentinel-filled outputs -> dict of numpy words"""
    R, dim, T = c.R, c.dim, c.T
    keep = {}
    emb = tok = hin = None
    if c.path == "tokens":
        emb, tok = b.emb.to(DEV), torch.from_numpy(b.tokens).to(DEV)
    else:
        hin = b.ht_in.to(DEV)
    slabs = b.slabs.to(DEV) if b.slabs is not None else None
    nw = torch.from_numpy(b.norm_w).to(X.TDT[c.dt]).to(DEV)
    # every output with a guard row behind it
    ht_out = hin if c.inplace else _sent16((dim + 1, R))
    xt_out = _sent16((dim + 1, R)) if "xt" in c.outputs else None
    x_last = _sent16((dim + 8,)) if "last" in c.outputs else None
    sq = _sent32((c.nwg + 1) * R)
    rc = L.teal_prefill_resid_norm(_ptr(emb), _ptr(tok), T, _ptr(hin), _ptr(slabs), c.split, nw.data_ptr(), float(c.eps), dim,
                                   ht_out.data_ptr(), _ptr(xt_out), _ptr(x_last), sq.data_ptr(), X.CODE[c.dt], runtime.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, ("teal_prefill_resid_norm", c.name, rc)
    keep.update(ht=ht_out, sq=sq, nw=nw)
    out = {"ht": ht_out.view(torch.int16).cpu().numpy(), "sumsq": sq.cpu().numpy().reshape(c.nwg + 1, R),
           "xt": None if xt_out is None else xt_out.cpu().numpy(), "last": None if x_last is None else x_last.cpu().numpy()}
    return out, keep


def _guarded(words, rows):
    """the expected words with the sentinel guard appended"""
    w = np.asarray(words)
    sent = X.SENT32_I if w.dtype == np.int32 else X.SENT16_I
    g = np.full((rows,) + w.shape[1:], sent, w.dtype)
    return np.concatenate([w, g], 0)


def _check_resid(c, b, out):
    n = 0
    ht_want = b.ht if c.inplace else _guarded(b.ht, 1)
    n += _compare("teal_prefill_resid_norm ht_out", c.name, out["ht"], ht_want, ("column", "slot"))
    n += _compare("teal_prefill_resid_norm sumsq_scratch", c.name, out["sumsq"], _guarded(b.sumsq, 1), ("workgroup", "slot"))
    if c.kind == "norm":
        if out["xt"] is not None:
            n += _compare("teal_prefill_resid_norm xt_out", c.name, out["xt"], _guarded(b.xt, 1), ("column", "slot"))
        if out["last"] is not None:
            n += _compare("teal_prefill_resid_norm x_last", c.name, out["last"], _guarded(b.x_last, 8), ("column",))
    return n


@pytest.mark.parametrize("name", list(RESID))
def test_resid_norm_bit_exact(name):
    L = _ready()
    c = RESID[name]
    b = X.build_resid(c)
    out, _ = _run_resid(L, c, b)
    n = _check_resid(c, b, out)
    print(f"PROBE resid_norm {name} dim={c.dim} T={c.T} R={c.R} {c.dt} path={c.path} in_place={c.inplace} split={c.split} kind={c.kind} "
          f"outputs={','.join(c.outputs) or 'ht only'} eps={c.eps} nwg={c.nwg} words compared = {n}, differing = 0")


def test_resid_norm_rejections():
    L = _ready()
    dt, R = "fp16", 8
    h = torch.zeros(16640, R, dtype=torch.float16, device=DEV)
    emb = torch.zeros(4, 16640, dtype=torch.float16, device=DEV)
    tok = torch.zeros(8, dtype=torch.int32, device=DEV)
    nw = torch.ones(16640, dtype=torch.float16, device=DEV)
    sq = torch.zeros(66 * R, device=DEV)
    out = _sent16((16640, R))

    def call(emb_, tok_, hin_, dim, T=2):
        return L.teal_prefill_resid_norm(_ptr(emb_), _ptr(tok_), T, _ptr(hin_), None, 0, nw.data_ptr(), 0.0, dim, out.data_ptr(), None, None,
                                         sq.data_ptr(), 0, runtime.stream_ptr())
    assert call(None, None, h, 16385) == -3           # past the documented ceiling
    assert call(emb, tok, h, 320) == -1               # both inputs
    assert call(None, None, None, 320) == -1          # neither
    assert call(None, None, h, 320, T=17) == -3 and call(None, None, h, 320, T=0) == -3
    torch.cuda.synchronize()
    assert bool((out == int(X.SENT16_I)).all()), "a rejected call wrote"
    assert call(None, None, h, 16384) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry", ["prefill", "batched"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_chain_resid_then_norm_gemm(entry, dt):
    """the hand-over the engines use: resid_norm's FIRST launch only (no xt_out / x_last), then an IN_NORM GEMM that reads its
    ht_out and its sumsq_scratch; the slabs against the reference of the composition"""
    L = _ready()
    rc_ = RESID[f"r_norm_{dt}_d4096_T5"]
    c = X.ResidCase(rc_.name, dt, rc_.dim, rc_.T, rc_.path, rc_.split, "norm", inplace=rc_.inplace, outputs=(), eps=rc_.eps, seed=rc_.seed)
    rb = X.build_resid(c)
    out, keep = _run_resid(L, c, rb)
    n = _check_resid(c, rb, out)
    b = X.build_chain(rb, entry, 16)
    gin = PrefillIn(mode=X.IN_NORM, xt=keep["ht"].data_ptr(), sumsq=keep["sq"].data_ptr(), nwg=c.nwg, norm_w=keep["nw"].data_ptr(), eps=float(c.eps))
    imgs = [None if t is None else t.to(DEV) for t in X.images(b)]
    split, words, cnt = _launch(L, b, gin, imgs)
    if split != b.split:
        b = X.build_chain(rb, entry, split)
        imgs = [None if t is None else t.to(DEV) for t in X.images(b)]
        split, words, cnt = _launch(L, b, gin, imgs)
    led = X.check_claims(b)
    n += _compare(f"{ENTRY[entry]} slabs after teal_prefill_resid_norm", b.case.name, words, b.slabs, ("slice", "column", "slot"))
    if cnt is not None:
        n += _compare(f"{ENTRY[entry]} counts after teal_prefill_resid_norm", b.case.name, cnt, b.counts, ("slice", "segment", "entry"))
    print(_probe_line(b.case, led, n))
