"""GPU: the reduce-and-store tail of the decode launches, bit for bit — the row-group reduce-scatter, the LDS deposit, the
fixed-order cross-wave sum and the hoisted RoPE / KV-append epilogue of the lean GEMV kernel (teal_amd/csrc/teal_gemv_fast.h), of
the general one (teal_gemv_kernel.h) and of the split-KV attention kernels (teal_attention.hip).

GEMV: tests/exact_gemv.py's cases, launch and integer reference (through tests/test_exact_gemv_gpu.py's _run), with the weight
values replaced: row r carries +-2^(r mod E) in every column, so that the partial of each row group of a wave, and of each wave,
is a different sum of powers of two and a total that took a partial from the wrong lane, LDS slot or wave differs from the
reference.  E is the largest modulus the format and the exactness bound allow: 2^(r mod 20) is not a number of fp16 from 2^16 on,
and 1024 kept rows of it times |x| <= 4 pass 2^24; E = 14 keeps sum |w| |x| below 2^24 up to Z = 2048 (exact_gemv asserts the
bound when it builds the case), int8 weights take E = 7, the 16-bit outputs of the RoPE epilogue E = 4.  PAIR needs its gate sums steered onto {16, 24, 32}, which the correction rows
can do only for small sums: the PAIR cases keep exact_gemv's own weights (integers in [-3, 3]).

Attention: q = 0, so every score is 0, m = 0, every probability exp(0) = 1, l = the number of rows of the split and o a plain
sum of V rows; V[row][d] = 2^((5 row + 3 d) mod 18 - 9), a pattern in which neighbouring rows, columns and 16-byte slices all
differ and whose sums over a split's rows (at most 6 equal powers) are exact in fp32.  The partials {m, l, o} of every (head,
split) are compared bit for bit with the host sum over the rows the split owns (row groups of `threads / 64 * 64 / (head_dim /
8)` rows dealt round-robin to the splits).
"""
import ctypes

import numpy as np
import pytest
import torch

import exact_gemv as X
import test_exact_gemv_gpu as G
from teal_amd import _lib, runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- GEMV ------------------------------------------------------------------------------------------------------------------------

def _pow2_rows(modulus):
    def weights(rng, Z, N):
        sign = rng.choice([-1.0, 1.0], (Z, N))
        return (sign * np.exp2(np.arange(Z) % modulus)[:, None]).astype(np.float32)
    return weights


def _gemv_cases():
    """fp32 outputs wherever the kernel offers one (a 16-bit output would round the low powers away and, in fp16, overflow): the
    lean kernel's unrounded slice-order sum (TEAL_OUT_SLAB_SUM) and its slabs, the general kernel's planar slabs.  The lean
    kernel takes split 2 from two rounds of 16 chunks on (Z = 2048); forced on Z = 64 / 1024 it is the general kernel's
    even-shares rule that runs, in both builds — the reference follows the geometry the launch reports."""
    C = []
    for dt in ("fp16", "bf16"):
        for N, lpr in ((64, 8), (128, 16)):
            for Z in (64, 1024):
                C.append(X.Case(f"lean_z{Z}_n{N}_split1_{dt}", dt, Z, out=X.OUT_SLAB_SUM, lib=(lpr, 1), segs=[(N, 1.0)],
                                expect=dict(kernel="lean", lpr=lpr, split=1)))
                for split in (1, 2):
                    C.append(X.Case(f"general_z{Z}_n{N}_split{split}_{dt}", dt, Z, out=X.OUT_SLABS, il=0, lib=(lpr, split), fast=0,
                                    segs=[(N, 1.0)], expect=dict(kernel="general", lpr=lpr, split=split)))
                C.append(X.Case(f"forced_z{Z}_n{N}_split2_{dt}", dt, Z, out=X.OUT_SLABS, lib=(lpr, 2), segs=[(N, 1.0)],
                                expect=dict(lpr=lpr, split=2)))
            C.append(X.Case(f"lean_z2048_n{N}_split2_{dt}", dt, 2048, out=X.OUT_SLABS, lib=(lpr, 2), segs=[(N, 1.0)],
                            expect=dict(kernel="lean", lpr=lpr, split=2)))
            C.append(X.Case(f"lean_z2048_n{N}_split2_ticket_{dt}", dt, 2048, out=X.OUT_SLAB_SUM, lib=(lpr, 2), segs=[(N, 1.0)],
                            expect=dict(kernel="lean", lpr=lpr, split=2)))
        for Z in (64, 1024):
            C.append(X.Case(f"w8_lean_z{Z}_{dt}", dt, Z, w8=True, out=X.OUT_SLAB_SUM, lib=(16, 1), segs=[(128, 1.0)], xmax=3,
                            expect=dict(kernel="lean", lpr=16, w8=True)))
            C.append(X.Case(f"w8_general_z{Z}_{dt}", dt, Z, w8=True, out=X.OUT_SLABS, il=0, lib=(16, 1), fast=0, segs=[(128, 1.0)], xmax=3,
                            expect=dict(kernel="general", lpr=16, w8=True)))
        for fast in (1, 0):
            C.append(X.Case(f"pair_{'lean' if fast else 'general'}_{dt}", dt, 1024, mode=X.IN_RESID_NORM, out=X.OUT_PAIR_SILU, lib=(8, 1),
                            fast=fast, segs=[(128, 1.0), (128, 2.0)], steer=True, nw_kind="sign",
                            expect=dict(kernel="lean" if fast else "general", lpr=8, pair=True)))
        # RoPE / KV-append epilogue (product geometry: the fused epilogue refuses forced ones): grouped-query widths at both head
        # sizes, first and last cache row.  16-bit outputs: modulus 4 keeps every sum inside fp16
        for hd, q, kv in ((64, 6656, 1664), (128, 8192, 1024)):
            for pos in (0, 5):
                C.append(X.Case(f"rope_hd{hd}_pos{pos}_{dt}", dt, 1024, mode=X.IN_RESID_NORM, out=X.OUT_QKV_ROPE,
                                segs=[(q, 1.0), (kv, 2.0), (kv, 0.5)], nslabs=2, nw_kind="sign", rope=dict(hd=hd, max_seq=6, pos=pos),
                                expect=dict(kernel="lean", rope=True, split=1)))
    return {c.name: c for c in C}


def _modulus(c):
    return 7 if c.w8 else (4 if c.out == X.OUT_QKV_ROPE else 14)


GEMV = _gemv_cases()


@pytest.mark.parametrize("name", list(GEMV))
def test_gemv_tail_bit_exact(name, monkeypatch):
    c = GEMV[name]
    if not c.pair:
        monkeypatch.setattr(X, "_weights", _pow2_rows(_modulus(c)))
    # (exact_gemv.build takes a "random" layout's geometry from nowhere but the launch's report)
    monkeypatch.setattr(X, "geometry", lambda cc, desc=None, ns=None, _g=X.geometry: _g(cc, desc, ns) if desc is not None else
                        dict(kernel="lean", lpr=cc.lib[0] if cc.lib else 8, split=cc.lib[1] if cc.lib else 1, kr=None, exact=False,
                             rope=False, w8=cc.w8, pair=cc.pair, mode=cc.mode))
    led, n, desc = G._run(c)
    assert n > 0
    if c.out == X.OUT_QKV_ROPE:
        assert led["rope"] and led["split"] == 1
    print("\n" + X.probe_line(c, led, n))
    print(f"LEDGER {c.name}: {desc}")


# ---- attention -------------------------------------------------------------------------------------------------------------------

POSITIONS = (0, 3, 4, 15, 16, 17, 63, 64, 65, 255)
#        name        (n_head, n_kv, hd, max_seq)  entry     threads  grouped
ATT = {"waves4_hd128": ((4, 4, 128, 256), "split", 256, 0),
       "waves4_hd64": ((4, 2, 64, 256), "split", 256, 0),
       "waves16_hd128": ((2, 2, 128, 2048), "split", 1024, 0),
       "waves16_hd64": ((4, 4, 64, 2048), "split", 1024, 0),
       "roped_waves4_hd128": ((4, 2, 128, 256), "roped", 256, 0),
       "roped_waves16_hd64": ((4, 4, 64, 2048), "roped", 1024, 0),
       "gqa8_hd128": ((8, 1, 128, 2048), "split", 512, 1),
       "gqa4_hd64": ((8, 2, 64, 4096), "split", 512, 1)}


def _v_pattern(n_kv, rows, hd):
    r, d, k = np.arange(rows)[None, :, None], np.arange(hd)[None, None, :], np.arange(n_kv)[:, None, None]
    return np.exp2((5 * r + 3 * d + 7 * k) % 18 - 9).astype(np.float64)


@pytest.mark.parametrize("dt", (torch.float16, torch.bfloat16), ids=("fp16", "bf16"))
@pytest.mark.parametrize("nsplit", (4, 8))
@pytest.mark.parametrize("name", list(ATT))
def test_attention_partials_bit_exact(name, nsplit, dt):
    (n_head, n_kv, hd, S), entry, threads, grouped = ATT[name]
    L = _lib.load()
    runtime.init()
    out = (ctypes.c_int * 4)()
    assert L.teal_decode_attention_split_plan(n_head, n_kv, hd, S, nsplit, int(entry == "roped"), out) == 0
    assert (out[0], out[1]) == (grouped, threads), (name, list(out))    # the instantiation the case was written for
    step = threads // 64 * (64 // (hd // 8))
    rep = n_head // n_kv
    rows = max(POSITIONS) + 1
    V = _v_pattern(n_kv, rows, hd)
    code, st = runtime.dtype_code(dt), runtime.stream_ptr()
    rope = torch.zeros(S, hd // 2, 2, dtype=dt, device=DEV)
    rope[..., 0] = 1.0
    worst = 0
    for pos in POSITIONS:
        kc = torch.full((n_kv, S, hd), float("nan"), dtype=dt, device=DEV)
        vc = torch.full((n_kv, S, hd), float("nan"), dtype=dt, device=DEV)
        kc[:, :rows] = 0.25                                      # any finite key: q = 0 makes every score 0
        vc[:, :rows] = torch.from_numpy(V).to(dt).to(DEV)
        n = pos + 1
        if entry == "split":                                      # the kernel appends row pos itself from q | k | v
            kc[:, pos], vc[:, pos] = float("nan"), float("nan")
            qkv = torch.cat([torch.zeros(n_head * hd), torch.full((n_kv * hd,), 0.25), torch.from_numpy(V[:, pos].reshape(-1)).float()]).to(dt).to(DEV)
        else:
            qkv = torch.zeros(n_head * hd, dtype=dt, device=DEV)
        p = torch.tensor([pos], device=DEV, dtype=torch.int32)
        part = torch.full((n_head, nsplit, hd + 2), float("nan"), device=DEV, dtype=torch.float32)
        if entry == "split":
            rc = L.teal_decode_attention_split(qkv.data_ptr(), rope.data_ptr(), p.data_ptr(), kc.data_ptr(), vc.data_ptr(), None, None, 0.0,
                                               n_head, n_kv, hd, S, nsplit, part.data_ptr(), part.numel() * 4, code, st)
        else:
            rc = L.teal_decode_attention_split_roped(qkv.data_ptr(), p.data_ptr(), kc.data_ptr(), vc.data_ptr(), None, None, 0.0,
                                                     n_head, n_kv, hd, S, nsplit, part.data_ptr(), part.numel() * 4, code, None, 0, st)
        torch.cuda.synchronize()
        assert rc == 0, (name, pos, rc)
        got = part.cpu().numpy()
        want = np.zeros((n_head, nsplit, hd + 2), np.float64)
        owner = (np.arange(n) // step) % nsplit
        for h in range(n_head):
            for sp in range(nsplit):
                mine = owner == sp
                want[h, sp, 0] = 0.0 if mine.any() else -np.inf
                want[h, sp, 1] = float(mine.sum())
                want[h, sp, 2:] = V[h // rep, :n][mine].sum(0)
        assert float(np.abs(want[..., 2:]).max()) < 2.0 ** 14 and np.array_equal(want.astype(np.float32).astype(np.float64), want)
        wb, gb = want.astype(np.float32).view(np.uint32), got.view(np.uint32)
        bad = np.argwhere(wb != gb)
        assert bad.size == 0, (f"{name} nsplit {nsplit} pos {pos}: {len(bad)} words differ; first at (head, split, word) {tuple(bad[0])}: "
                               f"got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")
        worst += wb.size
        if entry == "split":                                      # the appended rows: k unrotated (cos 1, sin 0), v as given
            assert bool((kc[:, pos] == 0.25).all()) and torch.equal(vc[:, pos].double().cpu(), torch.from_numpy(V[:, pos]))
    print(f"\nPROBE exit_audit attention {name} nsplit={nsplit} words compared = {worst}, differing = 0")
