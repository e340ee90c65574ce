"""GPU: exact-integer probes of the fused decode GEMV, teal_fused_gemv, through the C ABI — every input producer (PLAIN,
RESID_NORM, SILU_MUL +- gate_activated, MASKED, ATTN_MERGE), every output form (ROUNDED +- act_seg0 +- split-K by arrival
tickets, SLABS, SLAB_SUM, PAIR_SILU +- mask_out, QKV_ROPE), the lean kernel (teal_amd/csrc/teal_gemv_fast.h) and the general
one (teal_gemv_kernel.h), 16-bit and int8 weights, fp16 and bf16.

The inputs are small integers (tests/exact_gemv.py), so every fp32 partial sum is exact in any order and every output buffer is
compared WHOLE and BIT FOR BIT with an integer reference: 16-bit vectors as int16, fp32 slabs as int32, keep masks as int64,
the KV-cache rows, and the sentinel words behind every output, in the slab padding lanes and in the slabs no slice writes.
What a launch must not read holds NaN (int8 images: +127 / -128).  No tolerance anywhere.

The production geometry runs through the product library; forced geometries and the general kernel (fast = 0) through the
diagnostics build (helpers.lib_for).  After each launch the test reads *nslabs_out and teal_gemv_out.desc; the reference runs at
the geometry the launch REPORTED, and the ledger built from it is asserted against what the case was written for — a case
that silently falls from the lean to the general kernel, or gets another split, fails.  tests/test_exact_gemv_host.py shows on
the CPU that a dropped or doubled row, a neighbour's threshold, >= for >, a doubled rounding, slabs summed out of order ...
change a compared word in these very cases.  Each test prints a `PROBE` line (profiles/exact_gemv.txt).
"""
import ctypes

import numpy as np
import pytest
import torch

import exact_gemv as X
import helpers
from teal_amd import runtime
from teal_amd.gpt_fast.engine import GemvIn, GemvOut

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = X.cases()
SENT = {"i16": (torch.int16, int(X.SENT16_I)), "i32": (torch.int32, int(X.SENT32_I)), "i64": (torch.int64, int(X.SENT64_I))}


def _sent(kind, n):
    dt, v = SENT[kind]
    return torch.full((n,), v, dtype=dt, device=DEV)


def _launch(L, c, b, ws, mask_tau=None):
    """one teal_fused_gemv launch into sentinel-filled buffers -> (geometry reported, {buffer name: words})"""
    keep = {k: t.to(DEV) for k, t in b.inputs.items()}
    imgs = [t.to(DEV) for t in b.images_t]
    scales = [t.to(DEV) for t in b.scale_t] if c.w8 else None
    Ntot = sum(n for n, _ in c.segs)
    bufs = {}
    gin = GemvIn(mode=c.mode)
    if c.mode == X.IN_RESID_NORM:
        gin.resid_in, gin.norm_weight, gin.eps = keep["resid"].data_ptr(), keep["norm_w"].data_ptr(), c.eps
        if c.row_index:
            gin.row_index = keep["row_index"].data_ptr()
        if c.nslabs:
            gin.slabs, gin.nslabs, gin.slabs_interleaved = keep["slabs_in"].data_ptr(), c.nslabs, c.slabs_il
        if c.resid_out:
            bufs["resid_out"] = _sent("i16", c.Z + X.TAIL)
            gin.resid_out = bufs["resid_out"].data_ptr()
    else:
        gin.x = keep["x"].data_ptr()
        if c.mode == X.IN_MASKED:
            gin.masks = keep["masks"].data_ptr()
        if c.mode == X.IN_ATTN_MERGE:
            gin.att_head_dim, gin.att_nsplit = c.att_hd, c.att_ns
        gin.gate_activated = c.gate_activated
    gout = GemvOut()
    gout.nseg, gout.mode = len(c.segs), c.out
    if c.out in (X.OUT_ROUNDED, X.OUT_PAIR_SILU, X.OUT_QKV_ROPE):
        bufs["y"] = _sent("i16", (c.N if c.pair else Ntot) + X.TAIL)
    off = 0
    for s, (i, c0, n) in enumerate(b.seg_img):
        gout.w[s], gout.ld[s], gout.col0[s], gout.ncols[s], gout.tau[s] = imgs[i].data_ptr(), b.ld[i], c0, n, b.taus[s]
        if "y" in bufs and (s == 0 or c.out == X.OUT_ROUNDED):
            gout.y[s] = bufs["y"].data_ptr() + 2 * off
        if c.w8:
            gout.scale[s] = scales[i].data_ptr() + 2 * c0
        off += n
    gout.weight_bits = 8 if c.w8 else 16
    gout.act_seg0 = c.act_seg0
    if c.out in (X.OUT_SLABS, X.OUT_QKV_ROPE):
        bufs["slabs"] = _sent("i32", X.MAX_SLABS * Ntot + X.TAIL)
        gout.slabs, gout.slabs_bytes, gout.slabs_interleaved = bufs["slabs"].data_ptr(), X.MAX_SLABS * Ntot * 4, c.il
    elif c.out == X.OUT_SLAB_SUM:
        bufs["slabs"] = _sent("i32", Ntot + X.TAIL)
        gout.slabs, gout.slabs_bytes = bufs["slabs"].data_ptr(), Ntot * 4
    if c.pair:
        bufs["mask_out"] = _sent("i64", c.N // 64 + 8)
        gout.mask_out, gout.mask_tau = bufs["mask_out"].data_ptr(), mask_tau
    if c.out == X.OUT_QKV_ROPE:
        r = c.rope
        nkv = c.segs[1][0] // r["hd"]
        for nm in ("kc", "vc"):
            bufs[nm] = _sent("i16", nkv * r["max_seq"] * r["hd"] + X.TAIL)
        gout.rope, gout.rope_pos = keep["rope"].data_ptr(), keep["rope_pos"].data_ptr()
        gout.k_cache, gout.v_cache = bufs["kc"].data_ptr(), bufs["vc"].data_ptr()
        gout.rope_head_dim, gout.rope_max_seq = r["hd"], r["max_seq"]
    desc = ctypes.create_string_buffer(160)
    gout.desc, gout.desc_bytes = ctypes.cast(desc, ctypes.c_char_p), 160
    ns_out = ctypes.c_int(-1)
    rc = L.teal_fused_gemv(ctypes.byref(gin), ctypes.byref(gout), c.Z, X.CODE[c.dt], ws.data_ptr(), ws.numel() * 4, ctypes.byref(ns_out),
                           runtime.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (c.name, "rc", rc)
    geo = X.geometry(c, desc.value.decode(), ns_out.value)
    if c.out == X.OUT_QKV_ROPE:
        assert (ns_out.value == 0) == geo["rope"], (c.name, ns_out.value, desc.value)
    if c.out == X.OUT_SLAB_SUM:
        assert ns_out.value == 1
    return geo, {k: t.cpu().numpy() for k, t in bufs.items()}, desc.value.decode()


def _compare(c, name, got, want):
    d = X.first_diff(got, want)
    if d is not None:
        n = int((got != want).sum())
        raise AssertionError(f"case {c.name} buffer {name}: {n} of {want.size} words differ; first at word {d[0]}: got {int(got[d]):#x}, "
                             f"want {int(want[d]):#x}")
    return int(want.size)


def _run(c):
    runtime.init()
    tuning = None if c.lib is None else (c.lib[0], 0, c.lib[1], 0)
    with helpers.lib_for(fast=c.fast, tuning=tuning) as L:
        runtime.init()
        b = X.build(c)
        Ntot = sum(n for n, _ in c.segs)
        nbytes = int(L.teal_workspace_bytes(c.Z, Ntot))
        ws = runtime.new_workspace(c.Z, Ntot) if c.prepared else torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=DEV)
        words, led, geo0, descs = 0, None, None, []
        for j, mt in enumerate(b.mask_taus or [None]):
            geo, got, desc = _launch(L, c, b, ws, mt)
            assert geo0 is None or (geo["kernel"], geo["lpr"], geo["split"]) == (geo0["kernel"], geo0["lpr"], geo0["split"])
            geo0 = geo
            led = X.check_claims(b, geo)
            ref = X.reference(b, geo)
            if c.pair:
                ref["mask_out"] = ref.pop(f"mask_out{j}")
                for k in [k for k in ref if k.startswith("mask_out") and k != "mask_out"]:
                    del ref[k]
            assert set(ref) == set(got), (sorted(ref), sorted(got))
            for name in sorted(ref):
                words += _compare(c, name, got[name], ref[name])
            descs.append(desc)
        del ws
    return led, words, descs[0]


@pytest.mark.parametrize("name", list(CASES))
def test_fused_gemv_bit_exact(name):
    c = CASES[name]
    led, n, desc = _run(c)
    print("\n" + X.probe_line(c, led, n))
    print(f"LEDGER {c.name}: {desc}")


def test_resid_norm_beyond_the_register_cache_is_refused():
    """RESID_NORM caches the whole vector in registers in both kernels: Z = 16448, the first multiple of 64 beyond 16 rounds of
    16 chunks, is refused before any launch (TEAL_ERR_SHAPE) — neither kernel serves it, none may fall through silently"""
    from teal_amd import _lib
    L = _lib.load()
    runtime.init()
    Z, N = 16448, 64
    resid = torch.zeros(Z, dtype=torch.float16, device=DEV)
    nw = torch.ones(Z, dtype=torch.float16, device=DEV)
    W = torch.ones(Z, N, dtype=torch.float16, device=DEV)
    y = _sent("i16", N)
    ws = runtime.new_workspace(Z, N)
    gin = GemvIn(mode=X.IN_RESID_NORM, resid_in=resid.data_ptr(), norm_weight=nw.data_ptr(), eps=0.0)
    gout = GemvOut()
    gout.nseg, gout.mode = 1, X.OUT_ROUNDED
    gout.w[0], gout.ld[0], gout.col0[0], gout.ncols[0], gout.tau[0], gout.y[0] = W.data_ptr(), N, 0, N, 1.0, y.data_ptr()
    rc = L.teal_fused_gemv(ctypes.byref(gin), ctypes.byref(gout), Z, 0, ws.data_ptr(), ws.numel() * 4, None, runtime.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -3, rc
    assert bool((y == int(X.SENT16_I)).all())
