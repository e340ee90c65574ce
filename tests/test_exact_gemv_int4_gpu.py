"""GPU: exact-integer probes of the int4 fused GEMV (teal_amd/csrc/teal_gemv_int4.hip), teal_fused_gemv with weight_bits = 4
through the C ABI — PLAIN, RESID_NORM, SILU_MUL and ATTN_MERGE producers, ROUNDED (split 1 and split-K by arrival tickets) and
SLABS (interleaved, planar) outputs, both list walks (SHARE, GROUP), group sizes 32 / 64 / 128 / 256, one to three segments
of one image, fp16 and bf16.

The inputs are small integers, nibbles, power-of-two scales and integer zeros (tests/exact_gemv_int4.py), so every fp32 value
the kernel forms is exact in any order and every output buffer is compared WHOLE and BIT FOR BIT with an integer reference:
16-bit vectors as int16, fp32 slabs as int32, and the sentinel words behind every output, in the slab padding lanes and in the
slabs beyond split.  What a launch must not read holds nibble 15 next to dropped activations of +-1, 0xFF (the ld - N padding)
or NaN (scales_and_zeros outside the segments).  No tolerance anywhere (of a default quiet NaN the sign bit alone is not
compared: nan_half_pair_*).

Everything runs through the product library (the int4 path has no geometry switches).  After each launch the test reads
*nslabs_out and teal_gemv_out.desc; the reference runs at the split and kind the launch REPORTED, and the ledger built from
it is asserted against what the case was written for.  tests/test_exact_gemv_int4_host.py shows on the CPU that a leaked or
swapped pair half, a dropped pair, a stale list slot, a doubled dead unit, a neighbour group's parameters, an unscaled odd
nibble ... change a compared word in these very cases.  Each test prints a `PROBE` line (profiles/exact_gemv_int4.txt).
"""
import ctypes

import numpy as np
import pytest
import torch

import exact_gemv_int4 as X
from teal_amd import _lib, runtime
from teal_amd.gpt_fast.engine import GemvIn, GemvOut

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = X.cases()
SENT = {"i16": (torch.int16, int(X.SENT16_I)), "i32": (torch.int32, int(X.SENT32_I))}


def _sent(kind, n):
    dt, v = SENT[kind]
    return torch.full((n,), v, dtype=dt, device=DEV)


def _launch(L, c, b, dev, ws, out_mode):
    """one teal_fused_gemv launch into sentinel-filled buffers -> (geometry reported, {buffer name: words}, desc)"""
    keep, img, sz = dev
    bufs = {}
    gin = GemvIn(mode=c.mode)
    if c.mode == X.IN_RESID_NORM:
        gin.resid_in, gin.norm_weight, gin.eps = keep["resid"].data_ptr(), keep["norm_w"].data_ptr(), c.eps
        if c.row_index:
            gin.row_index = keep["row_index"].data_ptr()
        if c.nslabs:
            gin.slabs, gin.nslabs, gin.slabs_interleaved = keep["slabs_in"].data_ptr(), c.nslabs, 1
        bufs["resid_out"] = _sent("i16", c.Z + X.TAIL)
        gin.resid_out = bufs["resid_out"].data_ptr()
    else:
        gin.x = keep["x"].data_ptr()
        if c.mode == X.IN_ATTN_MERGE:
            gin.att_head_dim, gin.att_nsplit = c.att_hd, c.att_arg
    gout = GemvOut()
    gout.nseg, gout.mode, gout.weight_bits, gout.groupsize = len(c.segs), out_mode, 4, c.G
    if out_mode == X.OUT_ROUNDED:
        bufs["y"] = _sent("i16", c.N + X.TAIL)
    else:
        bufs["slabs"] = _sent("i32", X.SLAB_ROOM * c.N + X.TAIL)
        gout.slabs, gout.slabs_bytes, gout.slabs_interleaved = bufs["slabs"].data_ptr(), X.SLAB_ROOM * c.N * 4, c.il
    off = 0
    for s, (c0, n, _) in enumerate(c.segs):
        gout.w[s], gout.ld[s], gout.col0[s], gout.ncols[s], gout.tau[s] = img.data_ptr(), b.ld, c0, n, b.taus[s]
        gout.scale[s], gout.scale_ld[s] = sz.data_ptr(), b.scale_ld
        if "y" in bufs:
            gout.y[s] = bufs["y"].data_ptr() + 2 * off
        off += n
    desc = ctypes.create_string_buffer(160)
    gout.desc, gout.desc_bytes = ctypes.cast(desc, ctypes.c_char_p), 160
    ns_out = ctypes.c_int(-1)
    rc = L.teal_fused_gemv(ctypes.byref(gin), ctypes.byref(gout), c.Z, X.CODE[c.dt], ws.data_ptr(), ws.numel() * 4, ctypes.byref(ns_out),
                           runtime.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (c.name, "rc", rc)
    geo = X.geometry(c, desc.value.decode(), ns_out.value)
    return geo, {k: t.cpu().numpy() for k, t in bufs.items()}, desc.value.decode()


def _compare(c, name, got, want):
    got = X.nan_sign_dropped(got, c.dt)
    d = X.first_diff(got, want)
    if d is not None:
        n = int((got != want).sum())
        raise AssertionError(f"case {c.name} buffer {name}: {n} of {want.size} words differ; first at word {d[0]}: got {int(got[d]):#x}, "
                             f"want {int(want[d]):#x}")
    return int(want.size)


def _run(c):
    runtime.init()
    L = _lib.load()
    b = X.build(c)
    dev = ({k: t.to(DEV) for k, t in b.inputs.items()}, b.image_t.to(DEV), b.sz_t.to(DEV))
    nbytes = int(L.teal_workspace_bytes(c.Z, c.N))
    prepared = runtime.new_workspace(c.Z, c.N)
    ws = prepared if c.prepared else torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=DEV)
    geo, got, desc = _launch(L, c, b, dev, ws, c.out)
    ref = X.reference(b, geo)
    led = X.check_claims(b, geo)
    if c.twice:   # the same workspace again: the tickets must have been re-armed
        geo2, got2, _ = _launch(L, c, b, dev, ws, c.out)
        assert (geo2["kind"], geo2["split"]) == (geo["kind"], geo["split"])
        got["y2"] = got2["y"]
    assert set(ref) == set(got), (sorted(ref), sorted(got))
    words = sum(_compare(c, name, got[name], ref[name]) for name in sorted(ref))
    if c.also_rounded:   # the slabs summed in slice order in fp32, then rounded, are the ROUNDED launch's words
        geo3, got3, _ = _launch(L, c, b, dev, prepared, X.OUT_ROUNDED)
        assert (geo3["kind"], geo3["split"]) == (geo["kind"], geo["split"])
        words += _compare(c, "y (rounded from the slabs)", got3["y"], X.rounded_from_slabs(c, got["slabs"], geo["split"]))
    return led, words, desc


@pytest.mark.parametrize("name", list(CASES))
def test_int4_fused_gemv_bit_exact(name):
    c = CASES[name]
    led, n, desc = _run(c)
    print("\n" + X.probe_line(c, led, n))
    print(f"LEDGER {c.name}: {desc}")


# ---- refusals: nothing launched, every output still all sentinels ---------------------------------------------------------------

def _refuse_gate_activated(gin, gout):
    gin.mode, gin.gate_activated = X.IN_SILU_MUL, 1


def _refuse_act_seg0(gin, gout):
    gout.act_seg0 = 1


def _refuse_out(mode):
    def f(gin, gout):
        gout.mode = mode
    return f


def _refuse_masked(gin, gout):
    gin.mode = X.IN_MASKED


def _refuse_planar_in(gin, gout):
    gin.mode, gin.nslabs, gin.slabs_interleaved = X.IN_RESID_NORM, 2, 0


def _refuse_nslabs9(gin, gout):
    gin.mode, gin.nslabs, gin.slabs_interleaved = X.IN_RESID_NORM, 9, 1


def _refuse_g48(gin, gout):
    gout.groupsize = 48


def _refuse_ncols64(gin, gout):
    gout.ncols[0] = 64


def _refuse_norm_z(gin, gout):
    gin.mode = X.IN_RESID_NORM


REFUSALS = {
    "gate_activated": (_refuse_gate_activated, 1536, -1), "act_seg0": (_refuse_act_seg0, 1536, -1),
    "qkv_rope": (_refuse_out(X.OUT_QKV_ROPE), 1536, -1), "slab_sum": (_refuse_out(X.OUT_SLAB_SUM), 1536, -1),
    "pair_silu": (_refuse_out(X.OUT_PAIR_SILU), 1536, -1), "in_masked": (_refuse_masked, 1536, -1),
    "planar_input_slabs": (_refuse_planar_in, 1536, -1), "nslabs_9": (_refuse_nslabs9, 1536, -1), "groupsize_48": (_refuse_g48, 1536, -1),
    "ncols_64": (_refuse_ncols64, 1536, -3), "resid_norm_z16416": (_refuse_norm_z, 16416, -3),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_int4_refusals_leave_the_outputs_untouched(name):
    """what the int4 path does not serve is refused before any launch (TEAL_ERR_ARG / TEAL_ERR_SHAPE): every output buffer
    still holds its sentinels.  Every pointer a launch could follow is valid and large enough all the same."""
    change, Z, want = REFUSALS[name]
    runtime.init()
    L = _lib.load()
    N, G = 128, 32   # (Z = 1536 is a multiple of 48 too: the group size is refused for itself)
    x = torch.ones(2 * Z, dtype=torch.float16, device=DEV)
    slabs_in = torch.zeros(Z * 12, dtype=torch.float32, device=DEV)
    masks = torch.zeros(Z // 32 + 8, dtype=torch.int64, device=DEV)
    img = torch.zeros(Z // 2, N + 64, dtype=torch.uint8, device=DEV)
    sz = torch.ones(Z // G, N + 8, 2, dtype=torch.bfloat16, device=DEV)
    y, resid_out, slabs = _sent("i16", N + X.TAIL), _sent("i16", Z + X.TAIL), _sent("i32", X.SLAB_ROOM * N + X.TAIL)
    mask_out = torch.full((N // 64 + 8,), 0x5A5A, dtype=torch.int64, device=DEV)
    ws = runtime.new_workspace(Z, N)
    gin = GemvIn(mode=X.IN_PLAIN, x=x.data_ptr(), resid_in=x.data_ptr(), norm_weight=x.data_ptr(), slabs=slabs_in.data_ptr(),
                 resid_out=resid_out.data_ptr(), masks=masks.data_ptr(), att_head_dim=64, att_nsplit=4)
    gout = GemvOut()
    gout.nseg, gout.mode, gout.weight_bits, gout.groupsize = 1, X.OUT_ROUNDED, 4, G
    gout.w[0], gout.ld[0], gout.col0[0], gout.ncols[0], gout.tau[0], gout.y[0] = img.data_ptr(), N + 64, 0, N, 0.5, y.data_ptr()
    gout.scale[0], gout.scale_ld[0] = sz.data_ptr(), N + 8
    gout.slabs, gout.slabs_bytes, gout.slabs_interleaved = slabs.data_ptr(), X.SLAB_ROOM * N * 4, 1
    gout.mask_out, gout.mask_tau = mask_out.data_ptr(), 0.5
    change(gin, gout)
    ns_out = ctypes.c_int(-1)
    rc = L.teal_fused_gemv(ctypes.byref(gin), ctypes.byref(gout), Z, 0, ws.data_ptr(), ws.numel() * 4, ctypes.byref(ns_out), runtime.stream_ptr())
    torch.cuda.synchronize()
    assert rc == want, (name, rc)
    assert ns_out.value == -1
    assert bool((y == int(X.SENT16_I)).all()) and bool((resid_out == int(X.SENT16_I)).all()) and bool((slabs == int(X.SENT32_I)).all())
    assert bool((mask_out == 0x5A5A).all())
