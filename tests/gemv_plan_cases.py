"""The GEMV launch-plan case table: teal_fused_gemv requests (FUSED) and legacy-entry calls (LEGACY) whose return code, slab
count and launch description are pinned by tests/golden/gemv_plan_parent.json (recorded by scripts/record_gemv_plan.py on an
MI355X).  Which kernel and grid a request gets is integer arithmetic on shapes and a CU count, and its branches are thresholds
on real model widths against 256 CUs — so the shapes here are real model widths, the smallest that reach them.  The data is all
zeros: one zero-filled arena serves every weight image and every input, one scratch arena every output.

A case is a plain dict; `materialise` turns it into the two argument structs over a `Memory` — real device addresses for a
launch, made-up ones with the same nullness, alignment and identities for the host-only query."""
from __future__ import annotations

import ctypes

F16, BF16 = 0, 1
IN_PLAIN, IN_RESID_NORM, IN_SILU_MUL, IN_MASKED, IN_ATTN_MERGE = 0, 1, 2, 3, 4
OUT_ROUNDED, OUT_SLABS, OUT_PAIR_SILU, OUT_QKV_ROPE, OUT_SLAB_SUM = 0, 1, 2, 3, 4
MAX_SEQ = 4  # rows of the RoPE table and the KV caches


class GemvIn(ctypes.Structure):  # teal_gemv_in_t
    _fields_ = [("mode", ctypes.c_int), ("x", ctypes.c_void_p), ("resid_in", ctypes.c_void_p),
                ("row_index", ctypes.c_void_p), ("slabs", ctypes.c_void_p), ("nslabs", ctypes.c_int),
                ("norm_weight", ctypes.c_void_p), ("eps", ctypes.c_float), ("resid_out", ctypes.c_void_p),
                ("masks", ctypes.c_void_p), ("att_head_dim", ctypes.c_int), ("att_nsplit", ctypes.c_int),
                ("slabs_interleaved", ctypes.c_int), ("gate_activated", ctypes.c_int)]


class GemvOut(ctypes.Structure):  # teal_gemv_out_t
    _fields_ = [("nseg", ctypes.c_int), ("w", ctypes.c_void_p * 3), ("ld", ctypes.c_int * 3),
                ("col0", ctypes.c_int * 3), ("ncols", ctypes.c_int * 3), ("tau", ctypes.c_float * 3),
                ("y", ctypes.c_void_p * 3), ("mode", ctypes.c_int), ("slabs", ctypes.c_void_p),
                ("slabs_bytes", ctypes.c_size_t), ("mask_out", ctypes.c_void_p), ("mask_tau", ctypes.c_float),
                ("slabs_interleaved", ctypes.c_int), ("weight_bits", ctypes.c_int), ("scale", ctypes.c_void_p * 3),
                ("scale_ld", ctypes.c_int * 3), ("groupsize", ctypes.c_int),
                ("rope", ctypes.c_void_p), ("rope_pos", ctypes.c_void_p), ("k_cache", ctypes.c_void_p), ("v_cache", ctypes.c_void_p),
                ("rope_head_dim", ctypes.c_int), ("rope_max_seq", ctypes.c_int), ("act_seg0", ctypes.c_int),
                ("desc", ctypes.c_void_p), ("desc_bytes", ctypes.c_int)]


# ---- memory ---------------------------------------------------------------------------------------------------------------------
# the scratch arena, by region (bytes): nothing a launch of the table writes leaves its region
Y_OFF, RESID_OFF, MASK_OFF, KC_OFF, VC_OFF, SLABS_OFF = 0, 1 << 20, (1 << 20) + (256 << 10), 2 << 20, 3 << 20, 4 << 20
SLABS_ROOM = 60 << 20
SCRATCH_BYTES = SLABS_OFF + SLABS_ROOM
WS_BYTES = 64 << 20  # each of the two workspaces (the prepared one and the plain one)
WS_HEADER = 82176    # what teal_workspace_init keeps at the start of a prepared workspace (arrival counters, sampler scratch)


class Memory:
    """Base addresses: `zeros` (read only: weights, scales, every input), `scratch` (outputs), `ws` (a workspace prepared through
    the library under test), `plain` (an unprepared one)."""

    def __init__(self, zeros, scratch, ws, plain, zeros_bytes=None):
        self.zeros, self.scratch, self.ws, self.plain, self.zeros_bytes = zeros, scratch, ws, plain, zeros_bytes


FAKE = Memory(0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000, 0x7300_0000_0000)  # the host-only query follows no pointer


# ---- the table ------------------------------------------------------------------------------------------------------------------
FUSED: list = []
LEGACY: list = []


def fused(cid, Z, cols, inp=IN_PLAIN, out=OUT_ROUNDED, ws="prepared", dtype=F16, bits=16, **kw):
    """cols: columns per threshold segment (one image, the segments side by side; images=2: one image per segment).  kw: nslabs,
    in_il, gate_activated, att_hd, att_ns, out_il, slabs_bytes, ws_bytes, act_seg0, rope_hd, groupsize, null=(names), tweak=(names),
    switches={fast, wave_local, lpr, split} (diagnostics build)."""
    assert all(c["id"] != cid for c in FUSED), cid
    FUSED.append(dict(id=cid, Z=Z, cols=list(cols), inp=inp, out=out, ws=ws, dtype=dtype, bits=bits, **kw))


def legacy(cid, fn, Z, N, ws="prepared", dtype=F16, **kw):
    assert all(c["id"] != cid for c in LEGACY), cid
    LEGACY.append(dict(id=cid, fn=fn, Z=Z, N=N, ws=ws, dtype=dtype, **kw))


# name: (dim, intermediate, q | k | v columns, head_dim, vocabulary)
MODELS = {
    "1b": (2048, 5632, (2048, 256, 256), 64, 32000),           # TinyLlama-1.1B
    "7b": (4096, 11008, (4096, 4096, 4096), 128, 32000),       # Llama-2-7B
    "8b": (4096, 14336, (4096, 1024, 1024), 128, 128256),      # Llama-3-8B
    "13b": (5120, 13824, (5120, 5120, 5120), 128, 32000),      # Llama-2-13B
    "30b": (6656, 17920, (6656, 6656, 6656), 128, 32000),      # Llama-30B
    "70b": (8192, 28672, (8192, 1024, 1024), 128, 32000),      # Llama-2-70B
}


def _decode_layer(name, dt):
    """the launches of one decode layer of a model, in the forms the engines use and the ones they could"""
    dim, inter, qkv, hd, vocab = MODELS[name]
    other = BF16 if dt == F16 else F16
    norm = dict(inp=IN_RESID_NORM, nslabs=4)
    fused(f"{name}.wqkv.rope", dim, qkv, out=OUT_QKV_ROPE, dtype=dt, rope_hd=hd, **norm)
    fused(f"{name}.wqkv.slabs", dim, qkv, out=OUT_SLABS, dtype=other, **norm)
    fused(f"{name}.wqkv.rounded", dim, qkv, dtype=dt, **norm)
    fused(f"{name}.wqkv.rounded.nows", dim, qkv, ws="none", dtype=dt, inp=IN_RESID_NORM, nslabs=1, in_il=0)
    fused(f"{name}.wqkv.w8.slabs", dim, qkv, out=OUT_SLABS, dtype=dt, bits=8, **norm)
    fused(f"{name}.wo.merge.slabs", dim, [dim], inp=IN_ATTN_MERGE, att_hd=hd, att_ns=8 if dim <= 4096 else 4, out=OUT_SLABS, dtype=dt)
    fused(f"{name}.wo.plain.ticketed", dim, [dim], dtype=other)
    fused(f"{name}.wo.plain.reduce", dim, [dim], ws="plain", dtype=other)
    fused(f"{name}.wo.masked.slabsum", dim, [dim], inp=IN_MASKED, out=OUT_SLAB_SUM, dtype=dt)
    fused(f"{name}.wo.w8.merge.ticketed", dim, [dim], inp=IN_ATTN_MERGE, att_hd=hd, att_ns=4, bits=8, dtype=dt)
    fused(f"{name}.wo.w8.plain.reduce", dim, [dim], ws="plain", bits=8, dtype=other)
    fused(f"{name}.wo.w8.slabs", dim, [dim], out=OUT_SLABS, bits=8, dtype=other)
    fused(f"{name}.gateup.pair", dim, [inter, inter], images=2, out=OUT_PAIR_SILU, dtype=dt, **norm)
    fused(f"{name}.gateup.w8.pair", dim, [inter, inter], images=2, out=OUT_PAIR_SILU, bits=8, dtype=other, **norm)
    fused(f"{name}.gateup.act0", dim, [inter, inter], images=2, act_seg0=1, dtype=other, **norm)
    fused(f"{name}.gateup.slabs.planar", dim, [inter, inter], images=2, out=OUT_SLABS, out_il=0, dtype=dt, **norm)
    fused(f"{name}.down.silu.slabs", inter, [dim], inp=IN_SILU_MUL, out=OUT_SLABS, dtype=dt)
    fused(f"{name}.down.activated.slabsum", inter, [dim], inp=IN_SILU_MUL, gate_activated=1, out=OUT_SLAB_SUM, dtype=other)
    fused(f"{name}.down.masked.slabs.planar", inter, [dim], inp=IN_MASKED, out=OUT_SLABS, out_il=0, dtype=other)
    fused(f"{name}.down.silu.ticketed", inter, [dim], inp=IN_SILU_MUL, dtype=dt)
    fused(f"{name}.down.silu.reduce", inter, [dim], inp=IN_SILU_MUL, ws="plain", dtype=dt)
    fused(f"{name}.down.w8.slabs", inter, [dim], inp=IN_SILU_MUL, out=OUT_SLABS, bits=8, dtype=dt)
    fused(f"{name}.down.w8.slabsum", inter, [dim], inp=IN_SILU_MUL, out=OUT_SLAB_SUM, bits=8, dtype=other)
    fused(f"{name}.lm_head", dim, [vocab], ws="none", dtype=dt, inp=IN_RESID_NORM, nslabs=8)
    fused(f"{name}.lm_head.w8", dim, [vocab], ws="none", dtype=other, bits=8, inp=IN_RESID_NORM, nslabs=8)
    for g in (32, 64, 128, 256):  # int4: ncols multiples of 128
        if inter % g == 0:
            fused(f"{name}.i4.g{g}.down.slabs", inter, [dim], inp=IN_SILU_MUL, out=OUT_SLABS, bits=4, groupsize=g, dtype=dt)
        fused(f"{name}.i4.g{g}.wo.ticketed", dim, [dim], inp=IN_ATTN_MERGE, att_hd=hd, att_ns=4, bits=4, groupsize=g, dtype=other)
    fused(f"{name}.i4.wqkv.slabs", dim, qkv, out=OUT_SLABS, bits=4, groupsize=128, dtype=dt, **norm)
    fused(f"{name}.i4.wqkv.slabs.planar", dim, qkv, out=OUT_SLABS, out_il=0, bits=4, groupsize=64, dtype=dt, **norm)
    fused(f"{name}.i4.wo.nows", dim, [dim], ws="none", bits=4, groupsize=32, dtype=dt)
    fused(f"{name}.i4.wo.plainws", dim, [dim], ws="plain", bits=4, groupsize=32, dtype=other)
    if inter % 128 == 0:
        fused(f"{name}.i4.gateup.act.rounded", dim, [inter, inter], images=2, bits=4, groupsize=128, dtype=other, **norm)


for _i, _name in enumerate(MODELS):
    _decode_layer(_name, F16 if _i % 2 == 0 else BF16)

# ---- shapes beyond a layer's -------------------------------------------------------------------------------------------------
_N4 = dict(inp=IN_RESID_NORM, nslabs=4)
# tensor-parallel rank-local shapes: wo 2048 -> 4096 has two rounds, Llama-3-8B's wqkv / 2 four
fused("tp2.7b.wo.slabs", 2048, [4096], inp=IN_ATTN_MERGE, att_hd=128, att_ns=4, out=OUT_SLABS)
fused("tp2.7b.wo.slabsum", 2048, [4096], inp=IN_ATTN_MERGE, att_hd=128, att_ns=8, out=OUT_SLAB_SUM, dtype=BF16)
fused("tp2.7b.wo.slabsum.nows", 2048, [4096], out=OUT_SLAB_SUM, ws="plain")
fused("tp2.8b.wqkv.rope", 4096, (2048, 512, 512), out=OUT_QKV_ROPE, rope_hd=128, dtype=BF16, **_N4)
fused("tp2.8b.wqkv.slabs", 4096, (2048, 512, 512), out=OUT_SLABS, **_N4)
fused("tp2.7b.down.slabsum", 5504, [4096], inp=IN_SILU_MUL, out=OUT_SLAB_SUM)
fused("tp8.70b.down.slabsum", 3584, [8192], inp=IN_SILU_MUL, out=OUT_SLAB_SUM, dtype=BF16)
fused("tp8.70b.wqkv.rope", 8192, (1024, 128, 128), out=OUT_QKV_ROPE, rope_hd=128, **_N4)
# cache depth 16: the RMSNorm producer over more than 8 rounds (Llama-3-405B, dim 16384, wqkv of one of 8 ranks; GPT-3's 12288)
fused("405b.tp8.wqkv.slabs", 16384, (2048, 128, 128), out=OUT_SLABS, **_N4)
fused("405b.tp8.wqkv.slabs.bf16", 16384, (2048, 128, 128), out=OUT_SLABS, dtype=BF16, **_N4)
fused("405b.wqkv.slabs", 16384, (16384, 1024, 1024), out=OUT_SLABS, **_N4)
fused("405b.wo.merge.slabs", 16384, [16384], inp=IN_ATTN_MERGE, att_hd=128, att_ns=4, out=OUT_SLABS)
fused("175b.norm.slabs", 12288, [4096], out=OUT_SLABS, dtype=BF16, **_N4)
fused("175b.norm.rounded", 12288, [4096], **_N4)
fused("175b.pair.44k", 12288, [4096, 4096], images=2, out=OUT_PAIR_SILU, **_N4)
# ragged Z and N, Z above 16384, many slabs
fused("yi6b.lm_head", 4096, [64000], ws="none", inp=IN_RESID_NORM, nslabs=8)  # 256-column tiles
fused("yi6b.lm_head.plain", 4096, [64000], ws="none", dtype=BF16)
fused("ragged.z", 4100, [4096], ws="plain")
fused("ragged.z.slabs", 4100, [4096], out=OUT_SLABS, dtype=BF16)
fused("ragged.n", 4096, [11016], ws="none")
fused("ragged.n.slabs.planar", 4096, [4104], out=OUT_SLABS, out_il=0)
fused("ragged.pair", 4100, [11016, 11016], images=2, out=OUT_PAIR_SILU, **_N4)
fused("long.plain.reduce", 28672, [8192], ws="plain")
fused("long.plain.ticketed", 28672, [8192], dtype=BF16)
# a list too long for CUs / tiles slices: the split grows until the lists fit the LDS (7, 5) and then until tiles x slices
# fill whole rounds of workgroups (128 x 8, 128 x 6) — without that last step the slices outnumber the rounds' worth of
# cached chunks and the launch is the general kernel's
fused("long.65536.slabs.whole_rounds", 65536, [8192], out=OUT_SLABS)
fused("long.49152.slabs.whole_rounds", 49152, [8192], inp=IN_SILU_MUL, out=OUT_SLABS, dtype=BF16)
fused("long.49152.slabsum.whole_rounds", 49152, [8192], out=OUT_SLAB_SUM)
fused("long.65536.ticketed", 65536, [512])
fused("long.65536.planar", 65536, [512], out=OUT_SLABS, out_il=0, dtype=BF16)
fused("long.65536.interleave", 65536, [64], out=OUT_SLABS)
fused("long.norm.shape", 16448, [4096], **_N4)
fused("long.merge.shape", 16512, [4096], inp=IN_ATTN_MERGE, att_hd=128, att_ns=4)
fused("y_apart.general", 4096, (4096, 1024, 1024), tweak=("y_apart",), **_N4)
fused("three_images.general", 4096, (4096, 4096, 4096), images=3, **_N4)
fused("w8.scales_apart.general", 4096, (4096, 1024, 1024), bits=8, out=OUT_SLABS, tweak=("scales_apart",), **_N4)
fused("norm.planar2.general", 4096, (4096, 4096, 4096), inp=IN_RESID_NORM, nslabs=2, in_il=0, out=OUT_SLABS)
fused("norm.planar1.lean", 4096, (4096, 4096, 4096), inp=IN_RESID_NORM, nslabs=1, in_il=0, out=OUT_SLABS)
fused("norm.planar9.general", 4096, (4096, 4096, 4096), inp=IN_RESID_NORM, nslabs=9, in_il=0, out=OUT_SLABS)
fused("norm.row_index", 4096, (4096, 4096, 4096), inp=IN_RESID_NORM, nslabs=0, out=OUT_SLABS, tweak=("row_index",))
fused("rope.hd64", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=64, **_N4)
fused("rope.hd64.bf16", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=64, dtype=BF16, **_N4)
fused("rope.hd96.slabs", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=96, **_N4)
fused("rope.w8.slabs", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=128, bits=8, **_N4)
fused("rope.kv_unequal.slabs", 4096, (4096, 1024, 2048), out=OUT_QKV_ROPE, rope_hd=128, **_N4)
fused("slabsum.split1", 4096, [12288], out=OUT_SLAB_SUM, ws="none")
fused("slabsum.nseg2", 4096, [2048, 2048], out=OUT_SLAB_SUM)
fused("slabsum.ragged.config", 4100, [4096], out=OUT_SLAB_SUM)
fused("slabsum.small_dst", 4096, [4096], out=OUT_SLAB_SUM, slabs_bytes=4096 * 4 - 4)

# ---- refusals -------------------------------------------------------------------------------------------------------------------
fused("refuse.z0", 0, [4096])
fused("refuse.nseg0", 4096, [])
fused("refuse.dtype", 4096, [4096], dtype=2)
fused("refuse.z65600", 65600, [4096])
fused("refuse.act0.slabs", 4096, [4096], out=OUT_SLABS, act_seg0=1)
fused("refuse.in_mode", 4096, [4096], inp=7)
fused("refuse.out_mode", 4096, [4096], out=9)
fused("refuse.bits12", 4096, [4096], bits=12)
fused("refuse.null_x", 4096, [4096], null=("x",))
fused("refuse.null_masks", 4096, [4096], inp=IN_MASKED, null=("masks",))
fused("refuse.merge.hd96", 4096, [4096], inp=IN_ATTN_MERGE, att_hd=96, att_ns=4)
fused("refuse.merge.ns5", 4096, [4096], inp=IN_ATTN_MERGE, att_hd=128, att_ns=5)
fused("refuse.merge.lanes", 8320, [4096], inp=IN_ATTN_MERGE, att_hd=128, att_ns=8)  # one lane per (chunk, split)
fused("refuse.norm.null_weight", 4096, [4096], null=("norm_weight",), **_N4)
fused("refuse.norm.null_slabs", 4096, [4096], null=("slabs_in",), **_N4)
fused("refuse.norm.alias", 4096, [4096], tweak=("resid_alias",), **_N4)
fused("refuse.norm.il9", 4096, [4096], inp=IN_RESID_NORM, nslabs=9)
fused("refuse.null_w", 4096, [4096], null=("w0",))
fused("refuse.ncols4", 4096, [4100])
fused("refuse.col0_4", 4096, [4096], tweak=("col0_4",))
fused("refuse.ld4", 4096, [4096], tweak=("ld_4",))
fused("refuse.w_misaligned", 4096, [4096], tweak=("w_plus8",))
fused("refuse.null_y", 4096, [4096], null=("y0",))
fused("refuse.pair.nseg1", 4096, [11008], out=OUT_PAIR_SILU, **_N4)
fused("refuse.pair.plain_in", 4096, [11008, 11008], images=2, out=OUT_PAIR_SILU)
fused("refuse.pair.unequal", 4096, [11008, 4096], images=2, out=OUT_PAIR_SILU, **_N4)
fused("refuse.pair.z16448", 16448, [4096, 4096], images=2, out=OUT_PAIR_SILU, **_N4)
fused("refuse.slabs.null", 4096, [4096], out=OUT_SLABS, null=("out_slabs",))
fused("refuse.slabs.small", 4096, [4096], out=OUT_SLABS, slabs_bytes=4096 * 4 * 4 - 16)
fused("refuse.slabs.misaligned", 4096, [4096], out=OUT_SLABS, tweak=("slabs_plus8",))
fused("refuse.slabsum.null", 4096, [4096], out=OUT_SLAB_SUM, null=("out_slabs",))
fused("refuse.ws.small", 11008, [4096], ws_bytes=4096)
fused("refuse.ws.small.prepared", 11008, [4096], ws_bytes=WS_HEADER + 4096)
fused("refuse.ws.none", 11008, [4096], ws="none")
fused("refuse.lds64k", 8192, [128256], ws="none")  # (Llama-3-70B's lm_head: 512-column tiles and eight cached rounds)
fused("refuse.w8.null_scale", 4096, [4096], bits=8, null=("scale0",))
fused("refuse.rope.null_table", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=128, null=("rope",), **_N4)
fused("refuse.rope.null_pos", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=128, null=("rope_pos",), **_N4)
fused("refuse.rope.null_cache", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=128, null=("k_cache",), **_N4)
fused("refuse.rope.null_nslabs", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=128, null=("nslabs_out",), **_N4)
fused("refuse.rope.plain_in", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=128)
fused("refuse.rope.nseg2", 4096, (4096, 4096), out=OUT_QKV_ROPE, rope_hd=128, **_N4)
fused("refuse.rope.70b.null_slabs", 8192, (8192, 1024, 1024), out=OUT_QKV_ROPE, rope_hd=128, null=("out_slabs",), **_N4)
fused("rope.lean.null_slabs", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=128, null=("out_slabs",), **_N4)
# int4: interleaved slabs only, Z <= 16384 for RESID_NORM, no MASKED form, no rope / pair / slab sum
_I4 = dict(bits=4, groupsize=128)
fused("refuse.i4.rope", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=128, **_I4, **_N4)
fused("refuse.i4.slabsum", 4096, [4096], out=OUT_SLAB_SUM, **_I4)
fused("refuse.i4.pair", 4096, [11008, 11008], images=2, out=OUT_PAIR_SILU, **_I4, **_N4)
fused("refuse.i4.act0", 4096, [4096], act_seg0=1, **_I4)
fused("refuse.i4.activated", 11008, [4096], inp=IN_SILU_MUL, gate_activated=1, **_I4)
fused("refuse.i4.masked", 4096, [4096], inp=IN_MASKED, **_I4)
fused("refuse.i4.g48", 4608, [4096], bits=4, groupsize=48)
fused("refuse.i4.z_group", 4160, [4096], bits=4, groupsize=128)
fused("refuse.i4.ncols64", 4096, [4160], **_I4)
fused("refuse.i4.planar_in", 4096, [4096], inp=IN_RESID_NORM, nslabs=2, in_il=0, **_I4)
fused("refuse.i4.nslabs9", 4096, [4096], inp=IN_RESID_NORM, nslabs=9, in_il=1, **_I4)
fused("refuse.i4.norm.z16512", 16512, [4096], **_I4, **_N4)
fused("refuse.i4.null_scale", 4096, [4096], null=("scale0",), **_I4)
fused("refuse.i4.null_y", 4096, [4096], null=("y0",), **_I4)
fused("refuse.i4.slabs.null", 4096, [4096], out=OUT_SLABS, null=("out_slabs",), **_I4)
fused("refuse.i4.slabs.misaligned", 4096, [4096], out=OUT_SLABS, tweak=("slabs_plus8",), **_I4)
fused("refuse.i4.slabs.small", 4096, [4096], out=OUT_SLABS, slabs_bytes=4096 * 4 * 4 - 16, **_I4)
fused("refuse.i4.ws.small", 4096, [4096], ws_bytes=WS_HEADER + 4096, **_I4)
fused("refuse.i4.image_4g", 65536, [131072], ws="none", **_I4, tweak=("no_launch",))

# ---- the diagnostics switches (run through the diagnostics build) -----------------------------------------------------------------
for _sw_name, _sw in (("nofast", dict(fast=0)), ("nowl", dict(wave_local=0)), ("nowl.nofast", dict(wave_local=0, fast=0)),
                      ("lpr32", dict(lpr=32)), ("lpr16", dict(lpr=16)), ("split2", dict(split=2)), ("split16", dict(split=16)),
                      ("lpr64.split3", dict(lpr=64, split=3))):
    fused(f"diag.{_sw_name}.wqkv.rope", 4096, (4096, 4096, 4096), out=OUT_QKV_ROPE, rope_hd=128, switches=_sw, **_N4)
    fused(f"diag.{_sw_name}.wqkv8b.slabs", 4096, (4096, 1024, 1024), out=OUT_SLABS, switches=_sw, dtype=BF16, **_N4)
    fused(f"diag.{_sw_name}.wo.ticketed", 4096, [4096], inp=IN_ATTN_MERGE, att_hd=128, att_ns=8, switches=_sw)
    fused(f"diag.{_sw_name}.wo.w8.reduce", 4096, [4096], ws="plain", bits=8, switches=_sw, dtype=BF16)
    fused(f"diag.{_sw_name}.pair", 4096, [11008, 11008], images=2, out=OUT_PAIR_SILU, switches=_sw, **_N4)
    fused(f"diag.{_sw_name}.w8.pair", 4096, [11008, 11008], images=2, out=OUT_PAIR_SILU, bits=8, switches=_sw, **_N4)
    fused(f"diag.{_sw_name}.down70b.slabs", 28672, [8192], inp=IN_SILU_MUL, out=OUT_SLABS, switches=_sw)
    fused(f"diag.{_sw_name}.down.slabsum", 11008, [4096], inp=IN_SILU_MUL, out=OUT_SLAB_SUM, switches=_sw, dtype=BF16)
    fused(f"diag.{_sw_name}.i4.wo", 4096, [4096], switches=_sw, **_I4)
fused("diag.split16.interleave", 11008, [4096], out=OUT_SLABS, switches=dict(split=16))
fused("diag.nowl.merge.ns8", 8192, [8192], inp=IN_ATTN_MERGE, att_hd=128, att_ns=8, switches=dict(wave_local=0), ws="plain")

# ---- the legacy entry points (the diagnostics build keeps their description) ----------------------------------------------------------
for _name, (_dim, _inter, _qkv, _hd, _vocab) in MODELS.items():
    _dt = BF16 if _name in ("8b", "30b") else F16
    legacy(f"{_name}.sparse.wo", "sparse_gemv", _dim, _dim, dtype=_dt)
    legacy(f"{_name}.sparse.wo.plainws", "sparse_gemv", _dim, _dim, ws="plain", dtype=_dt)
    legacy(f"{_name}.sparse.down", "sparse_gemv", _inter, _dim, dtype=_dt)
    legacy(f"{_name}.dense.lm_head", "dense_gemv", _dim, _vocab, ws="none", dtype=_dt)
    legacy(f"{_name}.qkv", "sparse_qkv_gemv", _dim, sum(_qkv), N_q=_qkv[0], N_kv=_qkv[1], dtype=_dt)
    legacy(f"{_name}.qkv_ld", "sparse_qkv_gemv_ld", _dim, sum(_qkv), N_q=_qkv[0], N_kv=_qkv[1], ld=sum(_qkv) + 64, ws="plain", dtype=_dt)
    legacy(f"{_name}.qkv_i8", "sparse_qkv_gemv_i8", _dim, sum(_qkv), N_q=_qkv[0], N_kv=_qkv[1], ld=sum(_qkv), dtype=_dt)
    legacy(f"{_name}.qkv_i8.plainws", "sparse_qkv_gemv_i8", _dim, sum(_qkv), N_q=_qkv[0], N_kv=_qkv[1], ld=sum(_qkv), ws="plain", dtype=_dt)
    legacy(f"{_name}.gateup", "sparse_gateup_silu", _dim, _inter, dtype=_dt)
    legacy(f"{_name}.gateup.plainws", "sparse_gateup_silu", _dim, _inter, ws="plain", dtype=_dt)
legacy("refuse.sparse.ws.none", "sparse_gemv", 11008, 4096, ws="none")
legacy("refuse.sparse.ws.small", "sparse_gemv", 11008, 4096, ws="plain", ws_bytes=4096)
legacy("refuse.sparse.ws.misaligned", "sparse_gemv", 11008, 4096, ws="misaligned")
legacy("refuse.sparse.n4", "sparse_gemv", 4096, 4100)
legacy("refuse.sparse.dtype", "sparse_gemv", 4096, 4096, dtype=3)
legacy("refuse.sparse.z0", "sparse_gemv", 0, 4096)
legacy("refuse.dense.lds64k", "dense_gemv", 8192, 128256, ws="none")
legacy("long.sparse.reduce", "sparse_gemv", 65536, 4096, ws="plain")
legacy("refuse.qkv.split", "sparse_qkv_gemv", 4096, 6144, N_q=4096, N_kv=4096)
legacy("refuse.qkv_ld.ld", "sparse_qkv_gemv_ld", 4096, 6144, N_q=4096, N_kv=1024, ld=6140)
legacy("refuse.qkv_i8.split", "sparse_qkv_gemv_i8", 4096, 6144, N_q=4096, N_kv=512, ld=6144)
legacy("refuse.gateup.ws.none", "sparse_gateup_silu", 4096, 11008, ws="none")
legacy("refuse.gateup.ws.misaligned", "sparse_gateup_silu", 4096, 11008, ws="misaligned")
legacy("ragged.sparse", "sparse_gemv", 4100, 4104, ws="plain")
legacy("ragged.gateup", "sparse_gateup_silu", 4100, 11016, dtype=BF16)


# ---- a case over a memory ---------------------------------------------------------------------------------------------------------
def _wbytes(bits):
    return 2 if bits not in (8, 4) else 1


def zeros_bytes() -> int:
    """the zero arena: sized to the largest weight image of the table (and every input, all far smaller)"""
    need = 64 << 20
    for c in FUSED:
        if "no_launch" in c.get("tweak", ()) or not c["cols"]:
            continue
        ld = sum(c["cols"]) if c.get("images", 1) == 1 else max(c["cols"])
        rows = c["Z"] // 2 if c["bits"] == 4 else c["Z"]
        need = max(need, rows * (ld + 64) * _wbytes(c["bits"]) + 4096)
    for c in LEGACY:
        need = max(need, c["Z"] * (c.get("ld", c["N"]) + 64) * 2 + 4096)
    return need


def workspace(c, mem):
    """(pointer, bytes, prepared) of the caller's workspace of a case"""
    kind = c["ws"]
    if kind == "none":
        return None, 0, 0
    base = {"prepared": mem.ws, "plain": mem.plain, "misaligned": mem.plain + 8}[kind]
    return base, c.get("ws_bytes", WS_BYTES - 8 if kind == "misaligned" else WS_BYTES), int(kind == "prepared")


def materialise(c, mem):
    """(GemvIn, GemvOut, description buffer) of a FUSED case; the structs point into `mem` and into the buffer"""
    Z, cols, bits = c["Z"], c["cols"], c["bits"]
    null, tweak = set(c.get("null", ())), set(c.get("tweak", ()))
    zero, scr = mem.zeros, mem.scratch
    gin, gout = GemvIn(), GemvOut()
    gin.mode = c["inp"]
    if c["inp"] == IN_RESID_NORM:
        gin.resid_in, gin.norm_weight, gin.eps, gin.resid_out = zero, zero, 1e-5, scr + RESID_OFF
        gin.nslabs, gin.slabs_interleaved = c.get("nslabs", 0), c.get("in_il", 1)
        gin.slabs = zero if gin.nslabs > 0 else None
        if "row_index" in tweak:
            gin.row_index = zero
        if "resid_alias" in tweak:
            gin.resid_out = zero
    else:
        gin.x = zero
        gin.masks = zero if c["inp"] == IN_MASKED else None
        gin.att_head_dim, gin.att_nsplit = c.get("att_hd", 0), c.get("att_ns", 0)
        gin.gate_activated = c.get("gate_activated", 0)
    for name, field in (("x", "x"), ("masks", "masks"), ("norm_weight", "norm_weight"), ("slabs_in", "slabs")):
        if name in null:
            setattr(gin, field, None)
    gout.nseg, gout.mode, gout.weight_bits = len(cols), c["out"], bits
    gout.groupsize = c.get("groupsize", 0)
    images = c.get("images", 1)
    total = sum(cols)
    col = 0
    for i, n in enumerate(cols[:3]):
        own = images > 1  # one image per segment: every segment starts at column 0 of an image as wide as itself
        gout.w[i] = zero + ("w_plus8" in tweak) * 8
        gout.ld[i] = (n if own else total) + ("ld_4" in tweak) * 4
        gout.col0[i] = (0 if own else col) + ("col0_4" in tweak) * 4
        gout.ncols[i], gout.tau[i] = n, 0.5
        gout.y[i] = scr + Y_OFF + 2 * col + ("y_apart" in tweak) * 64 * i
        if bits == 8:
            gout.scale[i] = zero + 2 * col + ("scales_apart" in tweak) * 64 * i
        elif bits == 4:
            gout.scale[i], gout.scale_ld[i] = zero, gout.ld[i]
        col += n
    if "w0" in null:
        gout.w[0] = None
    if "y0" in null:
        gout.y[0] = None
    if "scale0" in null:
        gout.scale[0] = None
    gout.act_seg0 = c.get("act_seg0", 0)
    if c["out"] in (OUT_SLABS, OUT_SLAB_SUM, OUT_QKV_ROPE):
        gout.slabs = None if "out_slabs" in null else scr + SLABS_OFF + ("slabs_plus8" in tweak) * 8
        gout.slabs_bytes = c.get("slabs_bytes", 32 * total * 4 if c["out"] != OUT_SLAB_SUM else total * 4)
        gout.slabs_interleaved = c.get("out_il", 1) if c["out"] != OUT_SLAB_SUM else 0
        assert gout.slabs_bytes + 8 <= SLABS_ROOM, c["id"]
    if c["out"] == OUT_PAIR_SILU:
        gout.mask_out, gout.mask_tau = scr + MASK_OFF, 0.5
    if c["out"] == OUT_QKV_ROPE:
        gout.rope, gout.rope_pos, gout.k_cache, gout.v_cache = zero, zero, scr + KC_OFF, scr + VC_OFF
        gout.rope_head_dim, gout.rope_max_seq = c.get("rope_hd", 128), MAX_SEQ
        for name in ("rope", "rope_pos", "k_cache"):
            if name in null:
                setattr(gout, name, None)
    desc = ctypes.create_string_buffer(160)
    gout.desc, gout.desc_bytes = ctypes.addressof(desc), 160
    if mem.zeros_bytes is not None and cols and "no_launch" not in tweak:  # a real launch: every image inside the arena
        rows = Z // 2 if bits == 4 else Z
        assert rows * max(gout.ld[i] for i in range(len(cols[:3]))) * _wbytes(bits) + 64 <= mem.zeros_bytes, c["id"]
        assert total * 2 <= RESID_OFF and Z * 2 <= MASK_OFF - RESID_OFF and max(cols) * MAX_SEQ * 2 <= VC_OFF - KC_OFF, c["id"]
    return gin, gout, desc


def set_switches(D, sw) -> None:
    """the diagnostics build's switches for a case (sw None or {}: the defaults)"""
    sw = sw or {}
    assert D.teal_set_tuning(sw.get("lpr", 0), 0, sw.get("split", 0), 0) == 0
    D.teal_set_fast(sw.get("fast", 1))
    D.teal_set_wave_local(sw.get("wave_local", 1))


def call_fused(L, c, mem, stream=None):
    """teal_fused_gemv of a case through library L -> (return code, *nslabs_out or None, description)"""
    gin, gout, desc = materialise(c, mem)
    ws, ws_bytes, _ = workspace(c, mem)
    ns = ctypes.c_int(-1)
    ns_ref = None if "nslabs_out" in c.get("null", ()) else ctypes.byref(ns)
    rc = L.teal_fused_gemv(ctypes.byref(gin), ctypes.byref(gout), c["Z"], c["dtype"], ws, ws_bytes, ns_ref, stream)
    return rc, (ns.value if ns.value != -1 else None), desc.value.decode()


def call_plan(L, c, num_cu, mem=FAKE):
    """teal_fused_gemv_plan of the same case -> the same triple, without a device"""
    gin, gout, desc = materialise(c, mem)
    _, ws_bytes, prepared = workspace(c, mem)
    ns = ctypes.c_int(-1)
    ns_ref = None if "nslabs_out" in c.get("null", ()) else ctypes.byref(ns)
    rc = L.teal_fused_gemv_plan(ctypes.byref(gin), ctypes.byref(gout), c["Z"], c["dtype"], prepared, ws_bytes, num_cu, ns_ref)
    return rc, (ns.value if ns.value != -1 else None), desc.value.decode()


def call_legacy(D, c, mem, stream=None):
    """a legacy entry point through the diagnostics build D -> (return code, description of the launch it made or "")"""
    Z, N, dt = c["Z"], c["N"], c["dtype"]
    ws, ws_bytes, _ = workspace(c, mem)
    x, w, y, tau = mem.zeros, mem.zeros, mem.scratch + Y_OFF, 0.5
    fn = c["fn"]
    if fn == "sparse_gemv":
        rc = D.teal_sparse_gemv(x, w, y, tau, Z, N, dt, ws, ws_bytes, stream)
    elif fn == "dense_gemv":
        rc = D.teal_dense_gemv(x, w, y, Z, N, dt, ws, ws_bytes, stream)
    elif fn == "sparse_qkv_gemv":
        rc = D.teal_sparse_qkv_gemv(x, w, y, tau, tau, tau, Z, N, c["N_q"], c["N_kv"], dt, ws, ws_bytes, stream)
    elif fn == "sparse_qkv_gemv_ld":
        rc = D.teal_sparse_qkv_gemv_ld(x, w, c["ld"], y, tau, tau, tau, Z, N, c["N_q"], c["N_kv"], dt, ws, ws_bytes, stream)
    elif fn == "sparse_qkv_gemv_i8":
        rc = D.teal_sparse_qkv_gemv_i8(x, w, mem.zeros, y, tau, tau, tau, Z, N, c["N_q"], c["N_kv"], c["ld"], dt, ws, ws_bytes, stream)
    elif fn == "sparse_gateup_silu":
        rc = D.teal_sparse_gateup_silu(x, w, w, y, tau, tau, Z, N, dt, ws, ws_bytes, stream)
    else:
        raise KeyError(fn)
    return rc, (D.teal_last_launch_desc().decode() if rc == 0 else "")


def is_diag(c) -> bool:
    return bool(c.get("switches"))


# ---- device memory for real launches ------------------------------------------------------------------------------------------------
_SHARED: dict = {}


def device_memory(L) -> Memory:
    """the arenas on the current GPU (allocated once per process) and a workspace prepared through library L (a workspace prepared
    through one build of the library is plain memory to another)"""
    import torch
    if not _SHARED:
        for name, nbytes in (("zeros", zeros_bytes()), ("scratch", SCRATCH_BYTES), ("plain", WS_BYTES)):
            _SHARED[name] = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(WS_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.teal_workspace_init(ws.data_ptr(), WS_BYTES, None) == 0
    mem = Memory(_SHARED["zeros"].data_ptr(), _SHARED["scratch"].data_ptr(), ws.data_ptr(), _SHARED["plain"].data_ptr(),
                 zeros_bytes=_SHARED["zeros"].numel())
    mem.keep = ws
    return mem


def run_table(L, D):
    """every case as a real launch on the current GPU -> ({id: [rc, nslabs, desc]}, {id: [rc, desc]}): product cases through L,
    the switch cases and the legacy entries through the diagnostics build D"""
    import torch
    mem_l, mem_d = device_memory(L), device_memory(D)
    got_fused, got_legacy = {}, {}
    for c in FUSED:
        if is_diag(c):
            set_switches(D, c["switches"])
            got_fused[c["id"]] = list(call_fused(D, c, mem_d))
            set_switches(D, None)
        else:
            got_fused[c["id"]] = list(call_fused(L, c, mem_l))
    for c in LEGACY:
        got_legacy[c["id"]] = list(call_legacy(D, c, mem_d))
    torch.cuda.synchronize()
    L.teal_workspace_release(mem_l.ws)
    D.teal_workspace_release(mem_d.ws)
    return got_fused, got_legacy
