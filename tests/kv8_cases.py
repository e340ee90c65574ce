"""The cases of tests/test_kv8_gpu.py, built on the CPU so that tests/test_kv8_rule_host.py can check their preconditions without a
GPU: crafted and random rows for teal_kv8_quantize_rows, and the caches of the attention cases (chunked_attention_cases.py's inputs
with every cache row moved to a binade of its own).
"""
import numpy as np
import torch

import chunked_attention_cases as C
import kv8_rule as R

CODE_SENTINEL = 0x5A      # in every code byte a launch must not write
SCALE_SENTINEL = -7.0     # in every scale word a launch must not write (no power of two)
QUANT_HEADS = (2, 8)
QUANT_ROWS = (0, 1, 33)
QUANT_TENSORS = 3
SRC_HEAD_ROWS, DST_HEAD_ROWS = 40, 37   # unequal head strides
LONG = (1040, 1039)                      # max_seq, position of the long attention case
ATTN_B = {1: 0b1, 3: C.SLOT_MASKS[3], 8: C.SLOT_MASKS[8]}


def _from_bits(bits, dt):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint16).astype(np.int16)).view(dt)


def _bits(x):
    return x.contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF


def crafted_rows(dtype, hd):
    """{name: 16-bit row [hd]}: every corner the rule names.  Each row's stated maximum IS its maximum."""
    dt = getattr(torch, dtype)
    rows = {}

    def row(name, head, fill=0.0):
        r = torch.full((hd,), fill, dtype=torch.float32)
        r[:len(head)] = torch.tensor(head, dtype=torch.float32)
        r16 = r.to(dt)
        assert torch.equal(r16.to(torch.float32), r), name   # the values are the 16-bit dtype's
        rows[name] = r16

    for e in (-9, -1, 0, 1, 7):
        a = 448.0 * 2.0 ** e
        row(f"amax=448*2^{e}", [a, -a / 2, a / 448.0])
        nxt = _from_bits([int(_bits(torch.tensor([a]).to(dt))[0]) + 1], dt)[0].item()   # the next 16-bit value above
        row(f"amax=next above 448*2^{e}", [nxt, -a, a / 4])
    row("zeros", [0.0])
    row("negative zeros", [-0.0, 0.0, -0.0], fill=-0.0)
    row("-0 beside values", [-0.0, 3.0, -448.0, 0.0])
    # ties at scale 1 (amax 448): 17 / 19 / 21 / 23 lie half-way on the step-2 grid of [16, 32): even and odd lower neighbours
    row("ties both parities", [448.0, 17.0, -17.0, 19.0, -19.0, 21.0, 23.0, 1.0625, 1.1875, -1.0625, 0.0009765625, 0.0029296875])
    # results in the e4m3 subnormals (below 2^-6) and under half the smallest (-> +-0 with the sign)
    row("subnormal results", [448.0, 2.0 ** -7, -(2.0 ** -7), 3 * 2.0 ** -9, 2.0 ** -9, 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -11, 2.0 ** -12,
                               -(2.0 ** -12), 2.0 ** -6, 15 * 2.0 ** -10])
    if dtype == "bfloat16":
        row("clamp at -100", [2.0 ** -120, -(2.0 ** -118), 2.0 ** -125])     # e would be -128
        row("just above the clamp", [448.0 * 2.0 ** -100, 2.0 ** -101])      # e = -100 exactly, unclamped
        row("bf16 subnormal", [2.0 ** -130, -(2.0 ** -133)])
        row("large", [2.0 ** 120, -(2.0 ** 100), 1.0])
    else:
        row("fp16 subnormals", [2.0 ** -24, -(2.0 ** -20), 3 * 2.0 ** -24])
        row("fp16 max", [65504.0, -1.0, 0.5])
    return rows


def quant_source(dtype, hd, n_heads):
    """the source caches [QUANT_TENSORS][n_heads][SRC_HEAD_ROWS][hd]: random rows whose magnitudes span 2^-12 .. 2^12, the crafted
    rows dealt over the (tensor, head) pairs from row 0 down (rows = 1 reaches the first of each pair)"""
    dt = getattr(torch, dtype)
    rng = np.random.default_rng(hd * 131 + n_heads * 7 + (dtype == "bfloat16"))
    shape = (QUANT_TENSORS, n_heads, SRC_HEAD_ROWS, hd)
    mag = np.exp2(rng.integers(-12, 13, size=shape[:3] + (1,)).astype(np.float64))
    src = torch.from_numpy(((rng.random(shape) * 2.0 - 1.0) * mag).astype(np.float32)).to(dt)
    pairs = QUANT_TENSORS * n_heads
    for i, r in enumerate(crafted_rows(dtype, hd).values()):
        t, h = divmod(i % pairs, n_heads)
        assert i // pairs < min(QUANT_ROWS[-1], SRC_HEAD_ROWS)
        src[t, h, i // pairs] = r
    return src


def attention_caches(case_id, heads, dtype, B, max_seq=C.MAX_SEQ):
    """(slabs, rope, kc, vc) of C.make_inputs with cache row r of head h of sequence s moved by 2^j, j = (3 r + h + s) mod 7 - 3:
    neighbouring rows sit three binades apart and the rows of a head span 2^6"""
    dt = getattr(torch, dtype)
    slabs, rope, kc, vc = C.make_inputs(case_id, heads, dtype, B, 8, max_seq)
    n_kv = heads[1]
    s, h, r = torch.meshgrid(torch.arange(B), torch.arange(n_kv), torch.arange(max_seq), indexing="ij")
    move = torch.exp2(((3 * r + h + s) % 7 - 3).to(torch.float32))[..., None]
    kc = (kc.to(torch.float32) * move).to(dt)
    vc = (vc.to(torch.float32) * torch.roll(move, 1, dims=2)).to(dt)
    return slabs, rope, kc, vc


def attention_case(case_id, heads, dtype, B, pos, max_seq=C.MAX_SEQ):
    """everything a kv8 attention case needs, on the CPU: the 16-bit caches, their codes and scales by the host rule, and the 16-bit
    caches that hold the dequantised values.  Rows at and past a sequence's position hold sentinels in all three."""
    dt = getattr(torch, dtype)
    slabs, rope, kc, vc = attention_caches(case_id, heads, dtype, B, max_seq)
    out = {"slabs": slabs, "rope": rope, "k16": kc, "v16": vc}
    for name, c in (("k", kc), ("v", vc)):
        codes, scales = R.quantize(c)
        dq = R.dequantize(codes, scales)
        out[name + "_exact"] = R.representable(dq, dt)
        dq = dq.to(dt)
        for b, p in enumerate(pos):
            codes[b, :, p:] = CODE_SENTINEL
            scales[b, :, p:] = SCALE_SENTINEL
            dq[b, :, p:] = C.SENTINEL
        out[name + "_codes"], out[name + "_scales"], out[name + "_dq"] = codes, scales, dq
    return out


def attention_ids():
    """(id, heads, dtype, B, positions, mask, max_seq) of every attention case"""
    out = []
    for heads in C.HEADS:
        for dtype in C.DTYPES:
            for B, mask in ATTN_B.items():
                for m in sorted({mask, (1 << B) - 1}):
                    out.append(("kv8-h%d_%d_%d-%s-B%d-m%s" % (*heads, dtype, B, bin(m)), heads, dtype, B, C.BATCHED_POS[B], m, C.MAX_SEQ))
    for dtype in C.DTYPES:
        out.append((f"kv8-long-{dtype}", C.HEADS[2], dtype, 1, (LONG[1],), 1, LONG[0]))
    return out
