"""The cases of tests/test_chunked_attention_gpu.py and scripts/record_chunked_attention.py: the chunked split-KV attention of the
verify pass (teal_verify_attention) and of the batched step (teal_batched_decode_attention, ..._slots), both typed once in
teal_amd/csrc/teal_chunked_attention.h.

Inputs come from a seeded numpy generator on the CPU (uniform doubles only, rounded to the 16-bit dtype by torch on the CPU), so
the same case holds the same bits wherever it is built.  The rope table is uniform in (-1, 1) as well, not cos / sin: these cases
pin bits, and a libm's last place must not reach them.  Cache rows at and past a sequence's position hold a sentinel, the yt
buffer is pre-filled, and the workspace is NaN, so a row read from the wrong place or a slot left unwritten changes a hash.

A case's record is {"yt": sha256 of ALL KR (verify) or 8 (batched) slots of yt, "kv": sha256 of the written K rows then V rows};
run_case also asserts that every other cache row kept its bits.
"""
import hashlib

import numpy as np
import torch

MAX_SEQ = 96  # three 32-row chunks: nsplit = 3 on any part with at least 96 CUs, so the split order is exercised
SPLIT = 2     # slabs per column
HEADS = ((8, 2, 64), (8, 8, 64), (32, 8, 128))
DTYPES = ("float16", "bfloat16")
VERIFY_T = (1, 5, 8, 9, 16)
BATCHED_POS = {1: (32,), 3: (0, 31, 95), 8: (95, 0, 5, 31, 32, 32, 5, 95)}
SLOT_MASKS = {3: 0b101, 8: 0b10110101}
SENTINEL = -3.0
CODE = {"float16": 0, "bfloat16": 1}


def verify_p0(T):
    return (0, 31, 40, MAX_SEQ - T)


def group_cases(heads, dtype):
    """the cases of one (heads, dtype) group: (id, kind, rows, positions, mask)"""
    tag = "h%d_%d_%d-%s" % (*heads, dtype)
    out = []
    for T in VERIFY_T:
        for p0 in verify_p0(T):
            out.append((f"verify-{tag}-T{T}-p{p0}", "verify", T, (p0,), None))
    for B, pos in BATCHED_POS.items():
        out.append((f"batched-{tag}-B{B}", "batched", B, pos, None))
    for B, mask in SLOT_MASKS.items():
        out.append((f"slots-{tag}-B{B}-m{mask:#b}", "slots", B, BATCHED_POS[B], mask))
    return out


GROUPS = [(h, d) for h in HEADS for d in DTYPES]


def _seed(case_id):
    return int.from_bytes(hashlib.sha256(case_id.encode()).digest()[:8], "little")


def _uniform(rng, shape, scale):
    return torch.from_numpy(((rng.random(shape) * 2.0 - 1.0) * scale).astype(np.float32))


def make_inputs(case_id, heads, dtype, nseq, kr, max_seq=MAX_SEQ):
    """CPU tensors of one case: slabs fp32 [SPLIT][(n_head + 2 n_kv) hd][kr], rope [max_seq][hd / 2][2], caches [nseq][n_kv][max_seq][hd]"""
    n_head, n_kv, hd = heads
    dt = getattr(torch, dtype)
    rng = np.random.default_rng(_seed(case_id))
    slabs = _uniform(rng, (SPLIT, (n_head + 2 * n_kv) * hd, kr), 0.7)
    rope = _uniform(rng, (max_seq, hd // 2, 2), 1.0).to(dt)
    kc = _uniform(rng, (nseq, n_kv, max_seq, hd), 0.5).to(dt)
    vc = _uniform(rng, (nseq, n_kv, max_seq, hd), 0.5).to(dt)
    return slabs, rope, kc, vc


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.int16).cpu().numpy().tobytes())
    return h.hexdigest()


def launch(L, kind, slabs, rope, pos, kc, vc, yt, rows, heads, dtype, max_seq, stream, mask=None):
    """one launch on device tensors (the caches and yt are written in place); returns the return code"""
    n_head, n_kv, hd = heads
    dev = slabs.device
    pos_d = torch.tensor(list(pos), device=dev, dtype=torch.int32)
    if kind == "verify":
        nb = int(L.teal_verify_attention_ws_bytes(rows, n_head, hd))
    else:
        nb = int(L.teal_batched_decode_attention_ws_bytes(rows, n_head, hd))
    parts = torch.full(((nb + 3) // 4,), float("nan"), device=dev, dtype=torch.float32)
    a = (slabs.data_ptr(), SPLIT, rope.data_ptr(), pos_d.data_ptr())
    b = (kc.data_ptr(), vc.data_ptr(), yt.data_ptr(), parts.data_ptr(), parts.numel() * 4, rows, n_head, n_kv, hd, max_seq, CODE[dtype], stream)
    if kind == "verify":
        rc = L.teal_verify_attention(*a, *b)
    elif kind == "batched":
        rc = L.teal_batched_decode_attention(*a, *b)
    else:
        act = torch.tensor([mask], device=dev, dtype=torch.int32)
        rc = L.teal_batched_decode_attention_slots(*a, act.data_ptr(), *b)
    torch.cuda.synchronize()
    return rc


def run_case(L, case, heads, dtype, stream, dev="cuda"):
    """launch one case; {"yt": ..., "kv": ...} of what it left"""
    case_id, kind, rows, pos, mask = case
    n_head, n_kv, hd = heads
    dt = getattr(torch, dtype)
    verify = kind == "verify"
    kr = (8 if rows <= 8 else 16) if verify else 8
    nseq = 1 if verify else rows
    slabs, rope, kc, vc = make_inputs(case_id, heads, dtype, nseq, kr)
    written = torch.zeros(nseq, MAX_SEQ, dtype=torch.bool)
    for s in range(nseq):
        p = pos[0] if verify else pos[s]
        kc[s, :, p:] = SENTINEL  # the rows this launch writes and everything after them
        vc[s, :, p:] = SENTINEL
        if mask is None or (mask >> s) & 1:
            written[s, p:p + (rows if verify else 1)] = True
    k0, v0 = kc.clone(), vc.clone()
    kd, vd = kc.to(dev), vc.to(dev)
    yt = torch.full((n_head * hd, kr), 5.0, device=dev, dtype=dt)
    rc = launch(L, kind, slabs.to(dev), rope.to(dev), pos, kd, vd, yt, rows, heads, dtype, MAX_SEQ, stream, mask)
    assert rc == 0, (case_id, rc)
    k1, v1 = kd.cpu(), vd.cpu()
    keep = ~written
    for s in range(nseq):  # every row outside the written ones keeps its bits
        assert torch.equal(k1[s][:, keep[s]].view(torch.int16), k0[s][:, keep[s]].view(torch.int16)), (case_id, s, "k")
        assert torch.equal(v1[s][:, keep[s]].view(torch.int16), v0[s][:, keep[s]].view(torch.int16)), (case_id, s, "v")
    krows = [k1[s][:, written[s]] for s in range(nseq)]
    vrows = [v1[s][:, written[s]] for s in range(nseq)]
    return {"yt": _sha(yt), "kv": _sha(*krows, *vrows)}


def run_group(L, heads, dtype, stream):
    return {c[0]: run_case(L, c, heads, dtype, stream) for c in group_cases(heads, dtype)}
