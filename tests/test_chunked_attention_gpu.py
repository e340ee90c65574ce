"""GPU: the chunked split-KV attention body (teal_amd/csrc/teal_chunked_attention.h) behind teal_verify_attention,
teal_batched_decode_attention and teal_batched_decode_attention_slots.

  * every case of tests/chunked_attention_cases.py leaves the yt bits (all slots) and the K / V cache rows that the commit before
    the two kernels were folded left (tests/golden/chunked_attention_parent.json, scripts/record_chunked_attention.py), and
    touches no other cache row;
  * DESIGN §6c as a test: sequence b of a batched launch IS teal_verify_attention at T = 1 on that sequence's slot, bit for
    bit — yt[:, b] and the new cache rows.
"""
import json
import os

import pytest
import torch

import chunked_attention_cases as C
from teal_amd import _lib, runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chunked_attention_parent.json")) as _f:
    RECORD = json.load(_f)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("heads", C.HEADS, ids=lambda h: "h%d_%d_%d" % h)
def test_bits_are_the_parents(heads, dtype):
    L = _lib.load()
    runtime.init()
    if L.teal_init() != RECORD["num_cu"]:
        pytest.skip(f"the record is of a device with {RECORD['num_cu']} CUs, this one has {L.teal_init()}: nsplit, and with it "
                    "the order of the merge, depends on the count")
    got = C.run_group(L, heads, dtype, runtime.stream_ptr())
    want = {k: RECORD["cases"][k] for k in got}
    bad = [(k, got[k], want[k]) for k in got if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(got)} cases differ (id, launch, record): {bad[:4]}"


def test_the_record_holds_exactly_the_cases():
    ids = [c[0] for h, d in C.GROUPS for c in C.group_cases(h, d)]
    assert len(set(ids)) == len(ids) and set(ids) == set(RECORD["cases"])


# positions per (max_seq, B): row 0, the chunk boundary (31 and 32) and the last row are all covered at each cache length
SAME_POS = {(32, 3): (0, 15, 31), (32, 8): (0, 1, 15, 16, 30, 31, 31, 0),
            (64, 3): (31, 32, 63), (64, 8): (0, 5, 31, 32, 33, 62, 63, 32)}


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("max_seq", [32, 64])
@pytest.mark.parametrize("heads", C.HEADS, ids=lambda h: "h%d_%d_%d" % h)
def test_a_batched_sequence_is_the_verify_pass_at_one_token(heads, max_seq, B, dtype):
    L = _lib.load()
    runtime.init()
    n_head, n_kv, hd = heads
    dt = getattr(torch, dtype)
    # the same nsplit on both sides: one chunk is one split anywhere; two chunks are two splits on both sides while the batched
    # grid (n_kv * groups * B workgroups per split, groups = 1 up to 16 heads per KV head) does not exceed the CUs
    assert n_head // n_kv <= 16
    if max_seq > 32:
        assert n_kv * B <= torch.cuda.get_device_properties(0).multi_processor_count
    pos = SAME_POS[(max_seq, B)]
    slabs, rope, kc, vc = C.make_inputs(f"same-{heads}-{max_seq}-{B}-{dtype}", heads, dtype, B, 8, max_seq)
    for b, p in enumerate(pos):
        kc[b, :, p:] = C.SENTINEL
        vc[b, :, p:] = C.SENTINEL
    slabs, rope = slabs.to(DEV), rope.to(DEV)
    kb, vb = kc.to(DEV), vc.to(DEV)
    yb = torch.full((n_head * hd, 8), 5.0, device=DEV, dtype=dt)
    rc = C.launch(L, "batched", slabs, rope, pos, kb, vb, yb, B, heads, dtype, max_seq, runtime.stream_ptr())
    _lib.check(rc, "teal_batched_decode_attention")
    for b, p in enumerate(pos):
        s1 = torch.zeros_like(slabs)
        s1[:, :, 0] = slabs[:, :, b]
        k1, v1 = kc[b:b + 1].to(DEV), vc[b:b + 1].to(DEV)
        y1 = torch.full((n_head * hd, 8), 5.0, device=DEV, dtype=dt)
        rc = C.launch(L, "verify", s1, rope, (p,), k1, v1, y1, 1, heads, dtype, max_seq, runtime.stream_ptr())
        _lib.check(rc, "teal_verify_attention")
        assert torch.equal(yb[:, b].view(torch.int16), y1[:, 0].view(torch.int16)), (b, p, "yt")
        assert torch.equal(kb[b].view(torch.int16), k1[0].view(torch.int16)), (b, p, "k cache")
        assert torch.equal(vb[b].view(torch.int16), v1[0].view(torch.int16)), (b, p, "v cache")
        assert not bool((kb[b, :, p] == C.SENTINEL).all()) and not y1[:, 1:].float().any()
