"""GPU: the two entry points of the fp8 KV cache (teal_amd/csrc/teal_kv8.hip), with no tolerance anywhere.

  * teal_kv8_quantize_rows: codes and scales bit for bit against tests/kv8_rule.py on the crafted rows (tests/kv8_cases.py) and on
    random rows, a sentinel in every byte and scale word outside the written rows, and the refusals;
  * teal_batched_decode_attention_slots_kv8: dequantisation is exact and everything after the staging loop is the 16-bit launch's
    source, so yt must hold the WORDS teal_batched_decode_attention_slots leaves on a 16-bit cache of the dequantised values; the
    appended row's codes and scale are the rule applied to the row the 16-bit launch appended; nothing else is written.
"""
import pytest
import torch

import chunked_attention_cases as C
import kv8_cases as K
import kv8_rule as R
from teal_amd import _lib, runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _table(tensors):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(DEV)


@pytest.mark.parametrize("rows", K.QUANT_ROWS)
@pytest.mark.parametrize("n_heads", K.QUANT_HEADS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_quantize_rows_is_the_rule(dtype, hd, n_heads, rows):
    L = _lib.load()
    runtime.init()
    src = K.quant_source(dtype, hd, n_heads)
    want_codes, want_scales = R.quantize(src[:, :, :rows])
    srcs = [src[t].to(DEV) for t in range(K.QUANT_TENSORS)]
    codes = [torch.full((n_heads, K.DST_HEAD_ROWS, hd), K.CODE_SENTINEL, dtype=torch.uint8, device=DEV) for _ in srcs]
    scales = [torch.full((n_heads, K.DST_HEAD_ROWS), K.SCALE_SENTINEL, dtype=torch.float32, device=DEV) for _ in srcs]
    tables = [_table(srcs), _table(codes), _table(scales)]  # (held: a dropped table's memory is the next one's)
    rc = L.teal_kv8_quantize_rows(tables[0].data_ptr(), tables[1].data_ptr(), tables[2].data_ptr(), K.QUANT_TENSORS, n_heads, hd,
                                  rows, K.SRC_HEAD_ROWS, K.DST_HEAD_ROWS, C.CODE[dtype], runtime.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    for t in range(K.QUANT_TENSORS):
        c, s = codes[t].cpu(), scales[t].cpu()
        assert torch.equal(s[:, :rows].view(torch.int32), want_scales[t].view(torch.int32)), (t, "scales")
        bad = (c[:, :rows] != want_codes[t]).nonzero()
        assert bad.numel() == 0, (t, bad[:4].tolist(), c[:, :rows][tuple(bad[0])].item(), want_codes[t][tuple(bad[0])].item())
        assert bool((c[:, rows:] == K.CODE_SENTINEL).all()) and bool((s[:, rows:] == K.SCALE_SENTINEL).all()), (t, "outside the rows")


def test_quantize_rows_refusals():
    L = _lib.load()
    runtime.init()
    t = torch.zeros(8, dtype=torch.int64, device=DEV)
    p, st = t.data_ptr(), runtime.stream_ptr()
    q = L.teal_kv8_quantize_rows
    assert q(p, p, p, 2, 2, 64, 0, 4, 4, 0, st) == 0                       # rows == 0: nothing launched, nothing read
    assert q(None, p, p, 2, 2, 64, 1, 4, 4, 0, st) == -1 and q(p, None, p, 2, 2, 64, 1, 4, 4, 0, st) == -1
    assert q(p, p, None, 2, 2, 64, 1, 4, 4, 0, st) == -1
    assert q(p, p, p, 0, 2, 64, 1, 4, 4, 0, st) == -1 and q(p, p, p, 2, 0, 64, 1, 4, 4, 0, st) == -1 and q(p, p, p, 2, 2, 64, -1, 4, 4, 0, st) == -1
    assert q(p, p, p, 2, 2, 64, 1, 4, 4, 2, st) == -2
    assert q(p, p, p, 2, 2, 96, 1, 4, 4, 0, st) == -3 and q(p, p, p, 2, 2, 64, 5, 4, 8, 0, st) == -3 and q(p, p, p, 2, 2, 64, 5, 8, 4, 0, st) == -3
    assert q(p, p, p, 65536, 2, 64, 1, 4, 4, 0, st) == -3 and q(p, p, p, 2, 65536, 64, 1, 4, 4, 0, st) == -3
    assert q(p + 4, p, p, 2, 2, 64, 1, 4, 4, 0, st) == -4 and q(p, p, p + 4, 2, 2, 64, 1, 4, 4, 0, st) == -4
    torch.cuda.synchronize()


def _launch_kv8(L, c, pos, mask, B, heads, dtype, max_seq, kc, vc, ks, vs, yt):
    n_head, n_kv, hd = heads
    pos_d = torch.tensor(list(pos), device=DEV, dtype=torch.int32)
    act = torch.tensor([mask], device=DEV, dtype=torch.int32)
    nb = int(L.teal_batched_decode_attention_ws_bytes(B, n_head, hd))
    parts = torch.full(((nb + 3) // 4,), float("nan"), device=DEV, dtype=torch.float32)
    rc = L.teal_batched_decode_attention_slots_kv8(c["slabs"].data_ptr(), C.SPLIT, c["rope"].data_ptr(), pos_d.data_ptr(), act.data_ptr(),
                                                   kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), yt.data_ptr(), parts.data_ptr(),
                                                   parts.numel() * 4, B, n_head, n_kv, hd, max_seq, C.CODE[dtype], runtime.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", K.attention_ids(), ids=lambda c: c[0])
def test_attention_is_the_16bit_launch_on_the_dequantised_cache(case):
    case_id, heads, dtype, B, pos, mask, max_seq = case
    L = _lib.load()
    runtime.init()
    n_head, n_kv, hd = heads
    dt = getattr(torch, dtype)
    host = K.attention_case(case_id, heads, dtype, B, pos, max_seq)
    assert host["k_exact"] and host["v_exact"]
    c = {k: v.to(DEV) for k, v in host.items() if isinstance(v, torch.Tensor)}
    # the 16-bit launch on the dequantised values
    y16 = torch.full((n_head * hd, 8), 5.0, device=DEV, dtype=dt)
    rc = C.launch(L, "slots", c["slabs"], c["rope"], pos, c["k_dq"], c["v_dq"], y16, B, heads, dtype, max_seq, runtime.stream_ptr(), mask)
    assert rc == 0
    # the fp8 launch on the codes
    y8 = torch.full((n_head * hd, 8), 5.0, device=DEV, dtype=dt)
    rc = _launch_kv8(L, c, pos, mask, B, heads, dtype, max_seq, c["k_codes"], c["v_codes"], c["k_scales"], c["v_scales"], y8)
    assert rc == 0
    assert torch.equal(y8.view(torch.int16), y16.view(torch.int16)), case_id
    active = [b for b in range(B) if (mask >> b) & 1]
    assert not y8[:, [b for b in range(8) if b not in active]].float().any()    # inactive and absent slots: zero
    assert all(bool(y8[:, b].float().any()) for b in active)
    for name in ("k", "v"):
        codes, scales, new16 = c[name + "_codes"].cpu(), c[name + "_scales"].cpu(), c[name + "_dq"].cpu()
        for b, p in enumerate(pos):
            keep = torch.ones(max_seq, dtype=torch.bool)
            if b in active:  # the appended row: the rule applied to the row the 16-bit launch appended
                keep[p] = False
                assert not bool((new16[b, :, p] == C.SENTINEL).all())
                want_c, want_s = R.quantize(new16[b, :, p])
                assert torch.equal(codes[b, :, p], want_c) and torch.equal(scales[b, :, p].view(torch.int32), want_s.view(torch.int32)), (name, b, p)
            assert torch.equal(codes[b][:, keep], host[name + "_codes"][b][:, keep]), (name, b, "codes outside the new row")
            assert torch.equal(scales[b][:, keep].view(torch.int32), host[name + "_scales"][b][:, keep].view(torch.int32)), (name, b, "scales")


def test_attention_refusals():
    L = _lib.load()
    runtime.init()
    heads, dtype, B, pos = C.HEADS[0], "float16", 1, (5,)
    host = K.attention_case("kv8-refusals", heads, dtype, B, pos)
    c = {k: v.to(DEV) for k, v in host.items() if isinstance(v, torch.Tensor)}
    y = torch.zeros(heads[0] * heads[2], 8, device=DEV, dtype=torch.float16)
    a = (L, c, pos, 1, B, heads, dtype, C.MAX_SEQ)
    before = c["k_codes"].clone()
    assert _launch_kv8(*a, c["k_codes"].view(-1)[1:], c["v_codes"], c["k_scales"], c["v_scales"], y) == -4   # codes off 16 bytes
    n_head, n_kv, hd = heads
    z = torch.zeros(4, device=DEV, dtype=torch.int32)
    f = L.teal_batched_decode_attention_slots_kv8
    full = [c["slabs"].data_ptr(), C.SPLIT, c["rope"].data_ptr(), z.data_ptr(), z.data_ptr(), c["k_codes"].data_ptr(), c["v_codes"].data_ptr(),
            c["k_scales"].data_ptr(), c["v_scales"].data_ptr(), y.data_ptr(), z.data_ptr(), 16, B, n_head, n_kv, hd, C.MAX_SEQ, 0, runtime.stream_ptr()]
    assert f(*full) == -5                                                    # partials too small
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10):
        assert f(*[None if j == i else v for j, v in enumerate(full)]) == -1, i
    assert f(*full[:17], 2, full[18]) == -2 and f(*full[:12], 9, *full[13:]) == -3 and f(*full[:15], 96, *full[16:]) == -3
    torch.cuda.synchronize()
    assert torch.equal(c["k_codes"], before)
