"""GPU: the hardware e4m3 conversions of teal_kv8.hip against the rule (tests/kv8_rule.py) on EVERYTHING, with no tolerance — the
rule is the specification, and v_cvt_pk_fp8_f32 / v_cvt_pk_f32_fp8 are allowed only because these pass.

  * encode: all 65536 bit patterns of each 16-bit dtype through teal_kv8_quantize_rows, in rows of fixed scale — element 0 of a row
    is the row's largest magnitude and pins e, the other 63 are the patterns that fit under it (NaN / Inf are outside the contract).
    Pins: 448 * 2^e over several e, the dtype's largest finite value (so every finite pattern is sent at least once) and, in bf16,
    a maximum under the -100 clamp; bf16's subnormal inputs ride in every row set.  Codes and scales bit for bit.
  * decode: all 254 non-NaN codes, each under several scales and in every byte of a 32-bit word, through the attention launch.
    V: with q = 0 and one cached row next to the (zero) new row the softmax is (1/2, 1/2) exactly, so yt IS float(code) * scale / 2.
    K: a one-hot q of a power of two picks one code per (sequence, head) into a score of magnitude 1 .. 2; yt must be the words
    the 16-bit launch leaves on the dequantised row, and moves with the score (four launches cover the codes).
"""
import numpy as np
import pytest
import torch

import chunked_attention_cases as C
import kv8_cases as K
import kv8_rule as R
from teal_amd import _lib, runtime
from test_kv8_gpu import _launch_kv8, _table

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = 64
CODES = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)  # the 254 codes that are numbers
HEADS = (8, 8, 64)   # one query head per KV head: yt column (h, d) of slot b reads cache row (b, h)
SEQ = 32             # one chunk, one split


def _pins(dtype):
    """the rows' largest magnitudes as 16-bit patterns, with the e each must give"""
    dt = getattr(torch, dtype)
    exps = (-8, -3, 0, 1, 3, 7) if dtype == "float16" else (-100, -40, -8, 0, 5, 60, 119)
    pins = [(int(K._bits(torch.tensor([448.0 * 2.0 ** e], dtype=torch.float64).to(dt))[0]), e) for e in exps]
    pins.append((0x7BFF, 8) if dtype == "float16" else (0x7F7F, 120))   # the largest finite value
    if dtype == "bfloat16":
        pins.append((int(K._bits(torch.tensor([2.0 ** -110], dtype=torch.float64).to(dt))[0]), -100))  # e would be -118: clamped
    return pins


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_every_bit_pattern_encodes_by_the_rule(dtype):
    L = _lib.load()
    runtime.init()
    dt = getattr(torch, dtype)
    bits = np.arange(1 << 16, dtype=np.int64)
    mag = bits & 0x7FFF
    inf = 0x7C00 if dtype == "float16" else 0x7F80
    rows, sent = [], np.zeros(1 << 16, dtype=bool)
    for pin, e in _pins(dtype):
        assert int(R.scale_exp(pin, dtype)) == e
        fit = bits[(mag < inf) & (mag <= pin)]   # (magnitudes order as their patterns do)
        sent[fit] = True
        fit = np.concatenate([fit, np.zeros(-len(fit) % (HD - 1), dtype=np.int64)]).reshape(-1, HD - 1)
        rows.append(np.concatenate([np.full((fit.shape[0], 1), pin, dtype=np.int64), fit], axis=1))
    assert bool(sent[mag < inf].all()) and not sent[mag >= inf].any()   # every finite pattern, nothing else
    src = K._from_bits(np.concatenate(rows), dt)                        # [n][HD]
    n = src.shape[0]
    want_codes, want_scales = R.quantize(src)
    src_d = src.to(DEV)
    codes = torch.full((n + 1, HD), K.CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    scales = torch.full((n + 1,), K.SCALE_SENTINEL, dtype=torch.float32, device=DEV)
    tables = [_table([src_d]), _table([codes]), _table([scales])]
    rc = L.teal_kv8_quantize_rows(tables[0].data_ptr(), tables[1].data_ptr(), tables[2].data_ptr(), 1, 1, HD, n, n, n + 1, C.CODE[dtype],
                                  runtime.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    codes, scales = codes.cpu(), scales.cpu()
    assert torch.equal(scales[:n].view(torch.int32), want_scales.view(torch.int32))
    bad = (codes[:n] != want_codes).nonzero()
    assert bad.numel() == 0, (len(bad), [(hex(int(K._bits(src[r, d:d + 1])[0])), int(codes[r, d]), int(want_codes[r, d])) for r, d in bad[:6].tolist()])
    assert bool((codes[n] == K.CODE_SENTINEL).all()) and scales[n].item() == K.SCALE_SENTINEL


def _decode_inputs(dtype, B):
    """zero slabs, the identity rotation, and caches of one cached row per (sequence, head): codes 0x38 (1.0), scales 1"""
    n_head, n_kv, hd = HEADS
    dt = getattr(torch, dtype)
    rope = torch.zeros(SEQ, hd // 2, 2)
    rope[..., 0] = 1.0   # cos 1, sin 0
    c = {"slabs": torch.zeros(C.SPLIT, (n_head + 2 * n_kv) * hd, 8), "rope": rope.to(dt)}
    for name in ("k", "v"):
        c[name + "_codes"] = torch.full((B, n_kv, SEQ, hd), K.CODE_SENTINEL, dtype=torch.uint8)
        c[name + "_scales"] = torch.full((B, n_kv, SEQ), K.SCALE_SENTINEL, dtype=torch.float32)
        c[name + "_codes"][:, :, 0] = 0x38
        c[name + "_scales"][:, :, 0] = 1.0
    return c


def _row_scale(b, h):
    return 2.0 ** ((b + h) % 3 - 1)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_every_code_decodes_by_the_rule_in_v(dtype):
    L = _lib.load()
    runtime.init()
    n_head, n_kv, hd = HEADS
    B, dt = 8, getattr(torch, dtype)
    c = _decode_inputs(dtype, B)
    want = torch.zeros(n_head * hd, 8)
    seen = set()
    for b in range(B):
        for h in range(n_kv):
            idx = (np.arange(hd) + 67 * (b * n_kv + h)) % len(CODES)   # 4096 places: every code 16 times, in every byte of a word
            seen |= {(int(i), d % 4) for d, i in enumerate(idx)}
            c["v_codes"][b, h, 0] = torch.from_numpy(CODES[idx])
            c["v_scales"][b, h, 0] = _row_scale(b, h)
            want[h * hd:(h + 1) * hd, b] = torch.from_numpy(R.DECODE[CODES[idx]]) * _row_scale(b, h) / 2 + 0.0
    assert seen == {(i, k) for i in range(len(CODES)) for k in range(4)}   # (the conversion selects a byte pair of a 32-bit word)
    assert R.representable(want, dt)                                  # what must come out IS a 16-bit value: no rounding anywhere
    d = {k: v.to(DEV) for k, v in c.items()}
    yt = torch.full((n_head * hd, 8), 5.0, device=DEV, dtype=dt)
    rc = _launch_kv8(L, d, (1,) * B, 0xFF, B, HEADS, dtype, SEQ, d["k_codes"], d["v_codes"], d["k_scales"], d["v_scales"], yt)
    assert rc == 0
    # q = 0: both scores are 0, the weights are 1 and 1, l = 2; the new V row is +0: yt = float(code) * scale / 2 (a -0 code meets
    # the accumulator's +0 and leaves +0: the sign of a zero is the one thing this does not show)
    assert torch.equal(yt.cpu().view(torch.int16), want.to(dt).view(torch.int16))


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_every_code_decodes_by_the_rule_in_k(dtype):
    L = _lib.load()
    runtime.init()
    n_head, n_kv, hd = HEADS
    B, dt = 8, getattr(torch, dtype)
    covered = set()
    for j in range(4):
        c = _decode_inputs(dtype, B)
        idx = (np.arange(hd) + hd * j) % len(CODES)
        moved = torch.zeros(n_head, B, dtype=torch.bool)
        for b in range(B):
            for h in range(n_kv):
                c["k_codes"][b, h, 0] = torch.from_numpy(CODES[idx])
                c["k_scales"][b, h, 0] = _row_scale(b, h)
                dsel = h * B + b                                       # this (sequence, head) looks at code idx[dsel] alone
                val = float(R.DECODE[CODES[idx[dsel]]]) * _row_scale(b, h)
                covered.add(int(idx[dsel]))
                # q = Q at dsel, 0 elsewhere, Q a power of two with |Q * val| in [8, 16): the score Q * val / 8 has magnitude 1 .. 2
                Q = 1.0 if val == 0.0 else 2.0 ** (3 - int(np.floor(np.log2(abs(val)))))
                assert 2.0 ** -14 <= Q <= 2.0 ** 14
                c["slabs"][0, h * hd + dsel, b] = Q
                moved[h, b] = val != 0.0
        for name in ("k", "v"):   # the 16-bit caches of the dequantised rows
            dq = R.dequantize(c[name + "_codes"][:, :, :1], c[name + "_scales"][:, :, :1])
            assert R.representable(dq, dt)
            c[name + "_dq"] = torch.full((B, n_kv, SEQ, hd), C.SENTINEL, dtype=dt)
            c[name + "_dq"][:, :, :1] = dq.to(dt)
        d = {k: v.to(DEV) for k, v in c.items()}
        y16 = torch.full((n_head * hd, 8), 5.0, device=DEV, dtype=dt)
        assert C.launch(L, "slots", d["slabs"], d["rope"], (1,) * B, d["k_dq"], d["v_dq"], y16, B, HEADS, dtype, SEQ, runtime.stream_ptr(), 0xFF) == 0
        y8 = torch.full((n_head * hd, 8), 5.0, device=DEV, dtype=dt)
        assert _launch_kv8(L, d, (1,) * B, 0xFF, B, HEADS, dtype, SEQ, d["k_codes"], d["v_codes"], d["k_scales"], d["v_scales"], y8) == 0
        assert torch.equal(y8.view(torch.int16), y16.view(torch.int16)), j
        # the comparison can see the code: V is 1 in the cached row and 0 in the new one, so yt is the cached row's weight,
        # 1 / (1 + e^-s) — 1/2 exactly where the code is a zero, at least 0.23 away from it where the score has magnitude >= 1
        w = y8.float().cpu().view(n_head, hd, 8)
        assert bool((w == w[:, :1]).all())
        assert bool(((w[:, 0] - 0.5).abs() > 0.2)[moved].all()) and bool((w[:, 0] == 0.5)[~moved].all())
    assert covered == set(range(len(CODES)))
