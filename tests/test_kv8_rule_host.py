"""CPU: the fp8 KV cache of continuous batching (teal_kv8.hip, SlotDecodeEngine(kv_cache="fp8"), generate.py --kv_cache) — what needs
no GPU.

  * tests/kv8_rule.py (integers only) against torch.float8_e4m3fn casts over every fp16 and bf16 bit pattern in rows of fixed scale;
  * the scale choice at amax = 448 * 2^e and at the next 16-bit value above, amax = 0, the -100 clamp (bf16), -0, ties on both
    parities, results in the e4m3 subnormals;
  * the two entry points are exported and declared, and their unit builds for gfx950 with the library's flags, no scratch, no spills;
  * the preconditions of the GPU attention cases (tests/kv8_cases.py): every dequantised value is representable in the case's dtype
    (row maxima within 2^-6 .. 2^6), neighbouring rows' scales differ and a head's rows span at least 2^6;
  * the refusals that need no device: the keyword on the other engines, --kv_cache outside --requests.
"""
import os
import re

import numpy as np
import pytest
import torch

import kv8_cases as K
import kv8_rule as R
from teal_amd import _lib
from teal_amd.gpt_fast import generate as G
from test_continuous_host import _args, _resources

DTYPES = ("float16", "bfloat16")


def _all_patterns(dtype):
    bits = np.arange(1 << 16, dtype=np.int64)
    x = K._from_bits(bits, getattr(torch, dtype)).to(torch.float32)
    return bits, x


@pytest.mark.parametrize("dtype", DTYPES)
def test_rule_is_torchs_cast_on_every_bit_pattern(dtype):
    bits, x = _all_patterns(dtype)
    exps = (-8, -3, 0, 1, 3, 8) if dtype == "float16" else (-100, -40, -8, 0, 5, 60, 120)
    n = 0
    for e in exps:
        ok = torch.isfinite(x) & (x.abs() <= 448.0 * 2.0 ** e)
        y = x[ok].to(torch.float64) * 2.0 ** -e          # exact: a power-of-two factor, no underflow in fp64
        want = y.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        keep = (y.abs() >= 2.0 ** -120) | (y == 0)       # (below fp32's normals the product is not exact; the code is +-0 either way)
        got = R.encode(bits[ok.numpy()], e, dtype)
        assert np.array_equal(got[keep.numpy()], want[keep.numpy()]), (dtype, e)
        assert np.all((got[~keep.numpy()] & 0x7F) == 0)
        n += int(ok.sum())
    assert n > 100000


def test_decode_table_is_torchs():
    c = torch.arange(256, dtype=torch.uint8)
    want = c.view(torch.float8_e4m3fn).to(torch.float32)
    ok = ~torch.isnan(want)
    assert torch.equal(torch.from_numpy(R.DECODE)[ok], want[ok]) and int(ok.sum()) == 254
    assert torch.from_numpy(R.DECODE)[0x80].signbit() and R.DECODE[0x7E] == 448.0 and R.DECODE[1] == 2.0 ** -9


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_choice_at_the_boundary(dtype):
    dt = getattr(torch, dtype)
    for e in ((-9, -1, 0, 1, 7) if dtype == "float16" else (-99, -9, 0, 1, 7, 100)):
        a = torch.tensor([448.0 * 2.0 ** e], dtype=torch.float64).to(dt)
        assert a.to(torch.float64).item() == 448.0 * 2.0 ** e
        b = int(K._bits(a)[0])
        assert int(R.scale_exp(b, dtype)) == e           # exactly 448 * 2^e still fits
        assert int(R.scale_exp(b + 1, dtype)) == e + 1   # the next 16-bit value does not
        assert int(R.scale_exp(b - 1, dtype)) == e
    # the definition itself, over every finite positive pattern: a * 2^-e <= 448 < a * 2^-(e - 1), or the clamp
    bits, x = _all_patterns(dtype)
    pos = (bits < 0x8000) & torch.isfinite(x).numpy() & (x.numpy() > 0)
    e = R.scale_exp(bits[pos], dtype)
    a = x[torch.from_numpy(pos)].to(torch.float64).numpy()
    assert np.all(a * np.exp2(-e.astype(np.float64)) <= 448.0)
    free = e > R.MIN_EXP
    assert np.all(a[free] * np.exp2(-(e[free] - 1).astype(np.float64)) > 448.0)
    assert (e.min() == R.MIN_EXP) == (dtype == "bfloat16")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_crafted_rows(dtype, hd):
    rows = K.crafted_rows(dtype, hd)
    q = {n: R.quantize(r) for n, r in rows.items()}
    codes, scale = q["zeros"]
    assert not codes.any() and scale.item() == 1.0                                      # amax = 0: e = 0, every code +0
    codes, scale = q["negative zeros"]
    assert scale.item() == 1.0 and codes[:3].tolist() == [0x80, 0x00, 0x80] and bool((codes[3:] == 0x80).all())
    codes, scale = q["-0 beside values"]
    assert scale.item() == 1.0 and codes[:4].tolist() == [0x80, 0x44, 0xFE, 0x00]          # 3 = 1.5 * 2^1; -448
    codes, scale = q["ties both parities"]
    dq = R.dequantize(codes, scale)[:12].tolist()
    assert scale.item() == 1.0
    assert dq == [448.0, 16.0, -16.0, 20.0, -20.0, 20.0, 24.0, 1.0, 1.25, -1.0, 0.0, 2 * 2.0 ** -9]
    codes, scale = q["subnormal results"]
    assert scale.item() == 1.0
    assert codes[:12].tolist() == [0x7E, 0x04, 0x84, 0x03, 0x01, 0x00, 0x80, 0x01, 0x00, 0x80, 0x08, 0x08]   # (15 * 2^-10 = 7.5 steps: the tie goes up to 2^-6)
    for e in (-9, -1, 0, 1, 7):
        codes, scale = q[f"amax=448*2^{e}"]
        assert scale.item() == 2.0 ** e and codes[:3].tolist() == [0x7E, 0xF6, 0x38]    # 448, -224, 1
        codes, scale = q[f"amax=next above 448*2^{e}"]
        assert scale.item() == 2.0 ** (e + 1) and codes[1] == 0xF6                      # -448 * 2^e at the doubled scale: -224
    if dtype == "bfloat16":
        codes, scale = q["clamp at -100"]
        assert scale.item() == 2.0 ** -100 and codes[:3].tolist() == [0x00, 0x80, 0x00]
        codes, scale = q["just above the clamp"]
        assert scale.item() == 2.0 ** -100 and codes[:2].tolist() == [0x7E, 0x30]          # 448, 0.5
        codes, scale = q["bf16 subnormal"]
        assert scale.item() == 2.0 ** -100 and codes[:2].tolist() == [0x00, 0x80]
    # every row: the largest magnitude becomes a code in [224, 448], the row dequantises within half a step of itself
    for n, r in rows.items():
        codes, scale = q[n]
        x, dq = r.to(torch.float64), R.dequantize(codes, scale).to(torch.float64)
        if float(x.abs().max()) > 2.0 ** -90:
            assert 224.0 <= float(dq.abs().max() / scale.item()) <= 448.0, n
        step = torch.clamp(torch.exp2(torch.floor(torch.log2(torch.clamp(x.abs() / scale.item(), min=2.0 ** -6))) - 3), min=2.0 ** -9) * scale.item()
        assert bool(((x - dq).abs() <= step / 2).all()), n


def test_exports_match_the_header():
    hdr = open(os.path.join(_lib.INCLUDE, "teal_hip.h")).read()
    for name in ("teal_kv8_quantize_rows", "teal_batched_decode_attention_slots_kv8"):
        assert name in _lib.EXPORTS and name in _lib.OPTIONAL_WITH_OVERRIDE and re.search(r"\b%s\(" % name, hdr), name
    assert "teal_kv8.hip" in _lib.SOURCES
    decl = re.search(r"int teal_kv8_quantize_rows\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == 11
    decl = re.search(r"int teal_batched_decode_attention_slots_kv8\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == 19


def test_kv8_kernels_do_not_spill_to_scratch(tmp_path):
    res = _resources(tmp_path, "teal_kv8.hip")
    assert sum("kv8_quantize_rows" in n for n in res) == 4 and sum("batched_attention_kv8" in n for n in res) == 4, sorted(res)
    assert all(v == (0, 0) for v in res.values()), res


@pytest.mark.parametrize("case", K.attention_ids(), ids=lambda c: c[0])
def test_attention_case_preconditions(case):
    case_id, heads, dtype, B, pos, mask, max_seq = case
    dt = getattr(torch, dtype)
    c = K.attention_case(case_id, heads, dtype, B, pos, max_seq)
    assert c["k_exact"] and c["v_exact"]                       # every dequantised value is representable in the dtype
    for name in ("k16", "v16"):
        amax = c[name].to(torch.float32).abs().amax(-1)        # [B][n_kv][max_seq]
        assert float(amax.min()) >= 2.0 ** -6 and float(amax.max()) <= 2.0 ** 6
        assert float((amax.amax(-1) / amax.amin(-1)).min()) >= 2.0 ** 6      # a head's rows span at least 2^6
        _, scales = R.quantize(c[name])
        assert bool((scales[..., 1:] != scales[..., :-1]).all())            # neighbouring rows' scales differ
    for b, p in enumerate(pos):                                # what the launch may not touch holds the sentinels
        assert bool((c["k_codes"][b, :, p:] == K.CODE_SENTINEL).all()) and bool((c["v_scales"][b, :, p:] == K.SCALE_SENTINEL).all())


def test_engines_without_an_admission_refuse_the_keyword():
    from teal_amd.gpt_fast.batched import BatchedDecodeEngine, SlotDecodeEngine, kv_cache_refusal
    assert kv_cache_refusal("slot", None) is None and kv_cache_refusal("slot", "fp8") is None
    for kind in ("decode", "batched", "speculative", "tensor-parallel"):
        assert kv_cache_refusal(kind, None) is None
        assert "no admission" in kv_cache_refusal(kind, "fp8")
    assert "unknown" in kv_cache_refusal("slot", "fp4") and "unknown" in kv_cache_refusal("decode", "int8")
    with pytest.raises(ValueError, match="no admission"):
        BatchedDecodeEngine(None, [], 1, kv_cache="fp8")
    with pytest.raises(ValueError, match="unknown"):
        SlotDecodeEngine(None, [], 1, kv_cache="e5m2")
    from teal_amd.gpt_fast.engine import DecodeEngine
    with pytest.raises(ValueError, match="no admission"):
        DecodeEngine(None, [], kv_cache="fp8")
    from teal_amd.gpt_fast.speculative import SpeculativeDecoder
    with pytest.raises(ValueError, match="speculative decoding.*no admission"):
        SpeculativeDecoder(None, None, 4, 0.8, 50, False, 0, kv_cache="fp8")


@pytest.mark.parametrize("extra,msg", [
    (("--kv_cache", "fp8"), "--kv_cache.*--requests"),
    (("--kv_cache", "fp8", "--batch_size", "4"), "--kv_cache.*--requests"),
    (("--kv_cache", "fp8", "--self_speculate"), "--kv_cache.*--requests"),
])
def test_generate_refuses_kv_cache_without_requests(extra, msg):
    with pytest.raises(SystemExit, match=msg):
        G.main(_args("--synthetic", "tiny-test", *extra))


def test_kv_cache_flag():
    assert _args().kv_cache == "model" and _args("--kv_cache", "fp8").kv_cache == "fp8"
    with pytest.raises(SystemExit):
        _args("--kv_cache", "fp4")
