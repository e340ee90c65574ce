"""The fp8 KV-cache row rule (include/teal_hip.h, "fp8 KV cache") restated in integers: the host model the kv8 tests compare the
device against.  Nothing here casts to an fp8 type; torch's cast is what tests/test_kv8_rule_host.py checks THIS against.

A row x[0 .. hd) of 16-bit values (fp16 / bf16 bit patterns), each exactly m * 2^q with an integer m:
    a = max |x_d|;  e = 0 if a == 0, else the smallest integer with a * 2^-e <= 448, clamped below at -100;  scale = 2^e
    code_d = RNE_e4m3fn(x_d * 2^-e): the e4m3fn grid has step 2^(k - 3) in the binade [2^k, 2^(k+1)), k >= -6, and step 2^-9 below
    2^-6; ties go to the even multiple of the step; the sign is kept (-0 -> 0x80).  |x_d * 2^-e| <= 448 = code 0x7E: no saturation.
    x'_d = float(code_d) * scale.
"""
import numpy as np
import torch

MIN_EXP = -100
FMT = {"float16": (5, 10), "bfloat16": (8, 7)}  # exponent bits, fraction bits


def _decompose(bits, dtype):
    """(sign, m, q) of 16-bit patterns: |value| = m * 2^q, m an integer below 2^11 (0 for +-0)"""
    eb, fb = FMT[dtype]
    b = np.asarray(bits).astype(np.int64) & 0xFFFF
    sign = b >> 15
    E = (b >> fb) & ((1 << eb) - 1)
    F = b & ((1 << fb) - 1)
    bias = (1 << (eb - 1)) - 1
    m = np.where(E == 0, F, F | (1 << fb))
    q = np.where(E == 0, 1 - bias - fb, E - bias - fb)
    return sign, m, q


def _bit_length(m):
    n = np.zeros_like(m)
    for i in range(12):
        n += (m >> i) > 0
    return n


def scale_exp(amax_bits, dtype):
    """e of the rule for the 16-bit pattern(s) of a row's largest magnitude"""
    _, m, q = _decompose(amax_bits, dtype)
    L = _bit_length(m)
    k = L - 1 + q                                   # floor(log2 a)
    fits = (m << 9) <= (448 << L)                   # a * 2^-(k - 8) = m * 2^(9 - L) <= 448
    e = np.where(fits, k - 8, k - 7)
    return np.where(m == 0, 0, np.maximum(e, MIN_EXP)).astype(np.int64)


def encode(bits, e, dtype):
    """e4m3fn codes (uint8) of the 16-bit patterns scaled by 2^-e (e broadcasts against bits); |value * 2^-e| <= 448 is the caller's"""
    sign, m, q = _decompose(bits, dtype)
    s = q - np.asarray(e, dtype=np.int64)           # value * 2^-e = m * 2^s
    ky = _bit_length(m) - 1 + s                     # floor(log2 |y|)
    t = np.maximum(ky - 3, -9)                      # the grid's step is 2^t
    sh = np.clip(t - s, -40, 20)                    # n = RNE(m * 2^(s - t)); m < 2^11, so a shift of 13 or more leaves 0
    up = m << np.maximum(-sh, 0)
    shr = np.maximum(sh, 0)
    half = np.where(shr > 0, (1 << np.maximum(shr - 1, 0)) - 1, 0)
    down = np.where(shr > 0, (m + half + ((m >> shr) & 1)) >> shr, m)
    n = np.where(sh <= 0, up, down)
    # normal: exponent field ky + 7, fraction n - 8 (n == 16 carries into the exponent); subnormal: the code is n (8 = 2^-6)
    mag = np.where(ky >= -6, ((ky + 7) << 3) + n - 8, n)
    mag = np.where(m == 0, 0, mag)
    assert int(mag.max(initial=0)) <= 0x7E, "a value above 448 after scaling"
    return (mag | (sign << 7)).astype(np.uint8)


def quantize_bits(bits, dtype):
    """rows [..., hd] of 16-bit patterns -> (codes uint8 [..., hd], e int64 [...])"""
    b = np.asarray(bits).astype(np.int64) & 0xFFFF
    e = scale_exp((b & 0x7FFF).max(axis=-1), dtype)
    return encode(b, e[..., None], dtype), e


def _decode_table():
    c = np.arange(256, dtype=np.int64)
    E, M = (c >> 3) & 15, c & 7
    mag = np.where(E == 0, np.ldexp(M.astype(np.float64), -9), np.ldexp((8 + M).astype(np.float64), E - 10))
    return np.where(c >> 7 == 1, -mag, mag).astype(np.float32)   # (0x7F / 0xFF, NaN in e4m3fn, never come out of encode)


DECODE = _decode_table()


def _dtype_name(dt):
    return {torch.float16: "float16", torch.bfloat16: "bfloat16"}[dt]


def quantize(x: torch.Tensor):
    """16-bit CPU tensor [..., hd] -> (codes uint8 [..., hd], scales fp32 [...]) by the rule"""
    bits = x.contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    codes, e = quantize_bits(bits, _dtype_name(x.dtype))
    scales = np.ldexp(np.ones(e.shape, dtype=np.float32), e.astype(np.int32))  # 2^e, e in -100 .. 120: exact in fp32
    return torch.from_numpy(np.asarray(codes)), torch.from_numpy(np.asarray(scales, dtype=np.float32))


def dequantize(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 [..., hd] = float(code) * scale (exact in fp32)"""
    vals = torch.from_numpy(DECODE[codes.cpu().numpy()])
    return vals * scales.cpu().to(torch.float32)[..., None]


def representable(x32: torch.Tensor, dt) -> bool:
    """every fp32 value survives the round trip through the 16-bit dtype"""
    return bool(torch.equal(x32.to(dt).to(torch.float32), x32))
