"""Host model of the per-request logit processors (teal_amd/csrc/teal_logit_adjust.hip), numpy only.

One row of `vocab` 16-bit logits l, the request's state row w (int32: bit 31 = the token occurs in the prompt, prefix included;
low 31 bits n = how often it was generated so far), its parameters {theta, alpha_p, alpha_f} and an optional bias row b:

    x = float32(l[v])
    w[v] != 0:   x = x / theta if x > 0 else x * theta          (the repetition rule of HF's RepetitionPenaltyLogitsProcessor)
    n > 0:       x = fl(x - fl(alpha_f * float32(n)));  x = fl(x - alpha_p)
    bias:        x = fl(x + float32(b[v]))
    z[v] = round-to-nearest-even to the dtype of min(max(x, -MAXF), +MAXF)

Every operation is one fp32 operation with its own rounding (numpy's float32 arithmetic is exactly that: no fused multiply-add),
so the kernel is held to this module BIT FOR BIT.  The output never holds an infinity.  NaN logits are outside the contract.

Counting: `count(state, token)` is what a launch with count_token != 0 does to a row before it adjusts the token's element.
"""
import numpy as np

PROMPT_BIT = np.int32(-2 ** 31)
COUNT_MASK = 0x7FFFFFFF
MAXF = {False: np.float32(65504.0), True: np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0]}


def decode(bits: np.ndarray, bf16: bool) -> np.ndarray:
    """16-bit patterns -> float32 (exact)"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    return (bits.astype(np.uint32) << 16).view(np.float32) if bf16 else bits.view(np.float16).astype(np.float32)


def encode(x: np.ndarray, bf16: bool) -> np.ndarray:
    """finite float32 -> 16-bit patterns, round to nearest even"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if not bf16:
        return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def count(state: np.ndarray, token: int) -> np.ndarray:
    """the state row after token `token` was counted once more (a copy); a token outside 0 .. vocab-1 counts nothing and the
    count stays at 2^31 - 1"""
    out = np.array(state, dtype=np.int32, copy=True)
    if 0 <= int(token) < out.size:
        w = int(out[token]) & 0xFFFFFFFF
        if w & COUNT_MASK != COUNT_MASK:
            w += 1
        out[token] = np.array([w], dtype=np.uint32).view(np.int32)[0]
    return out


def prompt_state(vocab: int, prompt_tokens) -> np.ndarray:
    """the state row of a request that has generated nothing yet"""
    w = np.zeros(vocab, dtype=np.int32)
    w[np.asarray(list(prompt_tokens), dtype=np.int64)] = PROMPT_BIT
    return w


def adjust(bits: np.ndarray, bf16: bool, state: np.ndarray, theta=1.0, alpha_p=0.0, alpha_f=0.0, bias_bits=None) -> np.ndarray:
    """the adjusted row as 16-bit patterns"""
    f32 = np.float32
    x = decode(bits, bf16)
    w = np.asarray(state, dtype=np.int32)
    n = (w.view(np.uint32) & np.uint32(COUNT_MASK)).astype(np.float32)  # (uint32 -> float32: round to nearest even)
    theta, alpha_p, alpha_f = f32(theta), f32(alpha_p), f32(alpha_f)
    with np.errstate(all="ignore"):
        rep = np.where(x > 0, (x / theta).astype(f32), (x * theta).astype(f32))
        x = np.where(w != 0, rep, x).astype(f32)
        prod = (alpha_f * n).astype(f32)                 # rounded on its own ...
        pen = ((x - prod).astype(f32) - alpha_p).astype(f32)  # ... before each of the two subtractions
        x = np.where(n > 0, pen, x).astype(f32)
        if bias_bits is not None:
            x = (x + decode(bias_bits, bf16)).astype(f32)
        x = np.minimum(np.maximum(x, -MAXF[bf16]), MAXF[bf16]).astype(f32)
    return encode(x, bf16)


def fused_frequency(x, alpha_f, n) -> np.float32:
    """what a contracted fma(-alpha_f, n, x) would give: ONE rounding of the exact x - alpha_f * n (float64 holds the product of
    two float32 values exactly, and the sum of it and a float32 to well below half an fp32 ulp for the magnitudes the tests use)"""
    return np.float32(np.float64(np.float32(x)) - np.float64(np.float32(alpha_f)) * np.float64(np.float32(n)))
