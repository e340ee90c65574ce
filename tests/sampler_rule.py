"""Host model of the fused top-k sampler's draw (teal_sampler.hip: sample_topk*_kernel; gpt-fast/generate.py:49-66), numpy only.

What the kernels' comments promise, restated without the kernels' machinery:

  * logits are divided by max(T, 1e-5);
  * with 0 < top_k < V every logit that is not below the k-th largest VALUE stays eligible (ties at the pivot included), as
    `logits < pivot -> -inf` does in the reference — found here by np.partition on the decoded float64 values, not by the
    kernels' 16-bit keys, histograms or windows;
  * eligible index i scores exp((x_i - max) / T) / -log(u_i), u_i = ((hash3(seed, ctr, i) >> 8) + 0.5) / 2^24;
  * the token is the argmax, the smallest index winning exact ties; the draw counter then goes up by one.

hash3, uniform and order_key16 are spec_rule's (bit-exact restatements of teal_common.h); the draw is this module's.
tests/test_sampler_rule.py pins the model itself, tests/test_sampler_gpu.py holds every kernel and entry point to it.

NaN logits are out of scope: neither the kernels nor the reference define a draw from them.
"""
from functools import lru_cache

import numpy as np

from spec_rule import hash3, uniform

M32 = 0xFFFFFFFF
EPS = 1e-5


def decode(bits: np.ndarray, bf16: bool) -> np.ndarray:
    """16-bit patterns -> float32 (exact)"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    return (bits.astype(np.uint32) << 16).view(np.float32) if bf16 else bits.view(np.float16).astype(np.float32)


def kept_set(bits: np.ndarray, bf16: bool, top_k: int) -> np.ndarray:
    """boolean mask of the logits that stay eligible, by VALUE: everything when top_k <= 0 or top_k >= V, otherwise every
    logit not less than the k-th largest value (so +0.0 and -0.0, equal as values, are kept or dropped together)."""
    x = decode(bits, bf16).astype(np.float64)
    V = x.size
    if top_k <= 0 or top_k >= V:
        return np.ones(V, dtype=bool)
    pivot = np.partition(x, V - top_k)[V - top_k]
    return x >= pivot


@lru_cache(maxsize=6)
def _race_noise(seed32: int, ctr0: int, n: int, V: int):
    """(u [n][V] float32, -log(u) [n][V] float64) of draws ctr0 .. ctr0 + n - 1 (low 32 bits of each): a function of the stream
    and the vocabulary size alone, shared by every input, top_k and temperature that is drawn from it"""
    idx = np.arange(V, dtype=np.uint64)
    u = np.empty((n, V), dtype=np.float32)
    for j in range(n):
        u[j] = uniform(hash3(seed32, (ctr0 + j) & M32, idx))
    with np.errstate(divide="ignore"):
        e = -np.log(u.astype(np.float64))
    u.setflags(write=False)
    e.setflags(write=False)
    return u, e


def draws(bits: np.ndarray, bf16: bool, top_k: int, temperature: float, seed: int, ctr0: int, n: int, eps: float = EPS):
    """n consecutive draws, counters ctr0 .. ctr0 + n - 1 -> (token [n], runner_up [n], open [n]).

    Scores are float64 values of the kernel's fp32-exact inputs: u is spec_rule.uniform's fp32 value, (x - max) * inv_temp is
    rounded to fp32 once per operation as the kernel does, then exp, log and the division are float64.  Only the low 32 bits of
    seed and counter enter the hash, as in the kernel.

    token      the argmax, the smallest index winning exact ties.
    runner_up  the best index among those whose inputs (x_i, u_i) differ from the winner's; the winner itself if there is none.
               An index with the winner's very inputs gets the winner's very score on the device too, whatever its expf and logf
               round to, so there the smallest index must win and the twin is never a legitimate answer.
    open       runner_up's score is within eps (relative to the winner's) of the winner's: the device may return either.

    eps = 1e-5, the margin spec_rule.accept_numpy uses for the same race.  Why it suffices: the device's score is
    fl(expf(t) / -logf(u)) with t and u exact.  The ulp table of the HIP math API document is not part of a ROCm installation
    (only the runtime API's reference pages are), so no documented bound for expf and logf is quoted here and the margin stays
    the project's 1e-5.  What it covers: the library is built without fast-math, so the fp32 division is correctly rounded
    (0.5 ulp); if expf and logf are each within E ulps, and 1 ulp is at most 2^-23 relative, a device score is within
    (2 E + 0.5) * 2^-23 of the exact one and two scores can swap only if they are closer than twice that.  1e-5 >= 2 * (2 E +
    0.5) * 2^-23 holds up to E = 20, an order of magnitude more than device math libraries are usually given (1 to 2 ulps).
    (-logf(u) is no difference of nearly equal numbers: the error is relative to logf's own result, and u is either exactly 1
    or at most 1 - 2^-24.  expf results in the denormal range lose relative accuracy but never lead: the maximum scores 1 / e.)
    """
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    x = decode(bits, bf16)
    V = x.size
    inv = np.float32(1.0) / max(np.float32(temperature), np.float32(1e-5))
    idx = np.flatnonzero(kept_set(bits, bf16, top_k))
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((x[idx] - x.max()) * inv).astype(np.float32)  # two fp32 roundings, as written in the kernel
    pnum = np.exp(t.astype(np.float64))
    u_all, e_all = _race_noise(int(seed) & M32, int(ctr0) & M32, int(n), V)
    full = idx.size == V
    u = u_all if full else u_all[:, idx]
    e = e_all if full else e_all[:, idx]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = pnum[None, :] / e                     # [n][K]; u == 1 -> +inf (wins), 0 / 0 -> NaN (never considered)
    s = np.where(np.isnan(s), -1.0, s)
    rows = np.arange(n)
    w = np.argmax(s, axis=1)                      # first maximum = smallest index
    s1 = s[rows, w]
    twin = (t[None, :] == t[w][:, None]) & (u == u[rows, w][:, None])
    s2m = np.where(twin, -2.0, s)
    r = np.argmax(s2m, axis=1)
    s2 = s2m[rows, r]
    none = s2 < -1.5                              # every eligible index is a twin of the winner
    r = np.where(none, w, r)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isinf(s1), np.where(np.isinf(s2), 0.0, np.inf), s1 - s2)
        open_ = ~none & (gap <= eps * np.where(np.isinf(s1), 1.0, s1))
    return idx[w].astype(np.int64), idx[r].astype(np.int64), open_


def draw(bits: np.ndarray, bf16: bool, top_k: int, temperature: float, seed: int, ctr: int, eps: float = EPS):
    """one draw -> (token, runner_up, open); see draws()"""
    tok, ru, op = draws(bits, bf16, top_k, temperature, seed, ctr, 1, eps)
    return int(tok[0]), int(ru[0]), bool(op[0])


def premix(seed: int, ctr) -> np.ndarray:
    """the word hash3 has before the vocabulary index enters: a * C1 ^ f(b).  Two (seed, counter) pairs with equal words draw
    the same noise for every index."""
    a = np.uint64(int(seed) & M32)
    b = np.asarray(ctr, dtype=np.uint64) & np.uint64(M32)
    m = np.uint64(M32)
    return ((a * np.uint64(0x9E3779B1)) & m) ^ ((((b + np.uint64(0x7F4A7C15)) & m) * np.uint64(0x85EBCA77)) & m)
