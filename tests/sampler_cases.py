"""The inputs of the sampler's oracle tests, generated on the host so that tests/test_sampler_rule.py (the model alone) and
tests/test_sampler_gpu.py (every kernel against the model) see the same bits.  numpy only.

A case is (law, top_k, temperature, seed); every case is drawn in two blocks (BLOCKS): 32 draws from counter 0, and 8 draws
from counter 2^32 - 4 of seed 2^32 + 5 (the kernels use the low 32 bits of both: the counter wraps to 0, the seed is 5).
"""
from functools import lru_cache

import numpy as np

from spec_rule import hash3, uniform

SEED = 1234
N_MAIN, N_WRAP = 32, 8
WRAP_SEED, WRAP_CTR = 2 ** 32 + 5, 2 ** 32 - 4
TEMPS = (1e-6, 0.8, 1.0, 2.0)  # 1e-6 is clamped to 1e-5: argmax, drawn at random among tied maxima

# vocabulary -> the kernel sample_launch picks (teal_sampler.hip), per entry point:
#   plain   teal_sample_topk (no workspace) and every call with top_k <= 0 or top_k >= vocab
#   ws      teal_sample_topk_ws / teal_sample_topk_slot with a prepared workspace and 0 < top_k < vocab
# (the slot entry point runs the *_slot_kernel form of the same choice)
VOCABS = {
    8:      "plain, ws: window NV = 4 — one vector, 1023 threads hold padding",
    1000:   "plain, ws: generic two-pass radix kernel (vocab % 8 != 0), scalar tail of 1000 - 992 = 8 logits after 124 vectors",
    4096:   "plain, ws: window NV = 4, partly filled (512 of 4096 vector slots)",
    8192:   "plain, ws: window NV = 4 — the largest single-chunk size, never multi",
    8200:   "plain: window NV = 4; ws: multi-workgroup, 2 chunks, the second holds 8 logits",
    32001:  "plain, ws: generic kernel, scalar tail of one logit",
    32768:  "plain: window NV = 4 at its limit; ws: multi-workgroup, 4 full chunks",
    32776:  "plain: window NV = 16 at its smallest; ws: multi-workgroup, 5 chunks, the last holds 8 logits",
    128256: "plain: window NV = 16; ws: multi-workgroup, 16 chunks, the last partial (5376 logits)",
    131072: "plain: window NV = 16 at its limit; ws: multi-workgroup at its limit, 16 full chunks",
    131080: "plain, ws: generic kernel — the first size past the window and multi-workgroup limits",
}
SMALL = tuple(v for v in VOCABS if v <= 8200)  # full cross product of laws x top_k x temperature
LARGE = tuple(v for v in VOCABS if v > 8200)   # the combinations that reach the named paths


def _to_bits(x: np.ndarray, bf16: bool) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    if not bf16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16).copy()
    w = x.view(np.uint32).astype(np.uint64)
    return (((w + 0x7FFF + ((w >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)  # round to nearest even (no NaN here)


def _thread(i):
    """the workgroup thread that holds vocabulary index i in the single-workgroup kernels (one 16-byte vector = 8 logits)"""
    return (i >> 3) & 1023


@lru_cache(maxsize=None)
def twin_case(V: int):
    """(seed, draw, i, j): the first seed >= SEED and draw < N_MAIN at which two vocabulary indices i < j held by different
    WAVES of the single-workgroup kernels (different threads where the vocabulary fits in one wave) get the same uniform.  With
    the two largest logits there and T -> 0 the race ties exactly at that draw and the smaller index must win: the input on
    which a tie-break that prefers the larger index in the cross-lane or cross-wave reduction shows."""
    idx = np.arange(V, dtype=np.uint64)
    apart = (lambda a, b: (_thread(a) >> 6) != (_thread(b) >> 6)) if V > 8 * 64 else (lambda a, b: _thread(a) != _thread(b))
    for seed in range(SEED, SEED + 100000):
        for d in range(N_MAIN):
            u = uniform(hash3(seed, d, idx))
            order = np.argsort(u, kind="stable")
            same = np.flatnonzero(u[order][1:] == u[order][:-1])
            for p in same:
                i, j = sorted((int(order[p]), int(order[p + 1])))
                if apart(i, j):
                    return seed, d, i, j
    raise AssertionError(f"no twin uniforms for V = {V}")


@lru_cache(maxsize=None)
def logits_bits(law: str, V: int, bf16: bool) -> np.ndarray:
    """the 16-bit patterns of one input law (read-only)"""
    g = np.random.default_rng([V, int(bf16), sum(map(ord, law))])
    if law == "normal":
        x = g.standard_normal(V) * 3
    elif law == "tiemax":  # a tie group straddling rank k: top_k = 20 and 40 equal maxima, all 40 must be drawable
        x = g.standard_normal(V) * 3
        x[np.linspace(0, V - 1, min(40, V // 2)).astype(np.int64)] = 20.0
    elif law == "flat":    # large k and a wide spread: the fp16 window widens through every sh step (3, 6, 8)
        x = (g.random(V) - 0.5) * 200
    elif law == "spike":
        x = g.standard_normal(V) * 0.01
        x[777 % V] = 60.0
    elif law == "fewvals":  # a few distinct values: thousands of ties at every pivot
        x = g.integers(-3, 4, V).astype(np.float64)
    elif law == "zeros":    # both zeros present, and pivots that land on zero: -0.0 and +0.0 are one value
        x = g.choice(np.array([-1.0, -0.0, 0.0, 1.0]), V, p=[0.3, 0.3, 0.3, 0.1])
    elif law == "tail":     # the last quarter of the vocabulary is -inf
        x = g.standard_normal(V) * 3
        x[V - V // 4:] = -np.inf
    elif law == "equal":
        x = np.full(V, 1.5)
    elif law == "onechunk":  # the 600 largest logits all inside chunk 1 (indices 8192 .. 16383) of a multi-chunk vocabulary
        assert V >= 16384
        x = g.standard_normal(V) * 0.5
        x[8192 + g.choice(8192, 600, replace=False)] = 10.0 + g.random(600) * 20
    elif law == "twins":
        _, _, i, j = twin_case(V)
        x = g.standard_normal(V) * 0.01
        x[i] = x[j] = 5.0
    else:
        raise KeyError(law)
    bits = _to_bits(x, bf16)
    bits.setflags(write=False)
    return bits


def top_ks(V: int):
    """{0, 1, 2, 20, 511, 512, 513, V - 1, V, V + 1}, clipped to what the vocabulary can tell apart"""
    return tuple(sorted({k for k in (0, 1, 2, 20, 511, 512, 513) if k < V} | {V - 1, V, V + 1}))


LAWS = ("normal", "tiemax", "flat", "spike", "fewvals", "zeros", "tail", "equal")


@lru_cache(maxsize=None)
def cases(V: int):
    """[(law, top_k, temperature, seed)] of one vocabulary size"""
    out = []
    if V in SMALL:
        out += [(law, k, T, SEED) for law in LAWS for k in top_ks(V) for T in TEMPS]
    else:
        out += [("normal", k, T, SEED) for k, T in ((0, 1.0), (1, 1.0), (2, 1e-6), (20, 0.8), (511, 0.8), (512, 2.0), (513, 1.0),
                                                    (5000, 2.0), (V - 1, 1.0), (V, 1.0), (V + 1, 0.8))]
        out += [("tiemax", 20, 1.0, SEED), ("tiemax", 20, 1e-6, SEED), ("tiemax", 0, 1e-6, SEED),
                ("flat", 20, 1.0, SEED), ("flat", 511, 2.0, SEED), ("flat", 5000, 2.0, SEED), ("flat", 0, 0.8, SEED), ("flat", V - 1, 2.0, SEED),
                ("spike", 20, 1.0, SEED), ("spike", 0, 2.0, SEED), ("spike", 1, 0.8, SEED),
                ("fewvals", 20, 1.0, SEED), ("fewvals", 513, 0.8, SEED), ("fewvals", 0, 1e-6, SEED),
                ("zeros", 20, 1.0, SEED), ("zeros", V // 8, 0.8, SEED), ("zeros", V // 2, 2.0, SEED),
                ("tail", 20, 0.8, SEED), ("tail", V - 1, 1.0, SEED), ("tail", V - V // 4 + 5, 1.0, SEED), ("tail", 0, 2.0, SEED),
                ("equal", 20, 1.0, SEED), ("equal", 0, 1e-6, SEED), ("equal", V - 1, 0.8, SEED)]
        if V >= 16384:
            out += [("onechunk", k, T, SEED) for k, T in ((20, 1.0), (511, 2.0), (512, 1.0), (513, 2.0), (600, 1.0), (700, 2.0))]
    if V >= 64:  # (below that one wave holds everything in a single vector per thread: no cross-lane tie to break)
        s = twin_case(V)[0]
        out += [("twins", 2, 1e-6, s), ("twins", 0, 1e-6, s), ("twins", 2, 0.8, s)]
    return tuple(out)


def blocks(seed: int):
    """(seed, first counter, draws) of the two blocks every case is drawn in"""
    return ((seed, 0, N_MAIN), (WRAP_SEED, WRAP_CTR, N_WRAP))
