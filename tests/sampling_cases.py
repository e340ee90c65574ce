"""The inputs of the per-request sampling tests, generated on the host so that tests/test_sampling_rule_host.py (the model alone:
hand-worked counts, the share of open rows) and tests/test_sampling_gpu.py (teal_sample_rows against the model) see the same bits.
numpy only.

A parameter row is (temperature, top_k, top_p, min_p).  A configuration is a vocabulary, a dtype and a parameter row, run on the
N_ROWS random rows of that vocabulary and dtype; the model may call at most 15 % of a configuration's rows open.
"""
from functools import lru_cache

import numpy as np

from sampler_cases import _to_bits

SEED = 4321
N_ROWS = 8          # random rows per (vocabulary, dtype): one launch of B = 8
VOCABS = (8, 64, 8192, 8200, 32000, 128256, 131072)
CAP_VOCABS = (4096, 32000, 128256)  # where the share of open rows was surveyed before the GPU test's list was fixed

# eight different rows of settings (the B = 8 launch with a row of its own for every sequence); GRID: the configurations run on
# every random row.  T = 0.8 with top_p in {0.5, 0.9} and top_k in {0, 200} is the surveyed grid; the rest adds min_p, another
# temperature and the argmax limit.
MIXED = ((0.8, 0, 1.0, 0.0), (0.8, 200, 0.9, 0.0), (0.8, 0, 0.5, 0.0), (0.8, 0, 0.9, 0.0),
         (0.8, 200, 0.5, 0.0), (1.0, 50, 1.0, 0.05), (0.8, 0, 0.9, 0.02), (1.3, 20, 0.95, 0.1))
GRID = ((0.8, 0, 0.5, 0.0), (0.8, 0, 0.9, 0.0), (0.8, 200, 0.5, 0.0), (0.8, 200, 0.9, 0.0), (0.8, 0, 0.9, 0.02), (1.0, 50, 1.0, 0.05))


@lru_cache(maxsize=None)
def random_rows(V: int, bf16: bool, scale: float = 3.0) -> np.ndarray:
    """[N_ROWS][V] 16-bit patterns of randn * scale (read-only)"""
    g = np.random.default_rng([V, int(bf16), 77])
    bits = np.stack([_to_bits(g.standard_normal(V) * scale, bf16) for _ in range(N_ROWS)])
    bits.setflags(write=False)
    return bits


# hand-worked rows at V = 8: (name, logits, (temperature, top_k, top_p, min_p), kept count).  With T = 1 a logit x below a maximum of
# 4 weighs e^(x - 4): 1, .3679, .1353, .0498, .0183, .0067, .0025, .0009 for 4, 3, .., -3 (sum 1.5814).
LADDER = (4.0, 3.0, 2.0, 1.0, 0.0, -1.0, -2.0, -3.0)
HAND = (
    # 0.9 * 1.5814 = 1.4233; the mass above 4, 3, 2, 1 is 0, 1, 1.3679, 1.5032: the first three stay
    ("a boundary strictly inside", LADDER, (1.0, 0, 0.9, 0.0), 3),
    # Z = 1 + 3 * .3679 + .0498 + .0183 + .0067 + .0025 = 2.1809, 0.7 Z = 1.5266: above the three 3s lies 1 < 1.5266, so the class stays
    # WHOLE although the nucleus fills up inside it; above 1 lies 2.1036: dropped
    ("a boundary on a tie class", (4.0, 3.0, 3.0, 3.0, 1.0, 0.0, -1.0, -2.0), (1.0, 0, 0.7, 0.0), 4),
    # the others weigh e^-20 each: above them lies 1 >= 0.9 Z
    ("one dominant logit", (0.0, 0.0, 20.0, 0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 0, 0.9, 0.0), 1),
    ("all equal", (1.5,) * 8, (1.0, 0, 0.3, 0.0), 8),
    # top_k 6 keeps 6; top_p over those: Z = 1.5780, 0.99 Z = 1.5623, above 0 lies 1.5530 < 1.5623 < 1.5713 above -1: 5; min_p 0.2: 1, .3679
    ("min_p the strictest", LADDER, (1.0, 6, 0.99, 0.2), 2),
    # top_k 3; top_p over those: Z = 1.5032, 0.99 Z = 1.4882 > 1.3679: 3; min_p 0.01: down to .0183: 5
    ("top_k the strictest", LADDER, (1.0, 3, 0.99, 0.01), 3),
    # top_k 6; 0.7 * 1.5780 = 1.1046: above 3 lies 1, above 2 lies 1.3679: 2; min_p 0.01: 5
    ("top_p the strictest", LADDER, (1.0, 6, 0.7, 0.01), 2),
)


def hand_bits(values, bf16: bool) -> np.ndarray:
    return _to_bits(np.asarray(values, dtype=np.float32), bf16)


@lru_cache(maxsize=None)
def special_rows(V: int, bf16: bool):
    """(name, bits) of the degenerate rows at vocabulary V: -inf entries, and the most negative finite value as teal_logit_adjust
    leaves a banned or clamped logit"""
    g = np.random.default_rng([V, int(bf16), 78])
    x = g.standard_normal(V) * 3
    x[g.choice(V, V // 3, replace=False)] = -np.inf
    a = _to_bits(x, bf16)
    y = g.standard_normal(V) * 3
    b = _to_bits(y, bf16)
    b[g.choice(V, V // 2, replace=False)] = 0xFF7F if bf16 else 0xFBFF  # -MAXF
    eq = _to_bits(np.full(V, -2.25), bf16)
    spike = _to_bits(g.standard_normal(V) * 0.01, bf16)
    spike[V // 3] = _to_bits(np.array([40.0]), bf16)[0]
    return (("-inf entries", a), ("most negative finite", b), ("all equal", eq), ("one dominant logit", spike))
